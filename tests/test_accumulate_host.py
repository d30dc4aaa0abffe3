"""Gradient accumulation, the plumbing: a micro-batch is a rank that runs later.  The micro-batches'
gradients and statistics come from the oracle (as the ranks' do in tests/test_dp_gloo.py); the accumulation, the bucket's
hand-over, the ONE all-reduce and the division by the summed batch size are the product's Session.accumulate_grads /
reduce_accumulated on a ``device='cpu'`` session (tensor ops only, so they run here).  Bars: test_dp_gloo's, 5e-6 per
variable on the gradient and 2e-6 on the six statistics.  The HIP launch of the same arithmetic and the whole step are
covered on the GPU by tests/test_gpu_accumulate.py."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import load_pack
from test_dp_gloo import _free_port, _shard

D, T, PACK, SEED = 32, 2, "ragged_B6", 3
STAT_KEYS = ("loss", "acc", "TP", "FP", "TN", "FN")


@functools.lru_cache(maxsize=None)
def _oracle(lo, hi):
    """({statistic: float}, {variable: gradient of the mean loss of graphs lo .. hi-1, less the L2 term}): the L2 term is
    the optimiser kernel's, added after the reduction."""
    from oracle import params as P
    from oracle import torch_oracle as TO
    params = P.init_params(D, seed=SEED, perturb=True)
    out, grads = TO.loss_and_grads(params, _shard(load_pack(PACK, 0), lo, hi), T)
    return ({k: float(out[k].detach()) for k in STAT_KEYS},
            {k: grads[k] - TO.L2NORM_SCALING * params[k] for k in grads})


def _accumulate(sess, store, bounds):
    """One accumulate_grads per micro-batch bounds[k] .. bounds[k + 1], gradients and statistics from the oracle."""
    stats = None
    for k, (lo, hi) in enumerate(bounds):
        out, grads = _oracle(lo, hi)
        store.zero_grad()
        for name in store.names():
            store.grad_view(name).copy_(torch.from_numpy(grads[name]).float())
        stats = torch.tensor([out[key] for key in STAT_KEYS], dtype=torch.float32)
        before = store.grad.clone()
        sess.accumulate_grads(hi - lo, stats, first=(k == 0))
        assert torch.equal(store.grad, before)        # the micro-batch's gradient is only read
    return stats


def _check_against_whole_batch(got, stats):
    out, want = _oracle(0, 6)
    for i, k in enumerate(STAT_KEYS):
        assert abs(float(stats[i]) - out[k]) < 2e-6, (k, float(stats[i]), out[k])
    for k in want:
        scale = max(np.abs(want[k]).max(), 1e-12)
        assert np.abs(got[k] - want[k]).max() / scale < 5e-6, k


@pytest.mark.parametrize("split", [[0, 2, 6], [0, 4, 6], [0, 2, 4, 6], [0, 1, 2, 3, 4, 5, 6]])
def test_accumulated_shards_equal_the_global_batch(split):
    """Σ_k B_k · grad_k / Σ_k B_k is the gradient of the mean loss of the union; the singles cover B_k = 1 and K = 6."""
    import tspgnn
    model = tspgnn.build_network(D)
    sess = tspgnn.Session(model, device="cpu")
    store = model.store
    stats = _accumulate(sess, store, list(zip(split[:-1], split[1:])))
    sess.reduce_accumulated(stats)
    assert float(store.bucket[store.theta.numel()]) == 6.0
    _check_against_whole_batch(store.grad_dict(), stats)


def _worker(rank, world, port, plan, q):
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tsp-gnn_amd"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import tspgnn
    torch.set_num_threads(1)
    model = tspgnn.build_network(D)
    sess = tspgnn.Session(model, device="cpu")
    store = model.store
    calls = []
    all_reduce = dist.all_reduce

    def counted(tensor, *args, **kwargs):
        calls.append(tensor.numel())
        return all_reduce(tensor, *args, **kwargs)
    dist.all_reduce = counted
    try:
        stats = _accumulate(sess, store, plan[rank])
        sess.reduce_accumulated(stats)
    finally:
        dist.all_reduce = all_reduce
    q.put((rank, store.grad_dict(), stats.numpy().copy(), calls, store.theta.numel() + store.BUCKET_TAIL))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("plan", [([(0, 2), (2, 3)], [(3, 4), (4, 6)]),
                                  ([(0, 2)], [(2, 3), (3, 4), (4, 6)])], ids=["2+2", "1+3"])
def test_two_gloo_ranks_accumulate_then_reduce_once(plan):
    """Two ranks, each with micro-batches of its own (their numbers need not agree): ONE all-reduce, of the bucket, per
    rank and step, and every rank ends with the gradient and the statistics of the global batch."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, plan, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in results) == [0, 1]
    for rank, got, stats, calls, bucket_floats in results:
        assert calls == [bucket_floats], (rank, calls)
        _check_against_whole_batch(got, stats)


def test_an_empty_step_is_refused():
    import tspgnn
    sess = tspgnn.Session(tspgnn.build_network(D), device="cpu")
    with pytest.raises(ValueError, match="at least one micro-batch"):
        sess.train_step_accumulated([])


def test_first_discards_what_the_buffer_held():
    """``first=True`` writes: a buffer full of NaN (never written, or left by a diverged step) does not reach the sum."""
    import tspgnn
    model = tspgnn.build_network(D)
    sess = tspgnn.Session(model, device="cpu")
    store = model.store
    store.accum_bucket().fill_(float("nan"))
    stats = _accumulate(sess, store, [(0, 2), (2, 6)])
    assert bool(torch.isfinite(store.accum).all())
    sess.reduce_accumulated(stats)
    _check_against_whole_batch(store.grad_dict(), stats)
