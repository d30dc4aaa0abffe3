"""bench.py's N-rank path without a GPU: `--plumbing --gpus 8` under gloo on the loopback address -- the launcher (bench.py
spawns its own ranks through torch.distributed.run when WORLD_SIZE is unset, as the driver's `--gpus N` call does), the
rendezvous, shards of unequal size, the data-parallel bucket's ONE all-reduce with B_r / B weights (the Session code the
GPU path runs), barrier-bracketed timing with the max over ranks, rank 0 printing ONE JSON line with the driver's keys."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ranks", [8, 2])
def test_bench_plumbing_json_contract(ranks):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--plumbing", "--gpus", str(ranks), "--steps", "4",
                          "--warmup", "1"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]            # rank 0 alone prints
    r = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "rccl_ranks", "allreduce_us"):
        assert key in r, key
    assert r["plumbing"] is True and "PLUMBING" in r["metric"]
    assert "all-reduce" in r["value_is"]      # N > 1: the headline carries the collective (the GPU line: the training step)
    assert r["n_gpus"] == ranks and r["rccl_ranks"] == ranks and r["backend"] == "gloo"
    assert r["steps"] == 4 and r["warmup"] == 1 and r["scaling"] == "weak" and r["higher_is_better"] is True
    assert r["reduced_gradient_ok"] is True                # sum_r B_r (r + 1) / sum_r B_r on every rank
    assert r["allreduce_bytes"] == 4 * (31353 + 10) or r["allreduce_bytes"] > 4 * 10
    assert r["value"] > 0 and abs(r["value"] - ranks * 2 * 1e3 / r["ms_per_step"]) / r["value"] < 1e-3


def test_dump_outputs_writes_float32_and_a_fixed_row_sample(tmp_path):
    """bench.py --dump-outputs: every array of a step's output dict as <name>.npy in float32 (bf16 states widened); state
    arrays longer than DUMP_MAX_ROWS keep the same seeded rows on every call, and the rows kept are the rows computed."""
    import torch
    import bench
    from tspgnn.graphnn import LSTMStateTuple
    M, N, d, B = bench.DUMP_MAX_ROWS + 77, 40, 8, 3
    g = torch.Generator().manual_seed(3)
    Eh = torch.randn(M, d, generator=g)
    out = {"predictions": torch.rand(B, generator=g), "logits": torch.randn(B, generator=g), "E_vote": torch.randn(M, generator=g),
           "stats": torch.rand(6, generator=g), "range_guard": torch.zeros(4, dtype=torch.int32),
           "last_states": {"E": LSTMStateTuple(c=torch.randn(M, d, generator=g), h=Eh.to(torch.bfloat16)),
                           "V": LSTMStateTuple(c=torch.randn(N, d, generator=g), h=torch.randn(N, d, generator=g))}}
    theta = torch.randn(100, generator=g)
    sampled = bench.dump_outputs(out, theta, str(tmp_path / "a"))
    assert bench.dump_outputs(out, theta, str(tmp_path / "b")) == sampled
    assert sampled == {"last_states_E_c": [bench.DUMP_MAX_ROWS, M], "last_states_E_h": [bench.DUMP_MAX_ROWS, M]}
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(n + ".npy" for n in ("predictions", "logits", "E_vote", "stats", "last_states_E_c",
                                                "last_states_E_h", "last_states_V_c", "last_states_V_h", "variables"))
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b), n
    assert np.array_equal(np.load(tmp_path / "a" / "variables.npy"), theta.numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "last_states_V_h.npy"), out["last_states"]["V"].h.numpy())
    Eh_kept = np.load(tmp_path / "a" / "last_states_E_h.npy")
    Eh_all = Eh.to(torch.bfloat16).float().numpy()
    rows = [int(np.flatnonzero((Eh_all == r).all(axis=1))[0]) for r in Eh_kept[:50]]
    assert rows == sorted(rows) and len(set(rows)) == len(rows)   # distinct rows of the computed array, in order
