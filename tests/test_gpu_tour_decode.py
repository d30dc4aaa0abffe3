"""tspgnn_tour_from_votes on the GPU (csrc/tour_decode.hip, tspgnn.decode) against the NumPy restatement of
tests/decode_reference.py: tours and n_missing exactly, costs bit for bit (the summation order is defined and there is no
FMA), at the sizes where the kernel changes shape -- one wave up to n = 64, four up to 128, sixteen up to 256 -- and on the
inputs where ties, special values, stranded fragments and empty instances decide.  Then the Python surface end to end on
the trained weights of tests/golden/trained_d64.npz.  Nothing here claims that decoded tours are good."""
import functools
import os

import numpy as np
import pytest
import torch

import decode_cases as cases
import decode_reference as ref
import tspgnn
from conftest import GOLDEN
from tspgnn import _lib, decode

pytestmark = pytest.mark.gpu

SENTINEL = -77


def launch(case, n_max=None, dev="cuda:0"):
    """The raw entry point on a decode_cases batch -> (status, tours, costs as uint32 bits, n_missing), outputs prefilled
    with SENTINEL."""
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dev) for k in ("vote", "uv", "wc", "seg", "vseg")}
    if case["vote"].size == 0:
        t["vote"], t["uv"], t["wc"] = (torch.zeros(s, dtype=d, device=dev) for s, d in
                                       (((1,), torch.float32), ((1, 2), torch.int32), ((1, 2), torch.float32)))
    B, N = len(case["n"]), int(case["vseg"][-1])
    tours = torch.full((N,), SENTINEL, dtype=torch.int32, device=dev)
    costs = torch.full((B,), float(SENTINEL), dtype=torch.float32, device=dev)
    missing = torch.full((B,), SENTINEL, dtype=torch.int32, device=dev)
    status = _lib.lib.tspgnn_tour_from_votes(_lib.ptr(t["vote"]), _lib.ptr(t["uv"]), _lib.ptr(t["wc"]), _lib.ptr(t["seg"]),
                                             _lib.ptr(t["vseg"]), B, int(case["n"].max()) if n_max is None else n_max,
                                             _lib.ptr(tours), _lib.ptr(costs), _lib.ptr(missing), _lib.current_stream())
    torch.cuda.synchronize()
    return status, tours.cpu().numpy(), costs.cpu().numpy().view(np.uint32), missing.cpu().numpy()


@functools.lru_cache(maxsize=None)
def expected(name, *args):
    return ref.decode_batch(getattr(cases, name)(*args))


def check(case, want, n_max=None):
    status, tours, costs, missing = launch(case, n_max)
    assert status == 0, _lib.lib.tspgnn_last_error()
    for b, (tour, miss, cost, _) in enumerate(want):
        got = [int(v) for v in tours[case["vseg"][b]:case["vseg"][b + 1]]]
        assert got == tour, (b, int(case["n"][b]))
        assert int(missing[b]) == miss, b
        assert int(costs[b]) == int(np.float32(cost).view(np.uint32)), (b, costs[b:b + 1].view(np.float32), cost)


@pytest.mark.parametrize("n", [4, 5, 40, 64, 65, 128, 129, 256])
def test_complete_graphs(cuda_device, n):
    want = expected("complete_case", n)
    assert want[0][1] == 0 and want[0][3] == 1      # a complete graph: one Hamiltonian path, a feasible tour
    check(cases.complete_case(n), want)


def test_all_votes_equal(cuda_device):
    check(cases.ties_case(), expected("ties_case"))


def test_special_votes(cuda_device):
    check(cases.special_case(), expected("special_case"))


def test_sparse_graphs_strand(cuda_device):
    want = expected("sparse_case")
    assert tuple((w[1], w[3]) for w in want) == cases.SPARSE_OUTCOME    # several paths, and one unclosed path
    check(cases.sparse_case(), want)


def test_untouched_vertex_no_edges_bad_edges_and_surplus_edges(cuda_device):
    want = expected("odd_case")
    assert want[1][0] == list(range(6)) and want[1][1] == 6
    check(cases.odd_case(), want)


def test_ragged_batch_equals_each_instance_alone(cuda_device):
    want = expected("ragged_case")
    check(cases.ragged_case(), want)
    check(cases.ragged_case(), want, n_max=256)
    for k, inst in enumerate(cases.ragged_instances()):
        alone = cases.batch([inst])
        check(alone, [want[k]])
        if inst[0] <= 128:
            check(alone, [want[k]], n_max=2 * inst[0] + 1)      # another workgroup shape, the same result


def test_refusals_leave_the_outputs_untouched(cuda_device):
    case = cases.complete_case(5)
    for n_max, code in ((257, -2), (3, -1)):
        status, tours, costs, missing = launch(case, n_max)
        assert status == code
        assert (tours == SENTINEL).all() and (missing == SENTINEL).all()
        assert (costs.view(np.float32) == SENTINEL).all()
    out = torch.full((5,), SENTINEL, dtype=torch.int32, device="cuda:0")
    p = _lib.ptr(out)
    assert _lib.lib.tspgnn_tour_from_votes(None, p, p, p, p, 1, 5, p, p, p, _lib.current_stream()) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()


# ------------------------------------------------------------------------------------------- the Python surface

T = 8


@functools.lru_cache(maxsize=None)
def trained():
    z = np.load(os.path.join(GOLDEN, "trained_d64.npz"))
    model = tspgnn.build_network(64)
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer())
    model.store.load({k: z[k].astype(np.float64) for k in z.files})
    rng = np.random.RandomState(5)
    instances = [tspgnn.random_instance(20, rng) for _ in range(5)]
    return model, sess, instances


@functools.lru_cache(maxsize=None)
def decoded():
    model, sess, instances = trained()
    targets = [r[0] for r in tspgnn.get_costs(sess, model, instances, T)]
    return targets, tspgnn.decode_tours(sess, model, instances, T, polish=True)


def test_decode_tours_end_to_end(cuda_device):
    model, sess, instances = trained()
    targets, res = decoded()
    labels = tspgnn.label_tours([(Ma, Mw) for Ma, Mw, _ in instances], lower_bound=False)
    for (Ma, Mw, _), r, target, lab in zip(instances, res, targets, labels):
        n = Ma.shape[0]
        assert sorted(r.tour) == list(range(n)) and r.tour[0] == 0 and r.tour[1] < r.tour[-1]
        A = (Ma + Ma.T) != 0
        pairs = list(zip(r.tour, r.tour[1:] + r.tour[:1]))
        assert r.n_missing == sum(1 for a, b in pairs if not A[a, b])
        assert r.feasible == (r.n_missing == 0)
        cost = np.float32(0)
        for a, b in pairs:
            if A[a, b]:
                cost = np.float32(cost + np.float32(Mw[min(a, b), max(a, b)]))
        assert np.float32(r.cost) == cost
        assert r.target_cost == target and 0.0 <= r.prediction <= 1.0
        # the descent starts from the decoded tour and only ever takes improving moves in fp32: the fp64 cost of its
        # result may exceed the start's fp32 sum by rounding alone, n additions of relative error 2^-24 each
        assert sorted(r.polished_tour) == list(range(n))
        assert r.polished_cost <= r.cost * (1 + 2 * n * 2.0 ** -24)
        print("n=%d decoded %.4f  polished %.4f  label %.4f  decoded/label %.3f  polished/label %.3f  missing %d"
              % (n, r.cost, r.polished_cost, lab.cost, r.cost / lab.cost, r.polished_cost / lab.cost, r.n_missing))


def test_own_estimate_equals_explicit_targets(cuda_device):
    model, sess, instances = trained()
    targets, res = decoded()
    again = tspgnn.decode_tours(sess, model, instances, T, target_costs=targets, max_graphs=2)   # three chunks
    for a, b in zip(res, again):
        assert a.tour == b.tour and a.cost == b.cost and a.n_missing == b.n_missing and a.target_cost == b.target_cost
        assert b.polished_tour is None and b.polished_cost is None
    with pytest.raises(ValueError):
        tspgnn.decode_tours(sess, model, [tspgnn.random_instance(3, np.random.RandomState(0))], T, target_costs=[0.1])


def test_decoded_tour_curve_is_the_baseline_arithmetic_on_the_decoded_tours(cuda_device):
    from tspgnn import dataset, experiments
    model, sess, instances = trained()
    _, res = decoded()
    devs = [0.02, 0.5, 2.0]
    Q = [dataset._target(Ma, Mw, route) for Ma, Mw, route in instances]
    for polish, cost in ((False, [r.cost for r in res]), (True, [r.polished_cost for r in res])):
        got = experiments.decoded_tour_curve(sess, model, instances, T, devs, polish=polish)
        want = experiments.curve_from_costs(cost, [True] * len(res), Q, devs)     # complete graphs: all feasible
        assert sorted(got) == ["acc", "deviations", "fpr", "tpr"]
        for k in ("tpr", "fpr", "acc"):
            assert np.array_equal(got[k], want[k]), (polish, k)


def test_tours_from_votes_without_a_host_synchronisation(cuda_device):
    model, sess, instances = trained()
    EV, W, C, route_exists, n_vertices, n_edges = tspgnn.InstanceLoader.create_batch(instances, target_cost=0.2)
    feed = {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: T, model["route_exists"]: route_exists,
            model["n_vertices"]: n_vertices, model["n_edges"]: n_edges}
    b = sess.prepare(feed)
    out = sess.forward_device(b)
    torch.cuda.synchronize()
    slow = tspgnn.tours_from_votes(b, out["E_vote"])
    torch.cuda.synchronize()
    want = [x.cpu().numpy() for x in slow[:3]]
    votes = out["E_vote"].cpu().numpy()
    out = sess.forward_device(b)                        # enqueued, not waited for
    fast = tspgnn.tours_from_votes(b, out["E_vote"])    # behind it on the same stream
    got = [x.cpu().numpy() for x in fast[:3]]
    assert np.array_equal(out["E_vote"].cpu().numpy(), votes)
    assert all(np.array_equal(g.view(np.int32), w.view(np.int32)) for g, w in zip(got, want))
    case = {"n": n_vertices.astype(np.int32), "seg": b.seg.cpu().numpy(), "vseg": fast.vseg.cpu().numpy(), "uv": EV.uv,
            "wc": b.WC.cpu().numpy(), "vote": votes}
    for k, (tour, miss, cost, _) in enumerate(ref.decode_batch(case)):
        v0 = case["vseg"][k]
        assert [int(v) for v in got[0][v0:v0 + 20]] == tour and int(got[2][k]) == miss
        assert got[1][k:k + 1].view(np.uint32)[0] == np.float32(cost).view(np.uint32)
    assert decode.vote_key(votes).dtype == np.uint32
