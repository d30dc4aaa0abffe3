"""Exact tour labels on the GPU (tspgnn.dataset.prove_tours on csrc/tour_exact.hip): optima against the Held-Karp DP from
bad incumbents, the bound's validity when the node budget runs out, the root's bit-identity with
tspgnn_tour_lower_bound, the lane-ownership edges, determinism across calls and chunkings, the proved fraction at the
reference's training shape, and create_dataset(exact=True) end to end."""
import filecmp
import os
import random

import numpy as np
import pytest
import torch

from test_gpu_tour_solver import _check_tour, _instances, _w, held_karp
from test_tour_exact_host import int_family
from tspgnn import _lib, dataset

pytestmark = pytest.mark.gpu

# Measured 1.0000 (512 of 512) on the MI355X with the defaults (nodes p50 1, p90 36, p99 453, max 1 002 of
# the 2 048 allowed).  The floor is the measured fraction less 3.5 binomial standard deviations at 512 instances, and at
# p = 1 that deviation is 0: the run is deterministic, so a change of the solver or its defaults that loses an instance
# to the budget shows here.
PROVED_MIN = 1.0


def _incumbent(Ma, Mw, tour):
    """A TourResult that carries `tour` as the incumbent (prove_tours reads its tour and its feasibility)."""
    tour = [int(x) for x in tour]
    w = _w(Ma, Mw)
    pairs = list(zip(tour, tour[1:] + tour[:1]))
    feasible = all(np.isfinite(w[a, b]) for a, b in pairs)
    return dataset.TourResult(tour, float("nan"), float("nan"), feasible, float("nan"))


def _uniform(rng, sizes):
    """Complete graphs with independent uniform weights: not metric."""
    return [(np.triu(np.ones((n, n)), 1), np.triu(rng.rand(n, n), 1)) for n in sizes]


@pytest.fixture(scope="module")
def small_families():
    """kind -> (instances, incumbents, DP optima): 48 instances of n 5-13 each; the integer family also has one n = 4."""
    rng = np.random.RandomState(30)
    fam = {}
    insts, _ = _instances(rng, rng.randint(5, 14, size=48), "euc")
    fam["euc"] = (insts, [list(range(Ma.shape[0])) for Ma, _ in insts])
    insts = _uniform(rng, rng.randint(5, 14, size=48))
    fam["uniform"] = (insts, [list(range(Ma.shape[0])) for Ma, _ in insts])
    fam["sparse"] = _instances(rng, rng.randint(5, 14, size=48), "sparse")
    fam["int"] = int_family(rng, list(rng.randint(5, 14, size=48)) + [4])
    return {k: (insts, [_incumbent(Ma, Mw, t) for (Ma, Mw), t in zip(insts, tours)],
                [held_karp(_w(Ma, Mw)) for Ma, Mw in insts]) for k, (insts, tours) in fam.items()}


@pytest.mark.parametrize("kind", ["euc", "uniform", "sparse", "int"])
def test_optimum_from_a_bad_incumbent(cuda_device, small_families, kind):
    insts, incs, opts = small_families[kind]
    stats = {}
    res = dataset.prove_tours(insts, incs, stats=stats)
    print("%s: nodes > 1 on %.2f, max %d" % (kind, np.mean(stats["nodes"] > 1), stats["nodes"].max()))
    for (Ma, Mw), r, opt, st in zip(insts, res, opts, stats["status"]):
        _check_tour(r, Ma, Mw)
        assert st == "proved" and r.feasible
        assert abs(r.cost - opt) <= 1e-9 * opt, (r.cost, opt)
        assert r.lb <= opt and opt - r.lb <= 2e-6 * opt, (r.lb, opt)
    if kind == "int":   # otherwise this says nothing about branching
        assert np.mean(stats["nodes"] > 1) >= 1.0 / 3.0


def test_bound_is_valid_when_the_budget_runs_out(cuda_device, small_families):
    insts, incs, opts = small_families["int"]
    prev = np.full(len(insts), -np.inf)
    for max_nodes in (1, 2, 3, 5, 9):
        stats = {}
        res = dataset.prove_tours(insts, incs, max_nodes=max_nodes, stats=stats)
        lb = np.array([r.lb for r in res])
        assert np.all(lb <= np.array(opts))
        assert np.all(lb >= prev), max_nodes
        assert np.all(stats["nodes"] >= 1) and np.all(stats["nodes"] <= max_nodes)
        assert set(stats["status"]) <= {"proved", "budget"}
        prev = lb


def test_root_is_the_bound_kernel_bit_for_bit(cuda_device):
    rng = np.random.RandomState(31)
    sizes = [4, 63, 64, 65, 127, 128] + [int(x) for x in rng.randint(5, 129, size=26)]
    ns = np.array(sizes, dtype=np.int32)
    Ws, upper = [], []
    for n in sizes:
        p = rng.rand(n, 2)
        Mw = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
        W = dataset._penalised(np.ones((1, n, n), bool) & ~np.eye(n, dtype=bool), Mw[None])[0]
        Ws.append(W.reshape(-1))
        upper.append(np.float32(W[np.arange(n), np.roll(np.arange(n), -1)].astype(np.float64).sum()))
    dev = cuda_device
    d_W = torch.from_numpy(np.concatenate(Ws)).to(dev)
    d_woff = torch.from_numpy(np.concatenate([[0], np.cumsum(ns.astype(np.int64) ** 2)[:-1]])).to(dev)
    d_toff = torch.from_numpy(np.concatenate([[0], np.cumsum(ns.astype(np.int64))[:-1]])).to(dev)
    d_n = torch.from_numpy(ns).to(dev)
    d_up = torch.from_numpy(np.array(upper, dtype=np.float32)).to(dev)
    d_tours = torch.from_numpy(np.concatenate([np.arange(n, dtype=np.int32) for n in sizes])).to(dev)
    G = len(sizes)
    d_lb0 = torch.empty(G, dtype=torch.float64, device=dev)
    d_lb1 = torch.empty(G, dtype=torch.float64, device=dev)
    d_nodes = torch.empty(G, dtype=torch.int32, device=dev)
    d_stat = torch.empty(G, dtype=torch.int32, device=dev)
    d_ws = torch.empty(int(_lib.lib.tspgnn_tour_branch_bound_ws(G, 128)), dtype=torch.uint8, device=dev)
    st = _lib.current_stream()
    _lib.call("tspgnn_tour_lower_bound", _lib.ptr(d_W), _lib.ptr(d_woff), _lib.ptr(d_n), _lib.ptr(d_up), G, 128, 400,
              _lib.ptr(d_lb0), st)
    _lib.call("tspgnn_tour_branch_bound", _lib.ptr(d_W), _lib.ptr(d_woff), _lib.ptr(d_n), _lib.ptr(d_toff), _lib.ptr(d_up),
              G, 128, 400, 30, 1, 1e-9, _lib.ptr(d_ws), _lib.ptr(d_tours), _lib.ptr(d_lb1), _lib.ptr(d_nodes),
              _lib.ptr(d_stat), st)
    torch.cuda.synchronize(dev)
    lb0, lb1 = d_lb0.cpu().numpy(), d_lb1.cpu().numpy()
    assert np.all(np.isfinite(lb0)) and np.all(lb0 > 0)
    assert np.array_equal(lb0.view(np.int64), lb1.view(np.int64))
    assert np.all(d_nodes.cpu().numpy() == 1)
    assert set(d_stat.cpu().numpy().tolist()) <= {0, 1}


def test_n14_18_proved_from_a_single_descent(cuda_device):
    rng = np.random.RandomState(21)
    insts, inits = _instances(rng, [14, 16, 18], "euc")
    a, b = _instances(rng, [15, 17], "sparse")
    insts += a
    inits += b
    start = dataset.solve_tours(insts, init_tours=inits, restarts=1, kicks=0)
    stats = {}
    res = dataset.prove_tours(insts, start, stats=stats)
    assert list(stats["status"]) == ["proved"] * 5
    for (Ma, Mw), r in zip(insts, res):
        _check_tour(r, Ma, Mw)
        opt = held_karp(_w(Ma, Mw))
        assert abs(r.cost - opt) <= 1e-9 * opt, (r.cost, opt)
        assert r.lb <= opt


@pytest.mark.parametrize("n", [64, 65, 128])
def test_convex_position_at_the_lane_ownership_edges(cuda_device, n):
    """A lane owns vertices l and l + 64: n = 64, 65 and 128 are where the second slot is empty, holds one vertex, and is
    full.  Points in convex position have the hull order as their only optimal tour."""
    rng = np.random.RandomState(n)
    th = 2 * np.pi * (np.arange(n) + 0.3 * rng.rand(n)) / n
    p = 0.5 + 0.5 * np.stack([np.cos(th), np.sin(th)], axis=1)
    Mw = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
    Ma = np.triu(np.ones((n, n)), 1)
    stats = {}
    (r,) = dataset.prove_tours([(Ma, Mw)], [_incumbent(Ma, Mw, rng.permutation(n))], stats=stats)
    print("n=%d: %d nodes, %s" % (n, stats["nodes"][0], stats["status"][0]))
    assert r.tour == list(range(n))
    assert stats["status"][0] == "proved"


def test_deterministic_across_calls_and_chunks(cuda_device):
    rng = np.random.RandomState(32)
    sizes = rng.randint(20, 61, size=48)
    insts, inits = _instances(rng, sizes[:32], "euc")
    a, b = _instances(rng, sizes[32:], "sparse")
    insts += a
    inits += b
    start = dataset.solve_tours(insts, init_tours=inits, seed=3, lower_bound=False)
    s1, s2, s3, s4 = {}, {}, {}, {}
    r1 = dataset.prove_tours(insts, start, stats=s1)
    r2 = dataset.prove_tours(insts, start, stats=s2)
    r3 = dataset.prove_tours(insts, start, stats=s3, chunk=7)
    assert r1 == r2 == r3
    for s in (s2, s3):
        assert np.array_equal(s["status"], s1["status"]) and np.array_equal(s["nodes"], s1["nodes"])
    for (Ma, Mw), r in zip(insts, r1):
        _check_tour(r, Ma, Mw)
        assert r.lb <= r.cost
    half = dataset.prove_tours(insts[24:], start[24:], stats=s4)
    assert half == r1[24:]
    assert np.array_equal(s4["status"], s1["status"][24:]) and np.array_equal(s4["nodes"], s1["nodes"][24:])


def test_proved_fraction_n20_40(cuda_device):
    np.random.seed(24)
    random.seed(24)
    graphs = dataset.draw_instances(20, 40, samples=512)
    insts, inits = [(g[0], g[1]) for g in graphs], [g[2] for g in graphs]
    plain = dataset.solve_tours(insts, init_tours=inits)
    stats = {}
    res = dataset.label_tours(insts, init_tours=inits, exact=True, stats=stats)
    proved = stats["status"] == "proved"
    gap = np.array([(r.cost - r.lb) / r.cost for r in res])
    nd = stats["nodes"]
    print("proved fraction %.4f (%d of 512); nodes p50 %d p90 %d p99 %d max %d; %.2f s; gap of the proved: max %.3g; "
          "of the rest: max %.3g" % (proved.mean(), proved.sum(), np.percentile(nd, 50), np.percentile(nd, 90),
                                     np.percentile(nd, 99), nd.max(), stats["seconds"], gap[proved].max(initial=0.0),
                                     gap[~proved].max(initial=0.0)))
    for r, q in zip(res, plain):
        assert r.lb >= q.lb and r.cost <= q.cost and r.feasible
    assert np.all(gap >= 0)
    assert np.all(gap[proved] <= 2e-6)
    assert proved.mean() >= PROVED_MIN


def test_create_dataset_exact_end_to_end(cuda_device, tmp_path):
    def make(path, **kw):
        random.seed(7)
        np.random.seed(7)
        return dataset.create_dataset(str(path), 20, 40, samples=32, **kw)

    s1 = make(tmp_path / "a", exact=True)
    s2 = make(tmp_path / "b", exact=True)
    names = sorted(os.listdir(tmp_path / "a"))
    assert len(names) == 32
    _, mismatch, errors = filecmp.cmpfiles(tmp_path / "a", tmp_path / "b", names, shallow=False)
    assert not mismatch and not errors
    assert s1["proved"].dtype == bool and s1["proved"].shape == (32,) and np.array_equal(s1["proved"], s2["proved"])
    assert np.array_equal(s1["nodes"], s2["nodes"]) and np.all(s1["nodes"] >= 1)
    assert s1["times"]["exact"] > 0 and np.all(s1["lb"] <= s1["cost"])
    # without exact nothing changes: the same files and summary as the call that does not name the argument
    p1 = make(tmp_path / "c", exact=False)
    p2 = make(tmp_path / "d")
    _, mismatch, errors = filecmp.cmpfiles(tmp_path / "c", tmp_path / "d", names, shallow=False)
    assert not mismatch and not errors
    assert "proved" not in p1 and "exact" not in p1["times"]
    assert np.array_equal(p1["cost"], p2["cost"]) and np.array_equal(p1["lb"], p2["lb"])
    assert np.all(s1["cost"] <= p1["cost"]) and np.all(s1["lb"] >= p1["lb"])
