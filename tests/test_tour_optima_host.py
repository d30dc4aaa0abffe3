"""The exact optima behind tests/test_gpu_tour_optima.py, without a GPU: the rebuilt instances are the ones the fixture
was written for, its tours are Hamiltonian cycles of exactly the stored cost, the integer program that wrote it agrees
with the Held-Karp DP where the DP reaches, the NumPy branch and bound proves the recorded small cases in the recorded
number of nodes, and the incumbents handed to the kernel are strictly dearer than the optimum."""
import os

import numpy as np
import pytest

import tour_optima_cases as cases
from test_gpu_tour_solver import _w, held_karp
from test_tour_exact_host import branch_bound


@pytest.fixture(scope="module")
def loaded():
    return cases.load()


def test_fixture_covers_the_listed_sizes_and_stays_small(loaded):
    assert [(c.inst.family, c.inst.n) for c in loaded] == cases.SIZES
    assert os.path.getsize(cases.FIXTURE) < 256 * 1024
    for c in loaded:
        names = [r[0] for r in c.runs]
        assert names == (cases.incumbents((c.inst.family, c.inst.n, c.inst.seed)) if c.inst.n <= cases.BB_MAX_N else [])
        for name, nodes, proved, kind in c.runs:
            assert kind == cases.kind_of(c.inst.family, c.inst.n, nodes, proved)
            assert 1 <= nodes <= cases.RESTATEMENT_CAP
    main = [(c.inst.n, c.runs[0][3]) for c in loaded if c.runs]
    assert all(kind == "proving" for n, kind in main if n <= 64 and kind != "budget_expected")
    assert sum(kind == "proving" and n > 64 for n, kind in main) >= 3


def test_rebuilt_instances_match_their_crcs(loaded):
    z = np.load(cases.FIXTURE)
    for k, c in enumerate(loaded):
        assert cases.crcs(c.inst) == (int(z["crc_k"][k]), int(z["crc_mask"][k])), (c.inst.family, c.inst.n)
        K = c.inst.K
        edges = np.triu(c.inst.mask, 1)
        assert K.dtype == np.int64 and np.all(K[edges] >= 1) and np.array_equal(c.inst.Mw * cases.SCALE, K)
        # nothing is rounded on the way to the kernels, and every tour cost stays below 512
        W = cases.kernel_weights(c.inst)
        assert np.array_equal(W[c.inst.mask], (c.inst.Mw + c.inst.Mw.T)[c.inst.mask])
        assert np.all(W[~c.inst.mask & ~np.eye(c.inst.n, dtype=bool)] == c.inst.n * K[edges].max() / cases.SCALE + 1.0)
        assert c.inst.n * K[edges].max() < 512 * cases.SCALE


def test_stored_tours_are_cycles_of_the_stored_cost(loaded):
    for c in loaded:
        assert sorted(c.tour) == list(range(c.inst.n))
        assert c.tour[0] == 0 and c.tour[1] < c.tour[-1]
        assert cases.tour_cost(c.inst, c.tour) == c.optimum          # None if it used a missing edge
        if c.inst.planted is not None:
            assert cases.tour_cost(c.inst, c.inst.planted) >= c.optimum


@pytest.mark.parametrize("family", ["int", "euc", "uniform", "sparse", "clustered"])
def test_integer_program_equals_the_dp(family):
    pytest.importorskip("scipy")
    from oracle.tour_optima import solve_exact
    for n in range(6, 14):
        inst = cases.build(family, n, 100 + n)
        opt, tour = solve_exact(inst.K, inst.mask)
        dp = held_karp(_w(inst.Ma, inst.K.astype(np.float64)))      # integers in fp64: exact
        assert opt == dp, (family, n, opt, dp)
        assert cases.tour_cost(inst, tour) == opt and sorted(tour) == list(range(n))


def test_restatement_proves_the_recorded_small_cases(loaded):
    ran = 0
    for c in loaded:
        if c.inst.n > 32:
            continue
        w = cases.kernel_weights(c.inst)
        for name, nodes, proved, kind in c.runs:
            if kind != "proving":
                continue
            cost, tour, lb, got, ok = branch_bound(w, cases.incumbent(c.inst, c.tour, name),
                                                   max_nodes=cases.RESTATEMENT_CAP)
            assert ok and got == nodes, (c.inst.family, c.inst.n, name, got, nodes)
            assert cost * cases.SCALE == c.optimum and cases.tour_cost(c.inst, tour) == c.optimum
            assert lb <= cost and cost - lb <= 2e-6 * cost
            ran += 1
    assert ran >= 4


def test_worsened_incumbents_are_strictly_dearer(loaded):
    for c in loaded:
        t = cases.worsen(c.inst, c.tour)
        assert sorted(t) == list(range(c.inst.n))
        cost = cases.tour_cost(c.inst, t)
        assert cost is not None and cost > c.optimum, (c.inst.family, c.inst.n)
