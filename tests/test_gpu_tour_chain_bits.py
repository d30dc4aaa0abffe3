"""The tour chain kernels -- the three searches, the bound, nearest neighbour, the annealing and the branch and bound --
bit for bit against tests/golden/tour_chain_bits.npz (recorded by tools/record_tour_bits.py on the commit named in the
fixture's "meta" entry, before the kernels got one description of their LDS workspace, one starting-tour check, one
refusal, one 2-exchange evaluator and, for nearest neighbour and the annealing, one chain winner).  Cases: tests/tour_chain_cases.py.  Every output array of every case
must be numpy.array_equal to the recording: tours as int32, costs and bounds as bit patterns, node counts and statuses."""
import json
import os

import numpy as np
import pytest

import tour_chain_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tour_chain_bits.npz")
CASES = C.cases()


def _arrays(z, name):
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/") and "/" not in k[len(name) + 1:]}


@pytest.fixture(scope="module")
def recorded():
    z = np.load(GOLDEN)
    meta = json.loads(bytes(z["meta"]).decode())
    assert meta["commit"] and sorted(meta["cases"]) == sorted(c["name"] for c in CASES), meta
    return z


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tour_chain_bits(cuda_device, recorded, case):
    got = C.run_case(case, cuda_device)
    want = _arrays(recorded, case["name"])
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    bad = []
    for k in sorted(want):
        same = got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k])
        if not same:
            bad.append((k, int((got[k] != want[k]).sum()) if got[k].shape == want[k].shape else -1))
    print(" TOURBITS %s: %d arrays, %d differ %s" % (case["name"], len(want), len(bad), bad))
    assert not bad, bad


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_recording_answers_as_the_entry_points_promise(recorded, case):
    """Needs no GPU: the recording itself shows the refusal arm (NaN cost or bound, the tour slot still sentinel, the
    neighbours unaffected), TSPGNN_BB_BAD for an incumbent that is no permutation, and canonical tours everywhere else."""
    C.check_shape_of_answers(case, C.build(case), _arrays(recorded, case["name"]))


def test_the_two_layouts_recorded_the_same_bits(recorded):
    pairs = C.twins(CASES)
    assert len(pairs) >= 20
    for sq, tri in pairs:
        a, b = _arrays(recorded, sq["name"]), _arrays(recorded, tri["name"])
        assert sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), (sq["name"], k)


def test_fall_back_starts_are_taken():
    """An invalid starting tour must take the fall-back start: the ragged launches give chain 0 of instances 1, 2 and 3 an
    id equal to n, a repeated id and the -1 filler.  (The bits then equal the recording, which check_shape_of_answers
    shows to hold permutations; here: the cases do plant what they say.)"""
    c = next(c for c in CASES if c["name"] == "search/ragged/sq")
    h = C.build(c)
    kinds = dict(zip(range(5), c["starts"]))
    for i, sl in enumerate(C.slots(c)):
        t, n = h["starts"][sl], c["ns"][i]
        perm = sorted(t.tolist()) == list(range(n))
        assert perm == (kinds[i] == "valid"), (i, kinds[i])
        if kinds[i] == "n":
            assert t.max() == n
        if kinds[i] == "fill":
            assert (t == -1).all()
