"""The instances whose exact optima tests/golden/tour_optima.npz holds (oracle/tour_optima.py wrote it with an integer
program; tests/test_tour_optima_host.py and tests/test_gpu_tour_optima.py read it).  Instances are rebuilt here from
np.random.RandomState(seed), not stored; the fixture keeps a CRC32 of each.

Every weight is k / 4096 with an integer k >= 1, so every weight, the penalty n * max + 1 of a missing edge and every
tour cost below 512 are exact in fp32 and in fp64: dataset._penalised rounds nothing, and the integer program's
objective, sum of k, is the instance the kernels see.
"""
import collections
import os
import zlib

import numpy as np

from test_tour_exact_host import int_family
from tspgnn import dataset

SCALE = 4096
BB_MAX_N = dataset.MAX_N          # tspgnn_tour_branch_bound's limit: larger cases have bounds and searches only
RESTATEMENT_CAP = 600             # nodes the NumPy restatement was given when the fixture was written
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tour_optima.npz")

SIZES = ([("int", n) for n in (20, 24, 28, 32)]
         + [("euc", n) for n in (30, 40, 50, 63, 64, 65, 100, 128, 150, 200)]
         + [("uniform", n) for n in (40, 65, 66, 90, 127, 128, 129, 192, 193, 255, 256)]
         + [("sparse", n) for n in (30, 65, 100, 128, 200, 256)]
         + [("clustered", n) for n in (40, 65, 96)])

# (family, n, seed): the seeds that oracle/tour_optima.py's ``select`` printed for SIZES (the rule: kind_of).
CASES = [
    ("int", 20, 0), ("int", 24, 2), ("int", 28, 1), ("int", 32, 2),
    ("euc", 30, 0), ("euc", 40, 1), ("euc", 50, 0), ("euc", 63, 0), ("euc", 64, 0), ("euc", 65, 0), ("euc", 100, 0),
    ("euc", 128, 0), ("euc", 150, 0), ("euc", 200, 0),
    ("uniform", 40, 1), ("uniform", 65, 0), ("uniform", 66, 0), ("uniform", 90, 0), ("uniform", 127, 0),
    ("uniform", 128, 0), ("uniform", 129, 0), ("uniform", 192, 0), ("uniform", 193, 0), ("uniform", 255, 0),
    ("uniform", 256, 0),
    ("sparse", 30, 6), ("sparse", 65, 0), ("sparse", 100, 0), ("sparse", 128, 0), ("sparse", 200, 0), ("sparse", 256, 0),
    ("clustered", 40, 0), ("clustered", 65, 0), ("clustered", 96, 0),
]

Instance = collections.namedtuple("Instance", "family n seed K mask Ma Mw planted")
Instance.__doc__ = """K: int64 [n, n], upper triangular, the weights times SCALE; mask: symmetric bool edge set; Ma, Mw: what
the dataset functions take (Mw = K / SCALE); planted: the planted Hamiltonian cycle of a sparse graph, else None."""


def _distances(p):
    d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
    return np.maximum(1, np.rint(SCALE * d)).astype(np.int64)


def _plant(rng, Ma):
    n = Ma.shape[0]
    perm = [int(x) for x in rng.permutation(n)]
    for i, j in zip(perm, perm[1:] + perm[:1]):
        Ma[min(i, j), max(i, j)] = 1
    return perm


def build(family, n, seed):
    """The instance of (family, n, seed)."""
    rng = np.random.RandomState(seed)
    Ma = np.triu(np.ones((n, n)), 1)
    planted = None
    if family == "euc":
        K = _distances(rng.rand(n, 2))
    elif family == "uniform":
        K = rng.randint(1, SCALE + 1, size=(n, n)).astype(np.int64)
    elif family == "sparse":
        K = rng.randint(1, SCALE + 1, size=(n, n)).astype(np.int64)
        Ma = np.triu((rng.rand(n, n) < 0.2).astype(float), 1)
        planted = _plant(rng, Ma)
    elif family == "int":
        ((Ma, Mw),), (planted,) = int_family(rng, [n])
        K = Mw.astype(np.int64) * SCALE
    elif family == "clustered":
        centres = rng.rand(max(1, n // 8), 2)
        K = _distances(centres[rng.randint(len(centres), size=n)] + 0.02 * rng.randn(n, 2))
    else:
        raise ValueError(family)
    K = np.triu(K, 1)
    return Instance(family, n, seed, K, dataset._edge_mask(Ma), Ma, K / float(SCALE), planted)


def crcs(inst):
    return (zlib.crc32(np.ascontiguousarray(inst.K, dtype=np.int64).tobytes()),
            zlib.crc32(np.ascontiguousarray(inst.mask, dtype=np.uint8).tobytes()))


def tour_cost(inst, tour):
    """The integer cost (in 1 / SCALE) of a tour, or None when it uses a missing edge."""
    total = 0
    for a, b in zip(tour, list(tour[1:]) + list(tour[:1])):
        if not inst.mask[a, b]:
            return None
        total += int(inst.K[min(a, b), max(a, b)])
    return total


def kernel_weights(inst):
    """The matrix the kernels get, as fp64: exactly K / SCALE on the edges and the penalty off them."""
    return dataset._penalised(inst.mask[None], inst.Mw[None])[0].astype(np.float64)


def worsen(inst, tour):
    """``tour`` with one segment reversed, the first (i, j) in order whose two new edges exist and whose cost is strictly
    higher: a feasible incumbent that the branch and bound has to beat by itself."""
    n = len(tour)
    base = tour_cost(inst, tour)
    for i in range(n - 2):
        for j in range(i + 2, n - (i == 0)):
            t = list(tour[:i + 1]) + list(tour[i + 1:j + 1])[::-1] + list(tour[j + 1:])
            c = tour_cost(inst, t)
            if c is not None and c > base:
                return t
    raise ValueError("no 2-opt neighbour of the tour is dearer")


def incumbents(case):
    """The names of the incumbents the branch and bound is started from on a case, the main one first."""
    family, n, _ = case
    if family == "int":
        return ["planted"]
    if n <= 40 and family in ("euc", "uniform", "sparse"):
        return ["worse", "planted" if family == "sparse" else "identity"]
    return ["worse"]


def incumbent(inst, tour, name):
    return {"worse": lambda: worsen(inst, tour), "identity": lambda: list(range(inst.n)),
            "planted": lambda: list(inst.planted)}[name]()


def restatement_cap(n):
    return RESTATEMENT_CAP


def kind_of(family, n, nodes, proved):
    """What a run of the restatement (its node count; it proved the optimum) makes of a (case, incumbent):
    'proving' (8 to 512 nodes: the kernel has to branch and is expected to finish), 'budget_expected' (every clustered
    case; no proof within RESTATEMENT_CAP nodes), 'easy' (fewer than 8 nodes) or 'long' (more than 512)."""
    if family == "clustered" or not proved:
        return "budget_expected"
    return "proving" if 8 <= nodes <= 512 else ("easy" if nodes < 8 else "long")


Case = collections.namedtuple("Case", "inst optimum tour runs")
Case.__doc__ = """inst: the rebuilt Instance; optimum: the integer optimum (in 1 / SCALE); tour: one optimal tour;
runs: [(incumbent name, restatement nodes, restatement proved, kind)], empty for n > BB_MAX_N."""


def load():
    """The cases of the fixture, rebuilt; raises when the fixture and CASES disagree."""
    z = np.load(FIXTURE)
    listed = [(str(f), int(n), int(s)) for f, n, s in zip(z["family"], z["n"], z["seed"])]
    if listed != [tuple(c) for c in CASES]:
        raise AssertionError("tests/golden/tour_optima.npz was not written for tour_optima_cases.CASES")
    off = np.concatenate([[0], np.cumsum(z["n"])])
    out = []
    for k, case in enumerate(listed):
        runs = [(str(z["bb_incumbent"][r]), int(z["bb_nodes"][r]), bool(z["bb_proved"][r]), str(z["bb_kind"][r]))
                for r in np.flatnonzero(z["bb_case"] == k)]
        out.append(Case(build(*case), int(z["optimum"][k]), [int(x) for x in z["tours"][off[k]:off[k + 1]]], runs))
    return out
