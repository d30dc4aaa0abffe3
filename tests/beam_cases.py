"""Seeded inputs for the beam decoder's tests beyond those of decode_cases.py, whose batches it reuses with integer scores
in place of the votes.  Every array is built once per process and never modified."""
import functools

import numpy as np

import beam_reference as ref
import decode_cases as cases


@functools.lru_cache(maxsize=None)
def scores_of(name, *args):
    """q(votes) of a decode_cases batch, by the restatement."""
    return ref.q_scores(getattr(cases, name)(*args)["vote"])


@functools.lru_cache(maxsize=None)
def exhaustive_case():
    """The complete graph of 7 vertices on which any beam >= 6! = 720 enumerates every Hamiltonian path from vertex 0."""
    return cases.batch([cases.complete(np.random.RandomState(707), 7)])


# brute force over the 360 cycles of exhaustive_case (test_beam_host.py recomputes it): the optimum is unique
EXHAUSTIVE_TOUR = [0, 1, 4, 5, 2, 6, 3]
EXHAUSTIVE_COST = np.float32(1.7466016)
EXHAUSTIVE_RUNNER_UP = np.float32(1.9875989)


@functools.lru_cache(maxsize=None)
def clamp_case():
    """Scores outside [-2^22, 0] on input, on complete graphs of 6 and 70 vertices: a third lie below -2^22 (down to
    INT32_MIN), a third above 0 (up to INT32_MAX), the rest inside.  -> (batch, scores)."""
    rng = np.random.RandomState(21)
    b = cases.batch([cases.complete(rng, n) for n in (6, 70)])
    M = len(b["vote"])
    kind = rng.randint(0, 3, size=M)
    low = -(1 << 22) - rng.randint(0, 1 << 20, size=M).astype(np.int64) * rng.randint(1, 500, size=M)
    high = rng.randint(0, 1 << 20, size=M).astype(np.int64) * rng.randint(1, 2000, size=M)
    mid = -rng.randint(0, 1 << 22, size=M).astype(np.int64)
    s = np.where(kind == 0, low, np.where(kind == 1, high, mid))
    s[:4] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, -(1 << 22) - 1, 1]
    return b, np.clip(s, np.iinfo(np.int32).min, np.iinfo(np.int32).max).astype(np.int32)


# What the restatement makes of decode_cases.SPARSE with scores q(votes), per (graph, beam) for beam 1, 4, 64, as
# (stranded at step, n_closed, n_missing); test_beam_host.py asserts it.  11 of the 12 runs strand before step n - 1;
# (n = 12, beam 64) finishes with 10 closed entries of its final list and a feasible tour.
SPARSE_BEAMS = (1, 4, 64)
