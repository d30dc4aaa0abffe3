"""Seeded inputs for the vote decoder's tests: instances as (n, uv [m, 2] local endpoint ids, w [m] fp32 weights, votes [m]
fp32) and batches of them laid out as tspgnn_tour_from_votes reads them.  No reference code is involved; every array is
built once per process and never modified."""
import functools

import numpy as np


def complete_edges(n):
    """The edges of the complete graph in create_batch's order (np.nonzero of the upper triangle)."""
    iu = np.triu_indices(n, 1)
    return np.stack(iu, axis=1).astype(np.int32)


def complete(rng, n):
    uv = complete_edges(n)
    m = len(uv)
    return n, uv, rng.rand(m).astype(np.float32), rng.randn(m).astype(np.float32)


def sparse_planted(rng, n, connectivity):
    """A random graph of the given connectivity with a planted Hamiltonian cycle, as dataset.create_graph draws them."""
    A = np.triu(rng.rand(n, n) < connectivity, 1)
    perm = rng.permutation(n)
    for a, b in zip(perm, np.roll(perm, -1)):
        A[min(a, b), max(a, b)] = True
    uv = np.stack(np.nonzero(A), axis=1).astype(np.int32)
    m = len(uv)
    return n, uv, rng.rand(m).astype(np.float32), rng.randn(m).astype(np.float32)


def batch(instances):
    """Instances -> the device layout: global endpoint ids, wc with the weight in column 0 (column 1, the target cost, is
    filler the decoder must not read into its result), edge and vertex prefix sums."""
    ns = np.array([x[0] for x in instances], dtype=np.int32)
    ms = np.array([len(x[1]) for x in instances], dtype=np.int32)
    seg = np.concatenate([[0], np.cumsum(ms)]).astype(np.int32)
    vseg = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    M = int(seg[-1])
    uv = np.zeros((M, 2), dtype=np.int32)
    wc = np.full((M, 2), 7.25, dtype=np.float32)
    vote = np.zeros(M, dtype=np.float32)
    for b, (n, e, w, v) in enumerate(instances):
        uv[seg[b]:seg[b + 1]] = np.asarray(e, dtype=np.int32).reshape(-1, 2) + vseg[b]
        wc[seg[b]:seg[b + 1], 0] = w
        vote[seg[b]:seg[b + 1]] = v
    return {"n": ns, "seg": seg, "vseg": vseg, "uv": uv, "wc": wc, "vote": vote}


# The hand-written votes of the key test: every class of value, with equal votes at distinct edge ids.
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.0, 1.0, -1.0, 5e-39, -np.nan, 3.5, -2.0],
                   dtype=np.float32)


@functools.lru_cache(maxsize=None)
def complete_case(n):
    """One complete instance with random votes (n = 4, 5, 40 and the wave / workgroup boundaries 64 .. 256)."""
    return batch([complete(np.random.RandomState(700 + n), n)])


@functools.lru_cache(maxsize=None)
def ties_case():
    """All votes equal: the edge id decides everything.  n = 5 (one wave) and 70 (four waves)."""
    rng = np.random.RandomState(11)
    out = []
    for n in (5, 70):
        n, uv, w, _ = complete(rng, n)
        out.append((n, uv, w, np.full(len(uv), 0.25, dtype=np.float32)))
    return batch(out)


@functools.lru_cache(maxsize=None)
def special_case():
    """Votes drawn from SPECIAL (NaN, +-inf, +-0, subnormals, repeats) on complete graphs of 6 and 66 vertices."""
    rng = np.random.RandomState(12)
    out = []
    for n in (6, 66):
        n, uv, w, _ = complete(rng, n)
        out.append((n, uv, w, SPECIAL[rng.randint(0, len(SPECIAL), size=len(uv))]))
    return batch(out)


# Sparse graphs with a planted cycle, (n, connectivity, seed).  What the restatement makes of them on the CPU
# (test_decode_host.py asserts it), as (n_missing, paths): the greedy strands into 2, 6 and 7 paths on the first, third and
# fourth; on the second it finds one Hamiltonian path whose ends no edge joins.
SPARSE = ((12, 0.3, 1), (30, 0.2, 2), (70, 0.1, 3), (130, 0.1, 4))
SPARSE_OUTCOME = ((2, 2), (1, 1), (6, 6), (7, 7))


@functools.lru_cache(maxsize=None)
def sparse_case():
    return batch([sparse_planted(np.random.RandomState(900 + seed), n, c) for n, c, seed in SPARSE])


@functools.lru_cache(maxsize=None)
def odd_case():
    """An instance with a vertex no edge touches (vertex 3 of 9), one with no edge at all, one whose only edges are a
    self-loop and an endpoint outside the instance, and a multigraph whose 2 100 edges exceed the 64 x 32 register slots
    of the one-wave workgroup."""
    rng = np.random.RandomState(13)
    n, uv, w, v = complete(rng, 9)
    keep = (uv != 3).all(axis=1)
    lonely = (n, uv[keep], w[keep], v[keep])
    empty = (6, np.zeros((0, 2), dtype=np.int32), np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.float32))
    junk = (4, np.array([[2, 2], [1, 9], [-1, 0], [0, 1]], dtype=np.int32), rng.rand(4).astype(np.float32),
            np.array([9.0, 8.0, 7.0, -1.0], dtype=np.float32))
    m = 2100
    multi = (5, complete_edges(5)[rng.randint(0, 10, size=m)], rng.rand(m).astype(np.float32),
             rng.randn(m).astype(np.float32))
    multi[3][:2060] = -5.0      # the best edges sit past the register slots
    return batch([lonely, empty, junk, multi])


RAGGED_N = (4, 256, 17, 64, 129, 5, 65, 40)


@functools.lru_cache(maxsize=None)
def ragged_instances():
    rng = np.random.RandomState(14)
    return tuple(complete(rng, n) if k % 2 == 0 else sparse_planted(rng, n, 0.3) for k, n in enumerate(RAGGED_N))


@functools.lru_cache(maxsize=None)
def ragged_case():
    return batch(list(ragged_instances()))
