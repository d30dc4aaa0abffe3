"""NumPy restatement of tspgnn_build_instances (csrc/dataset_build.hip) for the tests: the matrices of one instance from
the flat random streams of dataset.draw_streams, with the arithmetic the header pins -- pair k is the k-th (i, j > i) in
row-major order; A = adj_u < conn, the planted cycle OR-ed in; euc_2D weights sqrt(dx dx + dy dy), each operation rounded
once; random weights wts[k] mirrored; both diagonals 0."""
import numpy as np


def build_instance(S, i):
    """-> (symmetric Ma float64 [n, n], Mw float64 [n, n] (no closure), planted permutation as a list)."""
    n = int(S["n"][i])
    p0, p1 = int(S["pair_off"][i]), int(S["pair_off"][i + 1])
    v0, v1 = int(S["vert_off"][i]), int(S["vert_off"][i + 1])
    assert p1 - p0 == n * (n - 1) // 2 and v1 - v0 == n
    iu = np.triu_indices(n, 1)
    Ma = np.zeros((n, n))
    Ma[iu] = S["adj_u"][p0:p1] < S["conn"][i]
    Ma = Ma + Ma.T
    Mw = np.zeros((n, n))
    if S["distances"] == "euc_2D":
        pts = S["pts"][2 * v0:2 * v1].reshape(n, 2)
        dx = pts[:, None, 0] - pts[None, :, 0]
        dy = pts[:, None, 1] - pts[None, :, 1]
        Mw = np.sqrt(dx * dx + dy * dy)
        np.fill_diagonal(Mw, 0.0)
    else:
        Mw[iu] = S["wts"][p0:p1]
        Mw = Mw + Mw.T
    perm = [int(x) for x in S["perm"][v0:v1]]
    for a, b in zip(perm, perm[1:] + perm[:1]):
        Ma[a, b] = Ma[b, a] = 1.0
    return Ma, Mw, perm
