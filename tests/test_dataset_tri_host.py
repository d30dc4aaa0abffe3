"""Host side of the n 129-256 labelling path (tspgnn.dataset.label_tours on the packed-triangle kernels): the argument
checks of tspgnn_tour_search_tri / tspgnn_tour_lower_bound_tri, the triangle packer against the dense one, and the
limits label_tours enforces before anything is launched.  No GPU."""
import ctypes

import numpy as np
import pytest

from tspgnn import _lib, dataset


def test_tri_entry_points_reject_bad_arguments_without_gpu():
    L = _lib.lib
    p = ctypes.c_void_p(16)
    # n_max > 256: EUNSUPPORTED before anything is launched
    assert L.tspgnn_tour_search_tri(p, p, p, None, p, None, 4, 257, 4, 8, 0, p, p, None) == -2
    assert b"256" in L.tspgnn_last_error()
    assert L.tspgnn_tour_lower_bound_tri(p, p, p, p, 4, 257, 10, p, None) == -2
    # bad sizes and null pointers: EINVAL
    assert L.tspgnn_tour_search_tri(None, p, p, None, p, None, 4, 200, 4, 8, 0, p, p, None) == -1
    assert L.tspgnn_tour_search_tri(p, p, p, None, p, None, 4, 200, 0, 8, 0, p, p, None) == -1
    assert L.tspgnn_tour_search_tri(p, p, p, None, p, None, 4, 200, 17, 8, 0, p, p, None) == -1
    assert L.tspgnn_tour_search_tri(p, p, p, None, p, None, 4, 200, 4, -1, 0, p, p, None) == -1
    assert L.tspgnn_tour_search_tri(p, p, p, None, p, None, 4, 3, 4, 8, 0, p, p, None) == -1
    assert L.tspgnn_tour_search_tri(p, p, p, None, p, None, -1, 200, 4, 8, 0, p, p, None) == -1
    assert L.tspgnn_tour_lower_bound_tri(p, p, p, None, 4, 200, 10, p, None) == -1
    assert L.tspgnn_tour_lower_bound_tri(p, p, p, p, 4, 200, 0, p, None) == -1
    assert L.tspgnn_tour_lower_bound_tri(p, p, p, p, 4, 2, 10, p, None) == -1
    # restarts over the LDS budget: 10 chains fit at n_max = 256, 16 at n_max = 242
    assert L.tspgnn_tour_search_tri(p, p, p, None, p, None, 4, 256, 11, 8, 0, p, p, None) == -1
    msg = L.tspgnn_last_error()
    assert b"restarts=11" in msg and b"at most 10" in msg
    assert L.tspgnn_tour_search_tri(p, p, p, None, p, None, 4, 243, 16, 8, 0, p, p, None) == -1
    assert dataset.tri_chains_fit(256) == 10 and dataset.tri_chains_fit(243) == 15 and dataset.tri_chains_fit(242) == 16
    # empty batches are a no-op
    assert L.tspgnn_tour_search_tri(None, None, None, None, None, None, 0, 0, 1, 0, 0, None, None, None) == 0
    assert L.tspgnn_tour_lower_bound_tri(None, None, None, None, 0, 0, 1, None, None) == 0


@pytest.mark.parametrize("n,conn", [(4, 1.0), (9, 0.5), (37, 0.3), (130, 1.0), (200, 0.1)])
def test_triangle_packer_matches_dense_packer(n, conn):
    rng = np.random.RandomState(n)
    b = 3
    Mw = rng.rand(b, n, n) * 10
    Mw[1] = np.triu(Mw[1], 1)           # an upper-triangular Mw, as read_graph returns
    Ma = rng.rand(b, n, n) < conn
    A = np.stack([dataset._edge_mask(m) for m in Ma])
    dense = dataset._penalised(A, Mw)
    tri = dataset._penalised_tri(A, Mw)
    iu = np.triu_indices(n, 1)
    assert tri.dtype == np.float32 and tri.shape == (b, n * (n - 1) // 2)
    assert np.array_equal(tri.view(np.uint32), dense[:, iu[0], iu[1]].view(np.uint32))
    # the kernels' row offset: w(a, b) for a < b at a (2n - 3 - a) / 2 - 1 + b
    a, c = iu
    assert np.array_equal(a * (2 * n - 3 - a) // 2 - 1 + c, np.arange(iu[0].size))


def test_label_tours_limits_without_gpu():
    big = np.ones((257, 257))
    with pytest.raises(ValueError, match="instance 1: n=257 .* 256"):
        dataset.label_tours([(np.ones((5, 5)), np.ones((5, 5))), (big, big)])
    n256 = (np.ones((256, 256)), np.ones((256, 256)))
    with pytest.raises(ValueError, match="at most 10 chains"):
        dataset.label_tours([n256], restarts=11)
    with pytest.raises(ValueError):
        dataset.label_tours([n256], restarts=17)
    with pytest.raises(ValueError):
        dataset.label_tours([n256], kicks=-1)
    # n < 4 is still solved on the host, with no device needed
    Ma = np.array([[0, 1, 1], [0, 0, 1], [0, 0, 0]])
    Mw = np.array([[0, 0.5, 0.25], [0.5, 0, 0.125], [0.25, 0.125, 0]])
    assert dataset.label_tours([(Ma, Mw)]) == dataset.solve_tours([(Ma, Mw)])
