"""The launch plans of the fp32 backward and training-tail kernels, as tests/plan_replay.py reads them from the library's
tspgnn_plan_* queries -- the planners the launchers themselves call.  The workspace-size queries must agree with them:
tspgnn_wgrad_workspace_floats = nc (kin nout + nout), tspgnn_wcolsum_workspace_floats = nc (d + 1) and
tspgnn_einit_bwd_workspace_floats.  Without a device n_cus() answers 256, so those pins are for cus = 256; the grid of
shapes holds every row count that tests/test_gpu_fp32_backward_plans.py and tests/test_gpu_batch_kernels.py use there.
The other tests pin the planners (linear, mlp_bwd, the einit_bwd grid, reduce_partials2's S) at the values the GPU tests
name in their ids and docstrings for 256 CUs: a launcher that changes fails here and says what moved, not silently in a
"deep" test."""
import pytest

import plan_replay as PR
from tspgnn import _lib

CUS = 256     # what n_cus() answers without a device, and the MI355X's count


def lib_cus():
    """The CU count the library plans with: the device's where there is one, else 256."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else CUS


WGRAD_ROWS = [1, 15, 16, 17, 255, 256, 257, 500, 4095, 4096, 4097, 70001, 99840, 131073, 636800, 5094400]
WGRAD_WIDTHS = [16, 32, 48, 64, 96, 128, 256, 512]


def test_wgrad_workspace_is_the_replayed_chunk_count():
    cus = lib_cus()
    for rows in WGRAD_ROWS:
        for kin in WGRAD_WIDTHS:
            for nout in WGRAD_WIDTHS:
                got = int(_lib.lib.tspgnn_wgrad_workspace_floats(rows, kin, nout))
                plan = PR.wgrad_plan(rows, kin, nout, cus)
                assert got == plan.n_chunks * (kin * nout + nout) == PR.wgrad_workspace_floats(rows, kin, nout, cus), (rows, kin, nout)
                assert 0 < plan.last_rows <= plan.chunk_rows and plan.chunk_rows % 16 == 0
    assert _lib.lib.tspgnn_wgrad_workspace_floats(0, 64, 64) == 0 == PR.wgrad_workspace_floats(0, 64, 64, cus)
    assert _lib.lib.tspgnn_wgrad_workspace_floats(100, 24, 64) == 0 == PR.wgrad_workspace_floats(100, 24, 64, cus)


COLSUM_ROWS = [1, 2, 994, 1023, 1024, 1025, 2047, 2048, 2049, 8 * 1024 + 1, 64 * 1024 + 1, 1024 * 4 * CUS - 1, 1024 * 4 * CUS,
               1024 * 4 * CUS + 1, 5094400]


def test_wcolsum_workspace_is_the_replayed_chunk_count():
    cus = lib_cus()
    for rows in COLSUM_ROWS + [1024 * 4 * cus + 1]:
        for d in (4, 32, 64, 128, 256, 1024):
            got = int(_lib.lib.tspgnn_wcolsum_workspace_floats(rows, d))
            plan = PR.colsum_plan(rows, cus)
            assert got == plan.n_chunks * (d + 1) == PR.wcolsum_workspace_floats(rows, d, cus), (rows, d)
            assert 0 < plan.last_rows <= plan.chunk_rows and (plan.n_chunks - 1) * plan.chunk_rows + plan.last_rows == rows
    assert _lib.lib.tspgnn_wcolsum_workspace_floats(0, 64) == PR.wcolsum_workspace_floats(0, 64, cus) == 65


def test_einit_bwd_workspace_holds_a_partial_row_per_workgroup():
    for d in (32, 64, 128):
        full = PR.einit_bwd_full_grid(d, CUS)
        for M in (1, 63, 64, 65, 333, 64 * full, 64 * full + 1, 64 * 2 * full + 1):
            got = int(_lib.lib.tspgnn_einit_bwd_workspace_floats(M, d))
            plan = PR.einit_bwd_plan(M, d, CUS)
            assert got == PR.einit_bwd_workspace_floats(M, d) == plan.n_chunks * PR.einit_np(d), (M, d)
            assert plan.grid * PR.einit_np(d) <= got          # the kernel writes one row per workgroup


def test_wgrad_plans_at_256_cus():
    """What tests/test_gpu_fp32_backward_plans.py names for 256 CUs: all nine (AV, BV) on the generic kernel at 70 001 rows
    except (4, 4), which is generic up to 4095 rows and wgrad_x3_kernel from 4096."""
    for kin, av in ((16, 1), (32, 2), (64, 4)):
        for nout, bv in ((16, 1), (32, 2), (64, 4)):
            p = PR.wgrad_plan(70001, kin, nout, CUS)
            assert (p.av, p.bv) == (av, bv) and p.kernel == ("x3" if av == bv == 4 else "generic")
            assert p.n_chunks == 274 and p.chunk_rows == 256 and p.last_rows == 113 and PR.reduce_slices(p.n_chunks) == 16
    p = PR.wgrad_plan(4095, 64, 64, CUS)
    assert p.kernel == "generic" and (p.n_chunks, p.chunk_rows, p.last_rows) == (16, 256, 255) and PR.reduce_slices(16) == 4
    assert PR.wgrad_plan(4096, 64, 64, CUS).kernel == "x3"
    # the d = 32 configurations: kin 32 -> AV = 2, nc = 8 CUs / nob chunks at ~10^5 rows
    p = PR.wgrad_plan(99840, 32, 128, CUS)
    assert (p.av, p.bv, p.nob, p.kernel) == (2, 4, 2, "generic") and p.n_chunks == 390


@pytest.mark.parametrize("kin,n1,n2,per_cu,streamed", [(256, 0, 64, 2, False), (128, 64, 64, 2, False), (256, 64, 64, 1, False),
                                                       (512, 128, 128, 1, True), (256, 48, 16, 2, False)])
def test_linear_plans_at_256_cus(kin, n1, n2, per_cu, streamed):
    """The four paths of launch_linear at the row counts of the GPU test, for 256 CUs."""
    P = lambda rows: PR.linear_plan(kin, n1, n2, rows, CUS)
    assert P(1).per_cu == per_cu
    if streamed:
        assert P(1).qc == 8 < kin // 16
        for rows in (1, 17, 16 * 4 * CUS, 16 * 4 * CUS + 1):
            assert P(rows).path == "streamed" and P(rows).nw == 8
        p = P(16 * 8 * (2 * CUS * per_cu) + 17)            # 65 553 rows
        assert (p.path, p.nw, p.grid, p.rounds, p.lo, p.hi, p.dead) == ("streamed", 8, 256, 513, 2, 3, 6)
        return
    assert P(1).qc == kin // 16
    for rows in (1, 15, 16, 17, 16 * 4 * CUS):             # 16 384 rows: the last on the split kernel
        assert P(rows).path == "split"
    first = P(16 * 4 * CUS + 1)                            # 16 385 rows: the first on the ticket kernel
    assert first.path == "ticket" and first.nw == (4 if per_cu == 2 else 8)
    full = CUS * per_cu
    if per_cu == 2:     # nw = 4 holds up to four tiles per workgroup: its deepest launch has one tile per wavefront
        p = P(16 * 4 * full - 15)                          # 32 753 rows
        assert (p.path, p.nw, p.grid, p.lo, p.hi) == ("ticket", 4, 512, 1, 1)
        assert P(16 * 4 * full + 1).nw == 8
    p = P(16 * (2 * full * 8) + 1)                         # 131 073 rows (65 537 with one workgroup per CU)
    assert (p.path, p.nw, p.grid, p.lo, p.hi) == ("ticket", 8, full, 2, 3)


def test_mlp_bwd_plans_at_256_cus():
    for d, full in ((32, 512), (64, 512), (128, 256)):
        assert PR.mlp_bwd_plan([(17, 2)], d, CUS) == PR.MlpBwdPlan(4, 1, [1], [0], [1])
        deep = 16 * (2 * full * 8) + 1                     # 131 073 rows (d = 128: 65 537)
        p = PR.mlp_bwd_plan([(deep, 2)], d, CUS)
        assert (p.nw, p.grid, p.lo, p.hi) == (8, full, [2], [3])
        p = PR.mlp_bwd_plan([(333, 2), (deep, 2)], d, CUS)
        assert p.nw == 8 and p.blocks[0] >= 1 and sum(p.blocks) == p.grid and p.lo[1] >= 2


def test_einit_bwd_and_colsum_plans_at_256_cus():
    assert PR.einit_bwd_plan(333, 64, CUS) == PR.EinitBwdPlan(6, 6, 1, 1)          # test_einit_backward: one chunk each
    for d, full in ((32, 512), (64, 512), (128, 256)):
        assert PR.einit_bwd_plan(64 * full, d, CUS) == PR.EinitBwdPlan(full, full, 1, 1)
        assert PR.einit_bwd_plan(64 * full + 1, d, CUS) == PR.EinitBwdPlan(full, full + 1, 1, 2)
        assert PR.einit_bwd_plan(64 * 2 * full + 1, d, CUS) == PR.EinitBwdPlan(full, 2 * full + 1, 2, 3)
    assert [PR.reduce_slices(n) for n in (1, 7, 8, 63, 64, 512)] == [1, 1, 4, 4, 16, 16]
    assert PR.colsum_plan(994, CUS) == PR.ColsumPlan(1, 994, 994, False)
    assert PR.colsum_plan(1025, CUS) == PR.ColsumPlan(2, 513, 512, False)
    assert PR.colsum_plan(8 * 1024 + 1, CUS) == PR.ColsumPlan(9, 911, 905, False)
    assert PR.colsum_plan(64 * 1024 + 1, CUS) == PR.ColsumPlan(65, 1009, 961, False)
    assert PR.colsum_plan(1024 * 4 * CUS + 1, CUS) == PR.ColsumPlan(1024, 1025, 2, True)
    assert [PR.colsum_rows_in_flight(d) for d in (4, 32, 64, 128, 256, 1024)] == [256, 32, 16, 8, 4, 1]
    assert PR.strided_blocks(16400 * 64, 4096) == (4096, True) and PR.strided_blocks(994 * 16, 4096) == (63, False)
    assert PR.strided_blocks(2 * 1024 * 256 + 3, 1024) == (1024, True) and PR.strided_blocks(115529, 1024) == (452, False)
