"""The plans of the forward cell and MLP launchers (plan_replay.cell_fwd_plan / mlp_fwd_plan: the library's
tspgnn_plan_cell_fwd / tspgnn_plan_mlp_fwd, and the kernels' own tile walks derived from them) against figures worked out
by hand from the planners' text (csrc/launch_plan.h, csrc/common.h) at the shapes the project runs -- no device.  The GPU
tests of tests/test_gpu_cell_forward_edges.py assert their branches through the same functions; when a planner changes,
the figures here say what moved."""
import pytest

from plan_replay import cell_fwd_plan, cell_task, mlp_fwd_plan, ticket_ranges, xcd_contiguous


@pytest.mark.parametrize("tiles", [1, 7, 8, 333, 4097, 6145, 100003])
def test_resident_ticket_ranges_partition_the_tiles(tiles):
    """For every workgroup count 1 ... 520 -- every remainder mod 8, below and above one workgroup per XCD -- xcd_contiguous
    is a permutation, and the ranges [t_beg, t_end) taken through it cover [0, tiles) exactly once."""
    for my_grid in range(1, 521):
        pos = sorted(xcd_contiguous(b, my_grid) for b in range(my_grid))
        assert pos == list(range(my_grid)), my_grid
        ranges = sorted(ticket_ranges(tiles, my_grid))
        assert ranges[0][0] == 0 and ranges[-1][1] == tiles, my_grid
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), my_grid
        assert all(e >= b for b, e in ranges), my_grid


def test_xcd_contiguous_keeps_an_xcd_consecutive():
    """What the map is for: the workgroups b, b + 8, b + 16, ... of one XCD hold consecutive positions."""
    for n in (1, 5, 8, 9, 15, 109, 229, 256):
        for x in range(min(8, n)):
            pos = [xcd_contiguous(b, n) for b in range(x, n, 8)]
            assert pos == list(range(pos[0], pos[0] + len(pos))), (n, x)


def step(M, N, d=64, cus=256, arith="h2"):
    """A message-passing step's cell launch: the edge gather cell + 3 layers, the vertex cell + 4 layers + projection."""
    return cell_fwd_plan([cell_task(M, 0, 3, False, True, True), cell_task(N, d, 4, True, True, True)], d, cus, arith)


# (M, N) -> nw, edge workgroups, vertex workgroups, split, the launcher's rounds per vertex workgroup
TABLE = [((7001, 333), 4, 109, 6, "fixed", 1),
         ((6080, 640), 4, 95, 10, "fixed", 1),              # C1
         ((99840, 5120), 12, 229, 27, "fixed", 1),          # C2
         ((695849, 25362), 12, 229, 27, "fixed", 5),        # C4
         ((100, 5000), 4, 1, 79, "plain", 1)]               # the fixed share would be 79 of 80 workgroups: the plain split


@pytest.mark.parametrize("shape,nw,be,bv,split,n_rounds", TABLE)
def test_step_launches_at_256_cus(shape, nw, be, bv, split, n_rounds):
    p = step(*shape)
    assert (p.nw, p.blk_end, p.split) == (nw, [be, be + bv], split)
    e, v = p.tasks
    assert e.mode == "resident" and e.blocks == be and len(e.ranges) == be
    assert v.mode == "lockstep" and v.together == 1 and v.kbc == 4 and v.chunks == 1 and v.preload
    assert v.lock_tiles == nw and v.n_rounds == n_rounds
    # the kernel's own walk agrees with the rounds the launcher meant to give each workgroup
    assert v.rounds_per_wg[1] == n_rounds and v.rounds_per_wg[0] >= n_rounds - 1
    assert not p.centered


def test_c4_footprint_turns_write_through_off():
    assert step(99840, 5120).wt and step(6080, 640).wt
    assert not step(695849, 25362).wt          # 2 * (3 * 695 849 + 2 * 25 362) * 256 B > 200 MiB


def test_vertex_task_alone_splits_plainly():
    """16 * (12 * 2 * 256) + 1 rows: 6145 tiles, 513 rounds of 12 over 256 workgroups, two or three each; the last round
    has one live wavefront."""
    p = cell_fwd_plan([cell_task(98305, 64, 4, True, True, True)], 64, 256)
    v = p.tasks[0]
    assert (p.nw, p.grid, p.split) == (12, 256, "plain")
    assert (v.mode, v.rounds, v.rounds_per_wg, v.n_rounds) == ("lockstep", 513, (2, 3), 2)
    assert v.tiles - (v.rounds - 1) * v.lock_tiles == 1


def test_modes_h2():
    one = lambda d, *a, **k: cell_fwd_plan([cell_task(333, *a, **k)], d, 256).tasks[0]
    e = one(64, 0, 3, mlp_out=True)                         # the edge gather cell + 3 layers
    assert (e.mode, e.kbc) == ("resident", 2)
    v = one(64, 64, 4, True)                                # the vertex cell + 4 layers + projection: K whole
    assert (v.mode, v.kbc, v.chunks, v.together, v.preload) == ("lockstep", 4, 1, 1, True)
    w = one(64, 192)                                        # 8 k-blocks in two chunks of 4, no operand preload
    assert (w.mode, w.kbc, w.chunks, w.preload) == ("lockstep", 4, 2, False)
    assert one(64, 64).mode == "resident" and one(64, 64).kbc == 4       # a plain cell with no MLP
    a = one(32, 256)                                        # 9 k-blocks fit whole
    assert (a.mode, a.kbc) == ("resident", 9)
    a4 = one(32, 256, 4)                                    # ... and stay whole in lock step beside four layers
    assert (a4.mode, a4.kbc, a4.chunks, a4.preload) == ("lockstep", 9, 1, False)
    b = one(32, 320)                                        # 11 k-blocks: chunks of 9
    assert (b.mode, b.kbc, b.chunks, b.preload) == ("lockstep", 9, 2, False)


def test_together_is_never_off_with_a_projection():
    """together = 0 (the MLP layers and the projection matrix in two residencies) needs mlp_layers * layer bytes + the
    projection matrix beyond the 160 KB budget: at d = 64 four layers and the matrix are 132 096 B, at d = 32 33 280 B.  With
    d in {32, 64} and at most four layers -- all the entry accepts -- no task reaches it, so no test invents one."""
    for d in (32, 64):
        for dx in range(0, 513, 32):
            for L in range(1, 5):
                t = cell_fwd_plan([cell_task(100, dx, L, True)], d, 256).tasks[0]
                assert t.mode == "lockstep" and t.together == 1, (d, dx, L)


def test_modes_x3():
    """launch_cell_x3: three pieces per weight, kbc = KBT - 1 forces the lock step where K would fit but the MLP or a
    projection does not; a lock-step task always gets the workgroups of one round; no WT or centred variant."""
    one = lambda d, *a, **k: cell_fwd_plan([cell_task(333, *a, **k)], d, 256, "x3")
    assert one(64, 0, 3).tasks[0].mode == "resident"
    v = one(64, 64, 4, True, True, True, True)
    assert (v.tasks[0].mode, v.tasks[0].kbc, v.tasks[0].chunks) == ("lockstep", 3, 2) and not v.wt and not v.centered
    assert one(32, 96).tasks[0].mode == "resident"
    f = one(32, 96, 4, True).tasks[0]                       # K fits, the projection forces the lock step: kbc = KBT - 1
    assert (f.mode, f.kbc, f.chunks) == ("lockstep", 3, 2)
    with pytest.raises(ValueError):
        one(32, 0, 1, True)                                 # one k-block cannot be walked in lock step
    p = step(695849, 25362, arith="x3")
    # one round would be 133 workgroups > 256 / 2: the plain split by cost, and the kernel walks 7 or 8 rounds on 17
    assert p.split == "plain" and p.blk_end == [239, 256] and p.tasks[1].rounds_per_wg == (7, 8)
    p = step(99840, 5120, arith="x3")
    assert (p.nw, p.blk_end, p.split) == (12, [229, 256], "fixed")


def test_mlp_launch_wavefronts():
    for tiles, nw in ((1024, 4), (1025, 8), (4096, 8), (4097, 16)):
        p = mlp_fwd_plan([(tiles * 16, 3, False)], 256)
        assert p.nw == nw and p.grid == min(256, -(-tiles // nw))
    p = mlp_fwd_plan([(9000, 3, False), (700, 4, True)], 256)
    # 563 + 44 tiles: 152 workgroups of 4 wavefronts; cost 563 * 3 against 44 * (4 + 5)
    assert p.nw == 4 and p.grid == 152 and p.blocks == [123, 29] and sum(e - b for b, e in p.ranges[1]) == 44
