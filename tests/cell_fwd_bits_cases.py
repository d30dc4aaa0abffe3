"""Cases of tests/test_gpu_cell_fwd_bits.py and tools/record_cell_bits.py: launches of tspgnn_lnlstm_mlp_fwd_multi_h2
(csrc/dense_h2.hip) on seeded inputs whose outputs are pinned BIT FOR BIT in tests/golden/cell_fwd_bits.npz.  The fixture is
recorded once, by tools/record_cell_bits.py on the commit its metadata names; the f32 arithmetic of the tile (mfma_tile.h:
packed or single-issue form) may be rewritten as long as every element still sees the same IEEE operations in the same order.

A launch is the two tasks of a time step, built with tests/cell_fwd_cases.FwdCell -- a gather-init edge task (dx = 0, 3 relu
layers -> messages) and a bias-init vertex task (dx = d, 4 layers, projection), blocked states in and out: write-through
stores -- or, for the plain-store variant of the kernel, two row-major cells without MLP.  Edge rows 1, 16, 17 and 47 (one
lane, a full tile, a tile plus one row, three tiles with a ragged end) at d = 32 and 64; the vertex task has as many rows,
3 beside the 47 (the fixture's size limit; three tiles of the ticket loop are the edge task's).  z_centered on and off, c == NULL.

Planted rows (the last three of a task; a one-row task takes one kind per launch), where a contracted or re-associated
operation shows first:
  "flat"  every gate pre-activation of the row equal: variance 0, the rows the range guard ignores.  h = x = 0; gather-init sums
          two constant source rows (0.5 and 0.25, exact through the mean pass), bias-init has zscale = 0.
  "sat"   z = 0 except one column per gate, at -5000 (gates i, f, o; +5000 for j), whose gamma is 30 for i, f, o: the
          normalised value -sqrt(d - 1) times gamma makes 2^t overflow and the reciprocal return 0.  (h[row, 0] = 100 against
          K[dx, gate * d] = -+50; column 0 of h is 0 in every other row.)
  "tiny"  z of subnormal size: gather-init sums two source rows of 1e-40-sized values, bias-init has zscale = 1e-42.
The range guard raises its low-variance bit on these; the flag word is part of the fixture."""
import numpy as np
import torch

from cell_fwd_cases import FwdCell

KINDS = ("flat", "sat", "tiny")
N_SRC = 64          # ordinary gather sources; rows N_SRC .. N_SRC + 5 are the planted rows' own
ROWS = (1, 16, 17, 47)
WIDTHS = (32, 64)


def _plant(cell, row, kind, rng):
    d, dx = cell.d, cell.dx
    cell.h[row] = 0.0
    if dx:
        cell.x[row] = 0.0
    if cell.mode == "bias":
        cell.zscale[row] = 0.0
    if cell.mode == "gather":
        cell.uv[row] = (N_SRC + 2, N_SRC + 2)              # a zero source row
    if kind == "flat":
        if cell.mode == "gather":
            cell.uv[row] = (N_SRC, N_SRC + 1)
    elif kind == "sat":
        cell.h[row, 0] = 100.0
    elif kind == "tiny":
        if cell.mode == "gather":
            cell.uv[row] = (N_SRC + 3, N_SRC + 4)
        elif cell.mode == "bias":
            cell.zscale[row] = 1e-42
    else:
        raise ValueError(kind)


def _prepare(cell, kinds, rng):
    """Plants `kinds` in the last len(kinds) rows of the cell; the operands every row shares are set for all of them."""
    d, dx = cell.d, cell.dx
    cell.h[:, 0] = 0.0
    for gate, w in enumerate((-50.0, 50.0, -50.0, -50.0)):
        cell.K[dx, gate * d] = w
    for gate in (0, 2, 3):                                   # GATES: input, transform, forget, output, state
        cell.ln[gate, 0, 0] = 30.0
    if cell.mode == "gather":
        cell.uv = np.stack([rng.randint(0, N_SRC, cell.rows), rng.randint(0, N_SRC, cell.rows)], 1).astype(np.int32)
        cell.Zx[N_SRC], cell.Zx[N_SRC + 1], cell.Zx[N_SRC + 2] = 0.5, 0.25, 0.0
        cell.Zx[N_SRC + 3] = (1e-40 * rng.randn(4 * d)).astype(np.float32)
        cell.Zx[N_SRC + 4] = (1e-40 * rng.randn(4 * d)).astype(np.float32)
    for i, kind in enumerate(kinds):
        _plant(cell, cell.rows - len(kinds) + i, kind, rng)
    return cell


def _kinds(rows, one):
    return (one,) if rows < 3 else KINDS


def step_launch(d, rows, seed, centred=False, null_c=False, one="flat"):
    """The two-task launch of a step -> [edge cell, vertex cell]."""
    v_rows = rows if rows <= 17 else 3
    rng = np.random.RandomState(seed)
    edge = FwdCell("h2", d, rows, seed + 1, mode="gather", mlp_layers=3, in_blocked=True, out_blocked=True, null_c=null_c,
                   n_src=N_SRC + 6)
    vert = FwdCell("h2", d, v_rows, seed + 2, dx=d, mode="bias", mlp_layers=4, relu_mask=0b0111, proj=True, mlp_out=False,
                   in_blocked=True, out_blocked=True, null_c=null_c)
    cells = [_prepare(edge, _kinds(rows, one), rng), _prepare(vert, _kinds(v_rows, one), rng)]
    return [c.centred() for c in cells] if centred else cells


def plain_launch(d, rows, seed, one="flat"):
    """Row-major states, no MLP: the launcher picks the plain-store variant -> [bias-init cell, gather-init cell]."""
    rng = np.random.RandomState(seed)
    a = FwdCell("h2", d, rows, seed + 1, dx=d, mode="bias")
    b = FwdCell("h2", d, rows, seed + 2, mode="gather", n_src=N_SRC + 6)
    return [_prepare(a, _kinds(rows, one), rng), _prepare(b, _kinds(rows, one), rng)]


def cases():
    """-> [(id, write-through expected, centred expected, builder of the launch's cells)]"""
    out = []
    for d in WIDTHS:
        for rows in ROWS:
            for one in (KINDS if rows == 1 else ("flat",)):
                name = "step-d%d-r%d" % (d, rows) + ("-" + one if rows == 1 else "")
                out.append((name, True, False, lambda d=d, rows=rows, one=one: step_launch(d, rows, 100 * d + rows, one=one)))
        out.append(("step-d%d-r17-centred" % d, True, True, lambda d=d: step_launch(d, 17, 100 * d + 51, centred=True)))
        out.append(("step-d%d-r1-nullc" % d, True, False, lambda d=d: step_launch(d, 1, 100 * d + 52, null_c=True, one="sat")))
    out.append(("plain-d32-r1", False, False, lambda: plain_launch(32, 1, 3253, one="tiny")))
    out.append(("plain-d64-r17", False, False, lambda: plain_launch(64, 17, 6453)))
    return out


def run_case(build, device, wt, centred):
    """Launches the case -> {"<task>.<output>": uint32 bit patterns (numpy), "<task>.flag": the range_flag word}."""
    from plan_replay import cell_fwd_plan
    from tspgnn import _lib
    cells = build()
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    p = cell_fwd_plan([c.plan() for c in cells], cells[0].d, cus, "h2")
    assert bool(p.wt) == wt and bool(p.centered) == centred, (p.wt, p.centered)
    _lib.call_multi("tspgnn_lnlstm_mlp_fwd_multi_h2", [c.task(device) for c in cells], cells[0].d)
    torch.cuda.synchronize()
    got = {}
    for k, c in enumerate(cells):
        assert not c.unwritten() and not c.untouched(), (c.unwritten(), c.untouched())
        for n, t in c.outputs().items():
            got["%d.%s" % (k, n)] = t.contiguous().cpu().numpy().view(np.uint32)
        got["%d.flag" % k] = np.array([c.range_flag()], dtype=np.uint32)
    return got
