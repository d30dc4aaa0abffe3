"""The library still answers tests/golden/launch_plans.json: every planner of csrc/launch_plan.h over a grid that crosses
its thresholds (tools/launch_plan_table.py lists the grid and rewrites the table after a deliberate launcher
change).  The table was first recorded from the Python restatement of the launchers that tests/plan_replay.py held before
the planners existed, and the library's dump equalled it byte for byte.  No device."""
import importlib.util
import json
import os

import pytest

import plan_replay
from conftest import GOLDEN, ROOT
from tspgnn import _lib


def generator():
    spec = importlib.util.spec_from_file_location("launch_plan_table", os.path.join(ROOT, "tools", "launch_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_library_answers_the_recorded_table():
    gen = generator()
    want = json.load(open(os.path.join(GOLDEN, "launch_plans.json")))
    got = json.loads(gen.dumps(gen.table(plan_replay)))
    assert sorted(got) == sorted(want)
    for name in want:
        assert len(got[name]) == len(want[name]), name
        for g, w in zip(got[name], want[name]):
            assert g == w, (name, w[0])
    assert gen.dumps(gen.table(plan_replay)) == open(os.path.join(GOLDEN, "launch_plans.json")).read()


def test_the_table_reaches_every_branch():
    """What the grid is for: each path, mode, split and variant occurs in it, the unsupported x3 shapes included."""
    tab = json.load(open(os.path.join(GOLDEN, "launch_plans.json")))
    assert {r[1][0] for r in tab["linear"]} == {"split", "ticket", "streamed"}
    assert {r[1][0] for r in tab["wgrad"]} == {"generic", "x3"}
    assert {(r[1][1], r[1][2]) for r in tab["wgrad"]} >= {(a, b) for a in (1, 2, 4) for b in (1, 2, 4)}
    assert {r[1][3] for r in tab["wcolsum"]} == {False, True}
    assert {r[1][0] for r in tab["mlp_fwd"]} == {4, 8, 16} and {r[1][0] for r in tab["mlp_bwd"]} == {4, 8}
    for arith in ("h2", "x3"):
        recs = [r for r in tab["cell_fwd"] if r[0][3] == arith]
        plans = [r[1] for r in recs if r[1] != "unsupported"]
        assert {p[0] for p in plans} == {4, 8, 12} and {p[3] for p in plans} == {"fixed", "plain"}
        assert {t[0] for p in plans for t in p[7]} == {"resident", "lockstep"}
        assert {len(r[0][0]) for r in recs} == {1, 2, 3, 4}
        if arith == "h2":
            assert {p[4] for p in plans} == {False, True} and {p[5] for p in plans} == {False, True}
            assert len(plans) == len(recs)
        else:
            assert len(plans) < len(recs) and not any(p[4] or p[5] for p in plans)
    # the cell backward launchers: both wavefront counts, K resident and chunked, each refusal; per record
    # [nw, grid, blocks, qc, chunked, lds_bytes]
    for arith, nws, declined in (("f32", {4, 8}, {"unsupported", "invalid"}), ("h2", {4, 8}, {"unsupported", "invalid"}),
                                 ("bf16", {4, 8}, set())):
        recs = [r for r in tab["cell_bwd"] if r[0][3] == arith]
        plans = [r[1] for r in recs if not isinstance(r[1], str)]
        assert {r[1] for r in recs if isinstance(r[1], str)} == declined, arith
        assert {p[0] for p in plans} == nws and {len(r[0][0]) for r in recs} >= {1, 2, 3, 4}
        assert {c for p in plans for c in p[4]} == ({False} if arith == "h2" else {False, True})
        assert all(p[0] == 8 for r, p in ((r, r[1]) for r in recs if not isinstance(r[1], str))
                   if arith == "f32" and r[0][1] == 64 and any(p[4]))       # a chunked fp32 task keeps all eight wavefronts
    for d in (32, 64, 128):
        assert {c for r in tab["lstm_fwd_bf16"] if r[0][1] == d for c in r[1][4]} == {False, True}
        assert {r[1][0] for r in tab["lstm_fwd_bf16"] if r[0][1] == d} == set(plan_replay.LSTM_FWD_BF16_NW[d])
    assert {r[1][0] for r in tab["mlp_fwd_bf16"]} == {8, 16} and not any(isinstance(r[1], str) for r in tab["mlp_fwd_bf16"])
    assert {(r[0][0][0][1], r[0][0][0][2]) for r in tab["mlp_fwd_bf16"] if len(r[0][0]) == 1} == {(L, p) for L in (1, 2, 3, 4) for p in (False, True)}
    # the fp32 forward launchers.  MLP, per record [nw, grid, blocks]: 16 wavefronts only where two workgroups fit a CU
    mlp = [r for r in tab["mlp_fwd_f32"] if not isinstance(r[1], str)]
    for d, nws in ((32, {4, 8, 16}), (64, {4, 8, 16}), (128, {4, 8})):
        assert {r[1][0] for r in mlp if r[0][1] == d} == nws, d
    assert {len(r[0][0]) for r in mlp} == {1, 2, 3, 4} and all(min(r[1][2]) >= 1 for r in mlp)
    assert [r[0][1] for r in tab["mlp_fwd_f32"] if r[1] == "invalid"] == [128, 128]       # three layers, a projection
    assert not any(r[1] == "unsupported" for r in tab["mlp_fwd_f32"])
    # cell, per record [nw, grid, blocks, qc, chunked, lds_bytes, chunks, chunk_grid, rounds_per_wg]
    recs = tab["lstm_fwd_f32"]
    plans = [r[1] for r in recs if not isinstance(r[1], str)]
    assert {p[0] for p in plans if p[1]} == {4, 8} and {c for p in plans for c in p[4]} == {False, True}
    assert {len([t for t in r[0][0] if t[0]]) for r in recs} == {1, 2, 3, 4}
    assert {r[1] for r in recs if isinstance(r[1], str)} == {"unsupported", "invalid"}
    mixed = [p for p in plans if len(set(p[4])) == 2]
    assert mixed and all(p[1] > 0 and all((b == 0) == c for b, c in zip(p[2], p[4])) for p in mixed)    # resident together, chunked apart
    assert any(len(set(ch)) == 2 for p in plans for ch in p[6] if ch)                       # a last chunk shorter than qc
    assert {lo != hi for p in plans for w in p[8] if w for lo, hi in [w]} == {False, True}  # workgroups that stride over rounds
    for r in recs:          # a chunked gather-init / bias-init task: refused whatever else the launch holds
        if r[0][1] != 128 or all(t[2] != "gather" for t in r[0][0]):
            fits = lambda t: (t[1] + r[0][1]) * 16 * r[0][1] + 40 * r[0][1] + 16 <= 160 * 1024
            assert (r[1] == "unsupported") == any(t[2] != "plain" and not fits(t) for t in r[0][0]), r[0]


def test_queries_validate_as_their_entries_do():
    """TSPGNN_EINVAL (-1) for the shape fields the entries reject, TSPGNN_EUNSUPPORTED (-2) exactly where the launch
    answers it, a zeroed plan where nothing would be launched."""
    def status(query, *args):
        try:
            _lib.plan(query, *args)
            return 0
        except _lib.TspgnnError as e:
            return e.status
    assert status("tspgnn_plan_linear", 24, 0, 64, 100, 256) == -1 and status("tspgnn_plan_linear", 64, 16, 16, 100, 256) == -1
    assert status("tspgnn_plan_wgrad", 100, 24, 64, 0, 256) == -1 and status("tspgnn_plan_wgrad", 100, 32, 64, 1, 256) == -2
    assert status("tspgnn_plan_wcolsum", 100, 24, 256) == -1 and status("tspgnn_plan_einit_bwd", 100, 48, 256) == -1
    assert status("tspgnn_plan_mlp_bwd", [_lib.MlpBwdTask(rows=5, n_layers=3)], 1, 128, 256) == -2
    assert status("tspgnn_plan_mlp_bwd", [_lib.MlpBwdTask(rows=5, n_layers=5)], 1, 64, 256) == -1
    assert status("tspgnn_plan_mlp_fwd", [_lib.MlpTask(rows=5, n_layers=0)], 1, 64, 256) == -1
    cell = lambda **k: [_lib.CellMlpTask(cell=_lib.LstmTask(rows=k.pop("rows", 5), dx=k.pop("dx", 0)), **k)]
    assert status("tspgnn_plan_cell_fwd", cell(dx=48), 1, 64, 0, 256) == -1
    assert status("tspgnn_plan_cell_fwd", cell(mlp_layers=5), 1, 64, 0, 256) == -1
    assert status("tspgnn_plan_cell_fwd", cell(), 1, 48, 0, 256) == -1 and status("tspgnn_plan_cell_fwd", cell(), 1, 64, 2, 256) == -1
    assert status("tspgnn_plan_cell_fwd", cell(mlp_layers=1, proj_w=1), 1, 32, 1, 256) == -2     # one k-block, no lock step
    assert status("tspgnn_plan_cell_fwd", cell(mlp_layers=1, proj_w=1), 1, 32, 0, 256) == 0
    bwd = lambda **k: [_lib.LstmBwdTask(rows=k.pop("rows", 5), **k)]
    assert status("tspgnn_plan_cell_bwd", bwd(), 1, 64, 1, 256) == -1                      # no bf16x3 backward
    assert status("tspgnn_plan_cell_bwd", bwd(), 1, 128, 0, 256) == -1 and status("tspgnn_plan_cell_bwd", bwd(), 1, 128, 2, 256) == 0
    assert status("tspgnn_plan_cell_bwd", bwd(dx=16), 1, 64, 2, 256) == 0 and status("tspgnn_plan_cell_bwd", bwd(dx=16), 1, 64, 3, 256) == -1
    assert status("tspgnn_plan_cell_bwd", bwd(KT=1), 1, 64, 0, 256) == -1 and status("tspgnn_plan_cell_bwd", bwd(KT=1, dxh=1), 1, 64, 0, 256) == 0
    assert status("tspgnn_plan_cell_bwd", bwd(KT=1), 1, 64, 3, 256) == -1 and status("tspgnn_plan_cell_bwd", bwd(zbias=1), 1, 64, 2, 256) == -1
    assert status("tspgnn_plan_cell_bwd", bwd(rows=1 << 23), 1, 64, 0, 256) == -1 and status("tspgnn_plan_cell_bwd", bwd(rows=1 << 23), 1, 64, 2, 256) == 0
    assert status("tspgnn_plan_cell_bwd", bwd(KT=1), 1, 32, 2, 256) == -2 and status("tspgnn_plan_cell_bwd", bwd(dx=96), 1, 64, 0, 256) == -2
    assert status("tspgnn_plan_lstm_fwd_bf16", [_lib.LstmTaskB(rows=5, dx=48)], 1, 64, 12, 256) == -1
    assert status("tspgnn_plan_lstm_fwd_bf16", [_lib.LstmTaskB(rows=5)], 1, 48, 8, 256) == -1
    assert status("tspgnn_plan_lstm_fwd_bf16", [_lib.LstmTaskB(rows=5)], 1, 64, 0, 256) == -1
    assert status("tspgnn_plan_mlp_fwd_bf16", [_lib.MlpTaskB(rows=5, n_layers=5)], 1, 64, 8, 256) == -1
    assert status("tspgnn_plan_mlp_fwd_bf16", [_lib.MlpTaskB(rows=5, n_layers=2)], 1, 64, 8, -1) == -1
    assert status("tspgnn_plan_linear", 64, 0, 64, 100, -1) == -1
    f32 = lambda **k: [_lib.MlpTask(rows=k.pop("rows", 5), n_layers=k.pop("n_layers", 2), **k)]
    assert status("tspgnn_plan_mlp_fwd_f32", f32(), 1, 48, 256) == -1 and status("tspgnn_plan_mlp_fwd_f32", f32(n_layers=5), 1, 64, 256) == -1
    assert status("tspgnn_plan_mlp_fwd_f32", f32(n_layers=3), 1, 128, 256) == -1 and status("tspgnn_plan_mlp_fwd_f32", f32(n_layers=3, rows=0), 1, 128, 256) == -1
    assert status("tspgnn_plan_mlp_fwd_f32", f32(proj_w=1), 1, 64, 256) == -1 and status("tspgnn_plan_mlp_fwd_f32", f32(proj_w=1, proj_out=1), 1, 128, 256) == -1
    assert status("tspgnn_plan_mlp_fwd_f32", f32(proj_w=1, proj_out=1), 1, 64, 256) == 0 and status("tspgnn_plan_mlp_fwd_f32", f32(), 1, 64, -1) == -1
    assert status("tspgnn_plan_mlp_fwd_f32", f32() * 5, 5, 64, 256) == -1
    lstm = lambda **k: [_lib.LstmTask(rows=k.pop("rows", 5), **k)]
    assert status("tspgnn_plan_lstm_fwd_f32", lstm(dx=8), 1, 64, 256) == -1 and status("tspgnn_plan_lstm_fwd_f32", lstm(dx=16), 1, 64, 256) == 0
    assert status("tspgnn_plan_lstm_fwd_f32", lstm(), 1, 48, 256) == -1 and status("tspgnn_plan_lstm_fwd_f32", lstm(rows=-1), 1, 64, 256) == -1
    assert status("tspgnn_plan_lstm_fwd_f32", lstm(uv=1), 1, 64, 256) == -1 and status("tspgnn_plan_lstm_fwd_f32", lstm(uv=1, Zx=1), 1, 64, 256) == 0
    assert status("tspgnn_plan_lstm_fwd_f32", lstm(uv=1, Zx=1), 1, 128, 256) == -1 and status("tspgnn_plan_lstm_fwd_f32", lstm(uv=1, Zx=1, dx=16), 1, 64, 256) == -1
    assert status("tspgnn_plan_lstm_fwd_f32", lstm(zbias=1), 1, 64, 256) == -1 and status("tspgnn_plan_lstm_fwd_f32", lstm(zbias=1, zscale=1), 1, 64, 256) == 0
    assert status("tspgnn_plan_lstm_fwd_f32", lstm(zbias=1, zscale=1, dx=80), 1, 64, 256) == 0
    assert status("tspgnn_plan_lstm_fwd_f32", lstm(zbias=1, zscale=1, dx=96), 1, 64, 256) == -2      # a chunked K starts z at zero
    assert status("tspgnn_plan_lstm_fwd_f32", lstm(dx=192) + lstm(zbias=1, zscale=1), 2, 128, 256) == -2
    assert status("tspgnn_plan_lstm_fwd_f32", lstm(dx=192) + lstm(zbias=1, zscale=1), 2, 64, 256) == 0    # only the task that does not fit
    assert _lib.plan("tspgnn_plan_mlp_fwd_f32", f32(rows=0), 1, 64, 256).grid == 0
    assert _lib.plan("tspgnn_plan_lstm_fwd_f32", lstm(rows=0, dx=192, zbias=1, zscale=1), 1, 64, 256).nw == 0
    assert _lib.plan("tspgnn_plan_linear", 64, 0, 64, 0, 256).grid == 0
    assert _lib.plan("tspgnn_plan_wgrad", 0, 64, 64, 0, 256).n_chunks == 0
    assert _lib.plan("tspgnn_plan_cell_fwd", cell(rows=0), 1, 64, 0, 256).grid == 0
    assert _lib.plan("tspgnn_plan_cell_bwd", bwd(rows=0), 1, 64, 0, 256).grid == 0
    assert _lib.plan("tspgnn_plan_lstm_fwd_bf16", [_lib.LstmTaskB(rows=0)], 1, 64, 12, 256).grid == 0
    assert _lib.plan("tspgnn_plan_mlp_fwd_bf16", [_lib.MlpTaskB(rows=0, n_layers=2)], 1, 64, 8, 256).grid == 0


def queries_at(cus):
    """One shape per planner."""
    cell = [_lib.CellMlpTask(cell=_lib.LstmTask(rows=99840), mlp_layers=3, mlp_out=1, state_out_blocked=1),
            _lib.CellMlpTask(cell=_lib.LstmTask(rows=5120, dx=64), mlp_layers=4, proj_w=1, proj_out=1, mlp_out=1)]
    calls = [("tspgnn_plan_linear", 256, 64, 64, 131073, cus), ("tspgnn_plan_wgrad", 99840, 64, 64, 0, cus),
             ("tspgnn_plan_wgrad", 99840, 128, 64, 1, cus), ("tspgnn_plan_wcolsum", 5094400, 64, cus),
             ("tspgnn_plan_einit_bwd", 99840, 64, cus),
             ("tspgnn_plan_mlp_bwd", [_lib.MlpBwdTask(rows=333, n_layers=2), _lib.MlpBwdTask(rows=131073, n_layers=2)], 2, 64, cus),
             ("tspgnn_plan_mlp_fwd", [_lib.MlpTask(rows=9000, n_layers=3), _lib.MlpTask(rows=700, n_layers=4, proj_w=1)], 2, 64, cus),
             ("tspgnn_plan_cell_fwd", cell, 2, 64, 0, cus), ("tspgnn_plan_cell_fwd", cell, 2, 64, 1, cus)]
    bwd = [_lib.LstmBwdTask(rows=5120, dx=64), _lib.LstmBwdTask(rows=99840)]
    calls += [("tspgnn_plan_cell_bwd", bwd, 2, 64, arith, cus) for arith in (0, 2, 3)]
    calls += [("tspgnn_plan_lstm_fwd_bf16", [_lib.LstmTaskB(rows=99840), _lib.LstmTaskB(rows=5120, dx=64)], 2, 64, 12, cus),
              ("tspgnn_plan_mlp_fwd_bf16", [_lib.MlpTaskB(rows=9000, n_layers=3), _lib.MlpTaskB(rows=700, n_layers=4, proj_w=1)], 2, 64, 8, cus)]
    calls += [("tspgnn_plan_mlp_fwd_f32", [_lib.MlpTask(rows=9000, n_layers=3), _lib.MlpTask(rows=700, n_layers=4, proj_w=1, proj_out=1)], 2, 64, cus),
              ("tspgnn_plan_lstm_fwd_f32", [_lib.LstmTask(rows=99840, uv=1, Zx=1), _lib.LstmTask(rows=5120, dx=64, zbias=1, zscale=1),
                                            _lib.LstmTask(rows=65537, dx=192)], 3, 64, cus)]
    return [bytes(_lib.plan(*c)) for c in calls]


def test_cus_zero_is_256_without_a_device():
    import torch
    if torch.cuda.is_available():
        return          # (with a device: test_cus_zero_is_the_devices_count)
    assert queries_at(0) == queries_at(256) != queries_at(64)


@pytest.mark.gpu
def test_cus_zero_is_the_devices_count(cuda_device):
    """cus == 0 -- the count the launchers take from n_cus() -- is torch's multi_processor_count, from which the GPU tests
    derive their row counts.  Launches nothing."""
    import torch
    cus = torch.cuda.get_device_properties(cuda_device).multi_processor_count
    assert queries_at(0) == queries_at(cus) != queries_at(cus + 8)
