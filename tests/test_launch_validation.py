"""Argument validation of the multi-task entry points (tspgnn_*_multi_*, tspgnn_mlp_head_fwd_h2) without a GPU.

Every entry validates its tasks before its first HIP call, so with pointers that are not memory (never dereferenced)
each rejection -- status AND the full tspgnn_last_error() text, prefix included -- can be pinned on a machine without a
device.  Every case here is one that validation rejects (-1 / -2) or one with no live task (0: nothing is launched); an
accepted call would go on to launch, so none is made.  For the same reason the module skips itself where a device is
present: a validation regression must never turn a fake pointer into a kernel launch.
"""
import ctypes

import pytest
import torch

from tspgnn import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(),
                                reason="host-side validation with fake pointers: runs only where nothing can launch")

A, B, C, D, F = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000   # distinct addresses, never dereferenced
BIG = (1 << 30) // 256                                    # rows with rows * 4 * 64 == 2^30

CASES = []


def case(cid, entry, tasks, d, status, message, n=None):
    CASES.append(pytest.param(entry, tasks, d, n, status, message, id="%s-%s" % (entry.replace("tspgnn_", ""), cid)))


def mlp(cls=_lib.MlpTask, **kw):
    f = dict(X=A, wb=F, Y=B, rows=16, n_layers=2)
    f.update(kw)
    return cls(**f)


def mlp_b(**kw):
    return mlp(_lib.MlpTaskB, **kw)


def lstm(cls=_lib.LstmTask, **kw):
    f = dict(x=None, dx=0, h=A, c=B, K=F, ln=F, h_out=C, c_out=D, rows=16)
    f.update(kw)
    return cls(**f)


def lstm_b(**kw):
    return lstm(_lib.LstmTaskB, **kw)


def cell(mlp_fields=None, **kw):
    return _lib.CellMlpTask(cell=lstm(**kw), **(mlp_fields or {}))


def lstm_bwd(**kw):
    f = dict(x=None, dx=0, h=A, c=B, K=F, ln=F, dh_out=F, dc_out=F, dz=C, dc_in=D, ln_grad=F, workspace=F, rows=16)
    f.update(kw)
    return _lib.LstmBwdTask(**f)


def mlp_bwd(**kw):
    f = dict(dY=A, wt=F, rows=16, n_layers=2)
    f.update(kw)
    return _lib.MlpBwdTask(**f)


def common(entry, make, count, d_msg, bad_d):
    """n_tasks 0 and 5, a null array, unsupported widths, the empty launch, rows = -1."""
    count_msg = "%s: 1..4 tasks" % count
    case("n_tasks=0", entry, [make()] * 5, 64, -1, count_msg, n=0)
    case("n_tasks=5", entry, [make()] * 5, 64, -1, count_msg, n=5)
    case("null-array", entry, None, 64, -1, count_msg, n=1)
    for d in bad_d:
        case("d=%d" % d, entry, [make()], d, -1, d_msg % d)
    case("all-empty", entry, [make(rows=0), make(rows=0)], 64, 0, None)


# ------------------------------------------------------------------------------------------------ MLP forward
for entry, make, count, p, d_list, bad_d in (
        ("tspgnn_mlp_fwd_multi_f32", mlp, "mlp_fwd_multi", "mlp_fwd", "32, 64 or 128", (48,)),
        ("tspgnn_mlp_fwd_multi_h2", mlp, "mlp_fwd_multi_h2", "mlp_fwd_h2", "32 or 64", (48, 128)),
        ("tspgnn_mlp_fwd_multi_x3", mlp, "mlp_fwd_multi_x3", "mlp_fwd_x3", "32 or 64", (48, 128)),
        ("tspgnn_mlp_fwd_multi_bf16", mlp_b, "mlp_fwd_multi_bf16", "mlp_fwd_bf16", "32, 64 or 128", (48,))):
    common(entry, make, count, p + ": d=%d must be " + d_list, bad_d)
    case("rows=-1", entry, [make(rows=-1)], 64, -1, p + ": rows=-1")
    for L in (0, 5, 9):
        case("n_layers=%d" % L, entry, [make(n_layers=L)], 64, -1, "%s: n_layers=%d must be in 1..4" % (p, L))
        case("n_layers=%d-empty" % L, entry, [make(rows=0, n_layers=L)], 64, -1,
             "%s: n_layers=%d must be in 1..4" % (p, L))
    for field in ("X", "wb", "Y"):
        case("null-" + field, entry, [make(), make(**{field: None})], 64, -1, p + ": null pointer")
    case("proj-without-out", entry, [make(proj_w=F)], 64, -1,
         p + ": projection needs proj_out" + (" and d in {32,64}" if p == "mlp_fwd" else ""))

for L in (3, 4):
    for rows in (16, 0):
        case("d=128-layers=%d-rows=%d" % (L, rows), "tspgnn_mlp_fwd_multi_f32", [mlp(n_layers=L, rows=rows)], 128, -1,
             "mlp_fwd: d=128 holds at most 2 layers in LDS (got %d)" % L)
case("proj-d=128", "tspgnn_mlp_fwd_multi_f32", [mlp(proj_w=F, proj_out=F)], 128, -1,
     "mlp_fwd: projection needs proj_out and d in {32,64}")
case("acts_stride=-1", "tspgnn_mlp_fwd_multi_bf16", [mlp_b(acts=F, acts_stride=-1)], 64, -1, "mlp_fwd_bf16: acts_stride=-1")
case("interleaved-proj", "tspgnn_mlp_fwd_multi_bf16", [mlp_b(y_interleaved=1, proj_w=F, proj_out=F)], 64, -1,
     "mlp_fwd_bf16: y_interleaved excludes a projection and saved activations")
case("interleaved-acts", "tspgnn_mlp_fwd_multi_bf16", [mlp_b(y_interleaved=1, acts=F)], 64, -1,
     "mlp_fwd_bf16: y_interleaved excludes a projection and saved activations")

# ------------------------------------------------------------------------------------------------ LN-LSTM forward, f32 / bf16
for entry, make, count, p, mult in (("tspgnn_lnlstm_fwd_multi_f32", lstm, "lnlstm_fwd_multi", "lnlstm_fwd", 16),
                                    ("tspgnn_lnlstm_fwd_multi_bf16", lstm_b, "lnlstm_fwd_multi_bf16", "lnlstm_fwd_bf16", 32)):
    common(entry, make, count, p + ": d=%d must be 32, 64 or 128", (48,))
    case("rows=-1", entry, [make(rows=-1)], 64, -1, p + ": rows=-1")
    for dx in (mult // 2, -mult):
        for rows in (16, 0):
            case("dx=%d-rows=%d" % (dx, rows), entry, [make(x=F, dx=dx, rows=rows)], 64, -1,
                 "%s: dx=%d must be a non-negative multiple of %d" % (p, dx, mult))
    for field in ("h", "c", "K", "ln", "h_out", "c_out"):
        if field == "c" and make is lstm_b:
            continue    # (c == NULL is the zero cell state of a first step there)
        case("null-" + field, entry, [make(), make(**{field: None})], 64, -1, p + ": null pointer")
    case("null-x", entry, [make(dx=mult)], 64, -1, p + ": null pointer")
    case("h_out=h", entry, [make(h_out=A)], 64, -1, p + ": outputs may not alias inputs")
    case("c_out=c", entry, [make(), make(c_out=B)], 64, -1, p + ": outputs may not alias inputs")
    gather = p + ": gather-init mode needs dx == 0" + (", Zx and d in {32,64}" if make is lstm else " and Zx")
    case("gather-dx", entry, [make(uv=F, Zx=F, x=F, dx=mult)], 64, -1, gather)
    case("gather-no-Zx", entry, [make(uv=F)], 64, -1, gather)

case("gather-d=128", "tspgnn_lnlstm_fwd_multi_f32", [lstm(uv=F, Zx=F)], 128, -1,
     "lnlstm_fwd: gather-init mode needs dx == 0, Zx and d in {32,64}")
case("zbias-no-zscale", "tspgnn_lnlstm_fwd_multi_f32", [lstm(zbias=F)], 64, -1,
     "lnlstm_fwd: zbias needs zscale and excludes gather-init mode")
case("zbias-gather", "tspgnn_lnlstm_fwd_multi_f32", [lstm(zbias=F, zscale=F, uv=F, Zx=F)], 64, -1,
     "lnlstm_fwd: zbias needs zscale and excludes gather-init mode")
# A bias-init task whose K does not fit LDS (the chunked kernel starts z at zero): TSPGNN_EUNSUPPORTED from the launch's plan,
# before its first HIP call -- also behind a task that could have run (plain, chunked) and behind one that fits.  (A
# gather-init task has dx == 0 and d <= 64: its K always fits.)
for cid, tasks, d in (("bias-chunked", [lstm(x=F, dx=96, zbias=F, zscale=F)], 64),
                      ("bias-chunked-d=32", [lstm(x=F, dx=288, zbias=F, zscale=F)], 32),
                      ("bias-chunked-d=128", [lstm(zbias=F, zscale=F)], 128),
                      ("chunked-then-bias-chunked", [lstm(x=F, dx=192), lstm(x=F, dx=192, zbias=F, zscale=F)], 64),
                      ("resident-then-bias-chunked", [lstm(uv=F, Zx=F), lstm(x=F, dx=64), lstm(x=F, dx=96, zbias=F, zscale=F)], 64)):
    case(cid, "tspgnn_lnlstm_fwd_multi_f32", tasks, d, -2,
         "lnlstm_fwd: gather-init / zbias need K[%d,%d] resident in LDS" % (d, 4 * d))
# (the alias check runs on empty tasks too: NULL == NULL)
case("empty-null-task", "tspgnn_lnlstm_fwd_multi_f32", [_lib.LstmTask()], 64, -1, "lnlstm_fwd: outputs may not alias inputs")
case("empty-null-task", "tspgnn_lnlstm_fwd_multi_bf16", [_lib.LstmTaskB()], 64, 0, None)

# ------------------------------------------------------------------------------------------------ cell (+ MLP) forward, h2 / x3
for arith in ("h2", "x3"):
    for entry, make, count in (
            ("tspgnn_lnlstm_fwd_multi_" + arith, lstm, "lnlstm_fwd_multi_" + arith),
            ("tspgnn_lnlstm_mlp_fwd_multi_" + arith, cell, "tspgnn_lnlstm_mlp_fwd_multi_" + arith)):
        p = entry
        common(entry, make, count, p + ": d=%d must be 32 or 64", (48, 128))
        case("rows=-1", entry, [make(rows=-1)], 64, -1, p + ": rows=-1")
        for rows, d in ((BIG, 64), (2 * BIG, 32)):
            case("rows=%d-d=%d" % (rows, d), entry, [make(rows=rows)], d, -1,
                 "%s: rows=%d too large for 32-bit offsets" % (p, rows))
        case("rows*dx", entry, [make(x=F, dx=512, rows=BIG // 2)], 64, -1,
             "%s: rows=%d too large for 32-bit offsets" % (p, BIG // 2))
        for dx in (16, -32):
            for rows in (16, 0):
                case("dx=%d-rows=%d" % (dx, rows), entry, [make(x=F, dx=dx, rows=rows)], 64, -1,
                     "%s: dx=%d must be a non-negative multiple of 32" % (p, dx))
        for field in ("h", "c", "K", "ln", "h_out", "c_out"):
            if field == "c" and arith == "h2":
                continue    # (c == NULL is the zero cell state of a first step there)
            case("null-" + field, entry, [make(), make(**{field: None})], 64, -1, p + ": null pointer")
        case("null-x", entry, [make(dx=32)], 64, -1, p + ": null pointer")
        if arith == "x3":   # (in place is accepted by the h2 entries: not called)
            case("h_out=h", entry, [make(h_out=A)], 64, -1, p + ": outputs may not alias inputs")
            case("c_out=c", entry, [make(), make(c_out=B)], 64, -1, p + ": outputs may not alias inputs")
        case("gather-dx", entry, [make(uv=F, Zx=F, x=F, dx=32)], 64, -1, p + ": gather-init mode needs dx == 0 and Zx")
        case("gather-no-Zx", entry, [make(uv=F)], 64, -1, p + ": gather-init mode needs dx == 0 and Zx")
        case("zbias-no-zscale", entry, [make(zbias=F)], 64, -1, p + ": zbias needs zscale and excludes gather-init mode")
        case("zbias-gather", entry, [make(zbias=F, zscale=F, uv=F, Zx=F)], 64, -1,
             p + ": zbias needs zscale and excludes gather-init mode")

    entry = p = "tspgnn_lnlstm_mlp_fwd_multi_" + arith
    for L in (-1, 5):
        for rows in (16, 0):
            case("mlp_layers=%d-rows=%d" % (L, rows), entry, [cell(dict(mlp_wb=F, mlp_layers=L), rows=rows)], 64, -1,
                 "%s: mlp_layers=%d must be in 0..4" % (p, L))
    case("layers-without-wb", entry, [cell(dict(mlp_layers=2))], 64, -1, p + ": mlp_layers > 0 needs mlp_wb")
    case("proj-without-out", entry, [cell(dict(mlp_wb=F, mlp_layers=2, proj_w=F))], 64, -1,
         p + ": a projection needs proj_out and at least one MLP layer")
    case("proj-without-layers", entry, [cell(dict(proj_w=F, proj_out=F))], 64, -1,
         p + ": a projection needs proj_out and at least one MLP layer")

p = "tspgnn_lnlstm_mlp_fwd_multi_x3"
case("state_in_blocked", p, [cell(dict(state_in_blocked=1))], 64, -1, p + ": blocked states are an f16x2 feature")
case("state_out_blocked", p, [cell(dict(state_out_blocked=1))], 64, -1, p + ": blocked states are an f16x2 feature")
case("mlp_acts", p, [cell(dict(mlp_wb=F, mlp_layers=2, mlp_acts=F))], 64, -1,
     p + ": saving the MLP's hidden activations is an f16x2 feature")
p = "tspgnn_lnlstm_mlp_fwd_multi_h2"
case("mlp_acts_stride=-1", p, [cell(dict(mlp_wb=F, mlp_layers=2, mlp_acts=F, mlp_acts_stride=-1))], 64, -1,
     p + ": mlp_acts_stride=-1")

# ------------------------------------------------------------------------------------------------ LN-LSTM backward
for entry, count, p, d_list, bad_d, mult in (
        ("tspgnn_lnlstm_bwd_multi_f32", "lnlstm_bwd_multi", "lnlstm_bwd", "32, 64 or 128", (48,), 16),
        ("tspgnn_lnlstm_bwd_multi_h2", "lnlstm_bwd_multi_h2", "lnlstm_bwd_h2", "32 or 64", (48, 128), 32),
        ("tspgnn_lnlstm_bwd_multi_bf16", "lnlstm_bwd_multi_bf16", "lnlstm_bwd_bf16", "32, 64 or 128", (48,), 32)):
    common(entry, lstm_bwd, count, p + ": d=%d must be " + d_list, bad_d)
    case("rows=-1", entry, [lstm_bwd(rows=-1)], 64, -1, p + ": rows=-1")
    for dx in (mult // 2, -mult):
        for rows in (16, 0):
            case("dx=%d-rows=%d" % (dx, rows), entry, [lstm_bwd(x=F, dx=dx, rows=rows)], 64, -1,
                 "%s: dx=%d must be a non-negative multiple of %d" % (p, dx, mult))
    for field in ("h", "c", "K", "ln", "dz", "dc_in", "ln_grad", "workspace"):
        case("null-" + field, entry, [lstm_bwd(), lstm_bwd(**{field: None})], 64, -1, p + ": null pointer")
    case("null-x", entry, [lstm_bwd(dx=mult)], 64, -1, p + ": null pointer")
    gather = p + ": gather-init mode needs dx == 0" + (", Zx and d in {32,64}" if p == "lnlstm_bwd" else " and Zx")
    case("gather-dx", entry, [lstm_bwd(uv=F, Zx=F, x=F, dx=mult)], 64, -1, gather)
    case("gather-no-Zx", entry, [lstm_bwd(uv=F)], 64, -1, gather)

entry = "tspgnn_lnlstm_bwd_multi_f32"
case("gather-d=128", entry, [lstm_bwd(uv=F, Zx=F)], 128, -1, "lnlstm_bwd: gather-init mode needs dx == 0, Zx and d in {32,64}")
f16x2 = "lnlstm_bwd: a bias-init z / a streamed data gradient are f16x2 features (tspgnn_lnlstm_bwd_multi_h2)"
case("zbias", entry, [lstm_bwd(zbias=F, zscale=F)], 64, -1, f16x2)
case("KTg", entry, [lstm_bwd(x=F, dx=64, KTg=F, dxg=F, dxh=F)], 64, -1, f16x2)

entry = "tspgnn_lnlstm_bwd_multi_h2"
for rows, d in ((BIG, 64), (2 * BIG, 32)):
    case("rows=%d-d=%d" % (rows, d), entry, [lstm_bwd(rows=rows)], d, -1,
         "lnlstm_bwd_h2: rows=%d too large for 32-bit offsets" % rows)
fused = "lnlstm_bwd_h2: the fused data gradient needs dxh and dx == 0"
case("KT-without-dxh", entry, [lstm_bwd(KT=F)], 64, -1, fused)
case("KT-dx", entry, [lstm_bwd(KT=F, dxh=F, x=F, dx=32)], 64, -1, fused)
case("zbias-no-zscale", entry, [lstm_bwd(zbias=F)], 64, -1, "lnlstm_bwd_h2: zbias needs zscale and excludes gather-init mode")
case("zbias-gather", entry, [lstm_bwd(zbias=F, zscale=F, uv=F, Zx=F)], 64, -1,
     "lnlstm_bwd_h2: zbias needs zscale and excludes gather-init mode")
streamed = ("lnlstm_bwd_h2: the streamed data gradient needs d == dx == 64, dxg, dxh and excludes KT / gather-init mode")
case("KTg-d=32", entry, [lstm_bwd(x=F, dx=64, KTg=F, dxg=F, dxh=F)], 32, -1, streamed)
case("KTg-dx=32", entry, [lstm_bwd(x=F, dx=32, KTg=F, dxg=F, dxh=F)], 64, -1, streamed)
case("KTg-without-dxg", entry, [lstm_bwd(x=F, dx=64, KTg=F, dxh=F)], 64, -1, streamed)
case("KTg-without-dxh", entry, [lstm_bwd(x=F, dx=64, KTg=F, dxg=F)], 64, -1, streamed)

entry = "tspgnn_lnlstm_bwd_multi_bf16"
plain = "lnlstm_bwd_bf16: no fused data gradient / bias-init in this mode"
case("KT", entry, [lstm_bwd(KT=F, dxh=F)], 64, -1, plain)
case("dxh", entry, [lstm_bwd(dxh=F)], 64, -1, plain)
case("zbias", entry, [lstm_bwd(zbias=F, zscale=F)], 64, -1, plain)
case("KTg", entry, [lstm_bwd(x=F, dx=64, KTg=F, dxg=F)], 64, -1, plain)

# ------------------------------------------------------------------------------------------------ MLP backward
for entry, count, p, d_list, bad_d in (
        ("tspgnn_mlp_bwd_multi_f32", "mlp_bwd_multi", "mlp_bwd", "32, 64 or 128", (48,)),
        ("tspgnn_mlp_bwd_multi_h2", "mlp_bwd_multi_h2", "mlp_bwd_h2", "64 or 128", (48, 32))):
    common(entry, mlp_bwd, count, p + ": d=%d must be " + d_list, bad_d)
    case("rows=-1", entry, [mlp_bwd(rows=-1)], 64, -1, p + ": rows=-1")
    for L in (0, 5):
        for rows in (16, 0):
            case("n_layers=%d-rows=%d" % (L, rows), entry, [mlp_bwd(n_layers=L, rows=rows)], 64, -1,
                 "%s: n_layers=%d must be in 1..4" % (p, L))
    for L in (3, 4):
        for rows in (16, 0):
            case("d=128-layers=%d-rows=%d" % (L, rows), entry, [mlp_bwd(n_layers=L, rows=rows)], 128, -2,
                 "%s: d=128 holds at most 2 layers in LDS (got %d)" % (p, L))
    case("null-dY", entry, [mlp_bwd(), mlp_bwd(dY=None)], 64, -1, p + ": null pointer")
    case("null-wt", entry, [mlp_bwd(), mlp_bwd(wt=None)], 64, -1, p + ": null pointer")
    case("relu-without-acts", entry, [mlp_bwd(relu_mask=1)], 64, -1, p + ": relu layers need the saved activations")
    case("last-relu-without-Yout", entry, [mlp_bwd(relu_mask=2)], 64, -1, p + ": relu on the last layer needs Yout")
    case("mixed-acts_bf16", entry, [mlp_bwd(), mlp_bwd(acts_bf16=1)], 64, -1, p + ": the tasks of a launch share acts_bf16")

case("pre_X", "tspgnn_mlp_bwd_multi_f32", [mlp_bwd(pre_X=F, pre_wt=F, pre_k=64)], 64, -1,
     "mlp_bwd: pre_X is an f16x2 feature (tspgnn_mlp_bwd_multi_h2)")
entry = "tspgnn_mlp_bwd_multi_h2"
case("rows*d", entry, [mlp_bwd(rows=1 << 25)], 64, -1, "mlp_bwd_h2: rows=%d" % (1 << 25))
pre = "mlp_bwd_h2: pre_X needs d == 64, pre_wt, no uv and pre_k in 32..256 (a multiple of 32), got %d"
case("pre_X-d=128", entry, [mlp_bwd(pre_X=F, pre_wt=F, pre_k=64)], 128, -1, pre % 64)
case("pre_X-without-wt", entry, [mlp_bwd(pre_X=F, pre_k=64)], 64, -1, pre % 64)
case("pre_X-uv", entry, [mlp_bwd(pre_X=F, pre_wt=F, pre_k=64, uv=F)], 64, -1, pre % 64)
for k in (0, 48, 288):
    case("pre_k=%d" % k, entry, [mlp_bwd(pre_X=F, pre_wt=F, pre_k=k)], 64, -1, pre % k)


def _run(entry, tasks, d, n):
    if tasks is None:
        arr, count = None, n
    else:
        arr = ctypes.cast(_lib.task_array(tasks), ctypes.c_void_p)
        count = len(tasks) if n is None else n
    return getattr(_lib.lib, entry)(arr, count, d, None)


@pytest.mark.parametrize("entry,tasks,d,n,status,message", CASES)
def test_multi_entry(entry, tasks, d, n, status, message):
    assert _run(entry, tasks, d, n) == status
    if message is not None:
        assert _lib.lib.tspgnn_last_error().decode() == message


def _head(task, head_w=F, head_b=F, y=F, d=64):
    t = None if task is None else ctypes.cast(ctypes.pointer(task), ctypes.c_void_p)
    return _lib.lib.tspgnn_mlp_head_fwd_h2(t, head_w, head_b, y, d, None)


HEAD = [
    ("null-task", dict(task=None), -1, "null task"),
    ("d=48", dict(task=mlp(), d=48), -1, "d=48 must be 32 or 64"),
    ("d=128", dict(task=mlp(), d=128), -1, "d=128 must be 32 or 64"),
    ("rows=-1", dict(task=mlp(rows=-1)), -1, "rows=-1"),
    ("n_layers=0", dict(task=mlp(n_layers=0)), -1, "n_layers=0 must be in 1..4"),
    ("n_layers=5", dict(task=mlp(n_layers=5)), -1, "n_layers=5 must be in 1..4"),
    ("n_layers=9-empty", dict(task=mlp(n_layers=9, rows=0)), -1, "n_layers=9 must be in 1..4"),
    ("proj_w", dict(task=mlp(proj_w=F, proj_out=F)), -1, "a head task has no projection"),
    ("proj_w-empty", dict(task=mlp(proj_w=F, proj_out=F, rows=0)), -1, "a head task has no projection"),
    ("empty", dict(task=mlp(rows=0), head_w=None, head_b=None, y=None), 0, None),
    ("null-X", dict(task=mlp(X=None)), -1, "null pointer"),
    ("null-wb", dict(task=mlp(wb=None)), -1, "null pointer"),
    ("null-head_w", dict(task=mlp(), head_w=None), -1, "null pointer"),
    ("null-head_b", dict(task=mlp(), head_b=None), -1, "null pointer"),
    ("null-y", dict(task=mlp(), y=None), -1, "null pointer"),
]


@pytest.mark.parametrize("kw,status,message", [pytest.param(*c[1:], id=c[0]) for c in HEAD])
def test_head_entry(kw, status, message):
    assert _head(**kw) == status
    if message is not None:
        assert _lib.lib.tspgnn_last_error().decode() == "mlp_head_fwd_h2: " + message
