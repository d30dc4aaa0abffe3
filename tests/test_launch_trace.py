"""What GraphNN's drivers launch, pinned: every library call of ``GraphNN.__call__``, ``GraphNN.forward_train`` and
``GraphNN.backward`` over a set of wirings, widths, arithmetics and opt-in switches is recorded -- entry point, integer
arguments, which pointers are null, every field of every task structure -- and compared with tests/golden/launch_trace.json.
A selector that changes (folded / pushed / plain cell, the f16x2 packings made up front, the bf16 tasks' flags, which driver a
wiring takes, which data-gradient GEMM rides in which backward launch, the weight gradients' chunking) fails its case here
instead of quietly routing a parity test through another path.

The recorder replaces ``_lib.call``, ``_lib.call_multi`` and ``_lib.current_stream``.  Without a device it records and
returns (tensors live on the CPU, nothing is computed: the drivers' control flow never depends on a value); with a device it
records and forwards, so the same traces are checked against launches that really ran.  Addresses and aliasing are not
recorded: allocation order may change.

The one-launch T-step loop is switched off (``persistent_loop = False``): it needs a work plan that only a device batch
carries, and tests/test_gpu_loop.py pins it against the stepwise launches recorded here.  bf16-storage cases hand over bf16
embeddings, so that the rounding of the inputs (a library call on a device, torch on the CPU) stays out of the trace.

The backward cases record what follows the training forward: ``GraphNN.last_backward`` and the calls of one
``GraphNN.backward`` from zero state gradients (a null dc_out).  The bf16-native pass vets the f16x2 packings of its message
MLPs against the range guard, which only a device can read: its cases run once with ``mlp_backward_h2`` off and once from the
state an eager pass over in-range weights leaves behind (``_mlp_h2_native_ok``), which the initial weights used here make a
device reach by itself -- so one fixture serves both.

``python tests/test_launch_trace.py`` rewrites the fixture from the code as it stands; pytest only ever compares.
"""
import contextlib
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_pack

import tspgnn
from tspgnn import _lib
from tspgnn import variables as V
from tspgnn.instance_loader import SparseEV

FIXTURE = os.path.join(GOLDEN, "launch_trace.json")
STRUCTS = (_lib.MlpTask, _lib.LstmTask, _lib.CellMlpTask, _lib.MlpTaskB, _lib.LstmTaskB, _lib.LstmBwdTask, _lib.MlpBwdTask,
           _lib.MlpBwdRcTask)
BY_POINTER = {"tspgnn_mlp_bwd_rc_h2": _lib.MlpBwdRcTask}    # entry points whose first argument is one task structure
BF16 = torch.bfloat16


def _pointer(p):
    return "p" if p else None


def _fields(s):
    """Every _fields_ member of a task structure, in order: integers as they are, pointers as null / non-null."""
    out = []
    for name, ctype in s._fields_:
        val = getattr(s, name)
        if issubclass(ctype, ctypes.Structure):
            out.append(_fields(val))
        elif issubclass(ctype, ctypes.Array):
            out.append([_pointer(x) for x in val])
        elif ctype is ctypes.c_void_p:
            out.append(_pointer(val))
        else:
            out.append(int(val))
    return out


@contextlib.contextmanager
def recording(forward, env={}):
    """-> the list the library calls made inside the block are appended to.  ``forward``: pass them on to the library.
    ``env``: the TSPGNN_* switches in force inside the block (every other one is cleared)."""
    trace, inside_multi = [], [False]
    real = (_lib.call, _lib.call_multi, _lib.current_stream)

    def call(name, *args):
        if not inside_multi[0]:
            argtypes = _lib.SIGNATURES[name]
            assert len(args) == len(argtypes), name
            trace.append([name] + [_pointer(a) if t is ctypes.c_void_p else a for t, a in zip(argtypes[:-1], args[:-1])])
            if name in BY_POINTER:
                trace[-1][1] = _fields(ctypes.cast(args[0], ctypes.POINTER(BY_POINTER[name])).contents)
        if forward:
            real[0](name, *args)

    def call_multi(name, tasks, d):
        trace.append({"multi": name, "d": int(d), "struct": type(tasks[0]).__name__, "tasks": [_fields(t) for t in tasks]})
        if forward:
            inside_multi[0] = True
            try:
                real[1](name, tasks, d)
            finally:
                inside_multi[0] = False

    def current_stream():
        return real[2]() if forward else None

    saved_env = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("TSPGNN_") and k != "TSPGNN_LIB"}
    os.environ.update(env)
    _lib.call, _lib.call_multi, _lib.current_stream = call, call_multi, current_stream
    try:
        yield trace
    finally:
        _lib.call, _lib.call_multi, _lib.current_stream = real
        for k in env:
            del os.environ[k]
        os.environ.update(saved_env)


# ---------------------------------------------------------------------------------------------------------------- wirings
def _tsp(d, float_dtype=torch.float32, **msg):
    """The network's own wiring (build_network): V <- EV^T msg(E), E <- EV msg(V).  ``msg``: MLP_depth, Msg_last_activation."""
    model = tspgnn.build_network(d, store=V.VariableStore(), float_dtype=float_dtype, **msg)
    return model["gnn"], {"V": "N", "E": "M"}, lambda ev: {"EV": ev}


def _tsp_msg(depth, last):
    """_tsp with message MLPs of ``depth`` hidden layers and the last layer's activation ``last`` (None / "relu")."""
    return lambda d, float_dtype=torch.float32: _tsp(d, float_dtype, MLP_depth=depth, Msg_last_activation=last)


def _two_entries(d, float_dtype=torch.float32):
    """Two loop entries per variable: the adjacency product of the other side's message next to the variable's own h."""
    store = V.VariableStore()
    gnn = tspgnn.GraphNN({"V": d, "E": d}, {"EV": ("E", "V")}, {"V_msg_E": ("V", "E"), "E_msg_V": ("E", "V")},
                         {"V": [{"mat": "EV", "msg": "E_msg_V", "transpose?": True, "var": "E"}, {"var": "V"}],
                          "E": [{"mat": "EV", "msg": "V_msg_E", "var": "V"}, {"var": "E"}]},
                         name="TWO", float_dtype=float_dtype, store=store)
    return gnn, {"V": "N", "E": "M"}, lambda ev: {"EV": ev}


class _Square(object):
    """A loop entry's 'fun' that brings its own vector-Jacobian product along."""

    def __call__(self, x):
        return x * x

    def vjp(self, h, g_out):
        return 2.0 * h * g_out


def _generic(d, float_dtype=torch.float32):
    """A 'fun' ahead of a message MLP, a 'fun' alone, a valued matrix and a dense matrix appended to the cell input (the
    wiring of test_generic_wiring_trains_through_fun_and_appended_matrix_entries)."""
    store = V.VariableStore()
    rng = np.random.RandomState(1)
    A = (rng.randn(9, 7) * (rng.rand(9, 7) < 0.6)).astype(np.float32)
    F = rng.randn(9, 32).astype(np.float32)
    gnn = tspgnn.GraphNN({"U": d, "W": d}, {"M": ("U", "W"), "F": ("U", 32)}, {"c": ("W", "U"), "b": ("U", "W")},
                         {"U": [{"var": "U", "fun": lambda x: 0.5 * torch.tanh(x)}, {"mat": "M", "msg": "c", "var": "W"},
                                {"mat": "F"}],
                          "W": [{"mat": "M", "transpose?": True, "msg": "b", "var": "U", "fun": _Square()}]},
                         name="G", float_dtype=float_dtype, store=store)
    return gnn, {"U": 9, "W": 7}, lambda ev: {"M": A, "F": F}


# message MLPs off the default (three hidden layers, a linear last one): the depth decides whether the vertex cell is pushed,
# the layers and relu masks of every message task, the tape's acts and how many kernels a chain takes (two layers each at 128)
MSG_DEPTH = {
    "tsp-d64-f16x2-depth0": (_tsp_msg(0, None), 64, torch.float32, dict(gemm="f16x2"), "h2"),
    "tsp-d64-f16x2-depth1": (_tsp_msg(1, None), 64, torch.float32, dict(gemm="f16x2"), "h2"),
    "tsp-d64-f16x2-depth2-relu": (_tsp_msg(2, "relu"), 64, torch.float32, dict(gemm="f16x2"), "h2"),
    "tsp-d64-f16x2-depth3-relu": (_tsp_msg(3, "relu"), 64, torch.float32, dict(gemm="f16x2"), "h2"),
    "tsp-d128-depth1": (_tsp_msg(1, None), 128, torch.float32, dict(gemm="f16x2"), "h2"),
    "tsp-d128-depth2": (_tsp_msg(2, None), 128, torch.float32, dict(gemm="f16x2"), "h2"),
    "tsp-d64-bf16-depth1-relu": (_tsp_msg(1, "relu"), 64, BF16, dict(gemm="f16x2"), "h2"),
}
# case -> (wiring, d, storage type, attributes set on the GraphNN, active_arith() expected)
FORWARD = {
    "tsp-d64-f16x2": (_tsp, 64, torch.float32, dict(gemm="f16x2"), "h2"),
    "tsp-d64-bf16x3": (_tsp, 64, torch.float32, dict(gemm="bf16x3"), "x3"),
    "tsp-d64-f32": (_tsp, 64, torch.float32, dict(gemm="f32"), None),
    "tsp-d128": (_tsp, 128, torch.float32, dict(gemm="f16x2"), "h2"),     # (no split kernels at 128: _plan, fp32 MFMA)
    "tsp-d32": (_tsp, 32, torch.float32, dict(gemm="f16x2"), "h2"),
    "tsp-d64-unfolded": (_tsp, 64, torch.float32, dict(gemm="f16x2", fold_adjacency=False), "h2"),
    "tsp-d64-bf16": (_tsp, 64, BF16, dict(gemm="f16x2"), "h2"),
    "tsp-d128-bf16": (_tsp, 128, BF16, dict(gemm="f16x2"), "h2"),
    "two-entries-d64": (_two_entries, 64, torch.float32, dict(gemm="f16x2"), "h2"),
    "two-entries-d64-f32": (_two_entries, 64, torch.float32, dict(gemm="f32"), None),
    "two-entries-d64-bf16": (_two_entries, 64, BF16, dict(gemm="f16x2"), "h2"),
    "generic-d32": (_generic, 32, torch.float32, dict(gemm="f16x2"), "h2"),
}
FORWARD.update(MSG_DEPTH)
TRAIN = {
    "tsp-d64-f16x2-pushed": (_tsp, 64, torch.float32, dict(gemm="f16x2"), "h2"),
    "tsp-d64-f16x2-unpushed": (_tsp, 64, torch.float32, dict(gemm="f16x2", push_training=False), "h2"),
    "tsp-d64-f16x2-fused": (_tsp, 64, torch.float32, dict(gemm="f16x2", fuse_training_messages=True), "h2"),
    "tsp-d64-f16x2-recompute": (_tsp, 64, torch.float32, dict(gemm="f16x2", recompute_messages=True), "h2"),
    "tsp-d64-bf16x3": (_tsp, 64, torch.float32, dict(gemm="bf16x3"), "x3"),
    "tsp-d64-f32": (_tsp, 64, torch.float32, dict(gemm="f32"), None),
    "tsp-d64-bf16": (_tsp, 64, BF16, dict(gemm="f16x2"), "h2"),
    "tsp-d32-bf16": (_tsp, 32, BF16, dict(gemm="f16x2"), "h2"),
    "two-entries-d64": (_two_entries, 64, torch.float32, dict(gemm="f16x2"), "h2"),
    "two-entries-d64-bf16": (_two_entries, 64, BF16, dict(gemm="f16x2"), "h2"),
    "generic-d32-f16x2": (_generic, 32, torch.float32, dict(gemm="f16x2"), "h2"),
    "generic-d32-f32": (_generic, 32, torch.float32, dict(gemm="f32"), None),
}
TRAIN.update(MSG_DEPTH)
SWITCHES = dict(fold_adjacency=True, center_gates=True, persistent_loop=False, push_training=True,
                fuse_training_messages=False, mlp_backward_h2=True, recompute_messages=False)


def _network(table, case, device, attrs={}):
    """Inside recording(): -> (the case's GraphNN with its variables initialised, matrices, embeddings, rows per variable)."""
    wiring, d, dtype, own, arith = table[case]
    pack = load_pack("n5_B2")
    ev = SparseEV(pack["ev_uv"], int(pack["ev_shape"][1]))
    gnn, rows, matrices = wiring(d, dtype)
    for k, val in dict(SWITCHES, **dict(own, **attrs)).items():
        setattr(gnn, k, val)
    gnn.store.finalize(device)
    gnn.store.initialize(seed=3)
    rng = np.random.RandomState(5)
    sizes = {"M": ev.shape[0], "N": ev.shape[1]}
    emb = {v: torch.from_numpy(rng.randn(sizes.get(r, r), d).astype(np.float32)).to(dtype).to(device)
           for v, r in rows.items()}
    assert gnn.active_arith() == arith
    return gnn, matrices(ev), emb, rows


def run_case(case, T, train):
    """-> what the fixture holds for the case: the selectors in force and the trace."""
    arith = (TRAIN if train else FORWARD)[case][4]
    device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    with recording(forward=device.type == "cuda") as trace:
        gnn, mats, emb, rows = _network(TRAIN if train else FORWARD, case, device)
        got = {}
        if train:
            states, tape = gnn.forward_train(mats, emb, T)
            got["pushed"] = {v: bool(p) for v, p in tape.pushed.items()}
            got["folded"] = {v: u is not None for v, u in tape.folded.items()}
            got["fused"] = bool(tape.fused)
            got["tape_arith"] = tape.arith
        else:
            states = gnn(mats, emb, T)
        assert gnn.active_arith() == arith and gnn.launched_loop is None
        if device.type == "cuda":
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(st.h.float()).all()) for st in states.values())
        assert sorted(states) == sorted(rows) and all(tuple(states[v].h.shape) == tuple(emb[v].shape) for v in rows)
    got["trace"] = trace
    return got


def run_backward_case(case, T, attrs={}, env={}, chunks=None, h2_ok=False):
    """-> GraphNN.last_backward and the calls after the training forward of a TRAIN wiring, or the exception of a wiring
    whose backward cannot run.  ``chunks``: the weight gradients' budget -- "one": a step per chunk; "partial": the first
    power of two that fits more than one step.  ``h2_ok``: as after an eager pass that found the message MLPs' weights
    inside the f16x2 range (the bf16-native pass)."""
    device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    with recording(forward=device.type == "cuda", env=env) as trace:
        gnn, mats, emb, rows = _network(TRAIN, case, device, attrs)
        gnn._mlp_h2_native_ok = h2_ok
        states, tape = gnn.forward_train(mats, emb, T)
        dstates = {v: (torch.zeros(st.h.shape, dtype=torch.float32, device=device), None) for v, st in states.items()}
        mark = len(trace)
        budgets = {None: [gnn.wgrad_chunk_bytes], "one": [1], "partial": [1 << k for k in range(48)]}[chunks]
        try:
            for budget in budgets:
                gnn.wgrad_chunk_bytes = budget
                del trace[mark:]
                gnn.store.zero_grad()
                d0 = gnn.backward(tape, dstates)
                if chunks != "partial" or gnn.last_backward["chunk_steps"] > 1:
                    break
        except NotImplementedError as e:
            assert not trace[mark:], "the plan refuses a wiring before the pass launches anything"
            return {"raises": [type(e).__name__, str(e)]}
        steps = gnn.last_backward["chunk_steps"]
        if chunks == "partial":
            assert 1 < steps < T and T % steps != 0, (steps, T)       # the last chunk is a partial one
        if chunks == "one":
            assert steps == 1 and gnn.last_backward["chunks"] == T
        if device.type == "cuda":
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(g).all()) for v in rows for g in d0[v]) and bool(torch.isfinite(gnn.store.grad).all())
        assert sorted(d0) == sorted(rows) and all(tuple(d0[v][0].shape) == tuple(emb[v].shape) for v in rows)
    return {"last_backward": gnn.last_backward, "trace": trace[mark:]}


FORWARD_IDS = [("%s/T%d" % (case, T), case, T) for case in FORWARD for T in (0, 1, 3)]
TRAIN_IDS = [("train/%s/T3" % case, case, 3) for case in TRAIN]
NATIVE = ("tsp-d64-bf16", "two-entries-d64-bf16")       # the wirings whose bf16 tape the backward reads as it is
PUSHED, UNPUSHED = "tsp-d64-f16x2-pushed", "tsp-d64-f16x2-unpushed"
# (key, wiring, T, run_backward_case's keywords)
BACKWARD_IDS = [("backward/%s/T3" % case, case, 3, dict(h2_ok=case in NATIVE + ("tsp-d64-bf16-depth1-relu",))) for case in TRAIN]
BACKWARD_IDS += [("backward/%s/T3/mlp-f32" % case, case, 3, dict(attrs=dict(mlp_backward_h2=False))) for case in NATIVE]
BACKWARD_IDS += [("backward/%s/T3/chunk-1" % PUSHED, PUSHED, 3, dict(chunks="one")),
                 ("backward/%s/T5/chunk-partial" % PUSHED, PUSHED, 5, dict(chunks="partial")),
                 ("backward/tsp-d64-bf16/T5/chunk-partial", "tsp-d64-bf16", 5, dict(chunks="partial", h2_ok=True))]
BACKWARD_IDS += [("backward/%s/T3/data-gradients-apart" % case, case, 3, dict(env={"TSPGNN_FUSE_DATA_GRADIENTS": "0"}))
                 for case in (PUSHED, UNPUSHED)]
BACKWARD_IDS += [("backward/tsp-d64-bf16/T3/widened", "tsp-d64-bf16", 3, dict(env={"TSPGNN_BF16_BACKWARD": "widened"}))]


def _expected():
    with open(FIXTURE) as f:
        return json.load(f)


def _check(key, got):
    want = _expected()
    assert want["fields"] == {s.__name__: [name for name, _ in s._fields_] for s in STRUCTS}
    assert key in want["cases"], "no recorded trace for %s" % key
    exp = want["cases"][key]
    got = json.loads(json.dumps(got))
    for k in exp:
        if k != "trace":
            assert got[k] == exp[k], (key, k)
    got_trace, exp_trace = got.get("trace", []), exp.get("trace", [])       # (a case that raises has none)
    for n, (g, e) in enumerate(zip(got_trace, exp_trace)):
        assert g == e, "%s: call %d differs\n got      %s\n expected %s" % (key, n, json.dumps(g), json.dumps(e))
    assert len(got_trace) == len(exp_trace), "%s: %d calls, expected %d" % (key, len(got_trace), len(exp_trace))
    assert sorted(got) == sorted(exp)


@pytest.mark.parametrize("key,case,T", FORWARD_IDS, ids=[k for k, _, _ in FORWARD_IDS])
def test_forward_launches(key, case, T):
    _check(key, run_case(case, T, train=False))


@pytest.mark.parametrize("key,case,T", TRAIN_IDS, ids=[k for k, _, _ in TRAIN_IDS])
def test_training_forward_launches(key, case, T):
    _check(key, run_case(case, T, train=True))


@pytest.mark.parametrize("key,case,T,how", BACKWARD_IDS, ids=[k for k, _, _, _ in BACKWARD_IDS])
def test_backward_launches(key, case, T, how):
    _check(key, run_backward_case(case, T, **how))


def test_a_relu_on_a_chain_s_last_layer_comes_with_its_output():
    """Every message-MLP backward task of every recorded backward pass: a relu on the task's last layer (bit n_layers - 1
    of relu_mask) is masked by the chain's forward output, so Yout is not null -- the library refuses the task otherwise
    (csrc/launch_plan.h, check_mlp_bwd_task; tspgnn_mlp_bwd_rc_h2 likewise)."""
    fields = {s.__name__: [name for name, _ in s._fields_] for s in (_lib.MlpBwdTask, _lib.MlpBwdRcTask)}
    seen = ended_in_relu = 0
    for key, case, T, how in BACKWARD_IDS:
        for call in run_backward_case(case, T, **how).get("trace", []):
            if isinstance(call, dict) and call["struct"] in fields:
                tasks = [dict(zip(fields[call["struct"]], t)) for t in call["tasks"]]
            elif isinstance(call, list) and call[0] in BY_POINTER:
                tasks = [dict(zip(fields[BY_POINTER[call[0]].__name__], call[1]))]
            else:
                continue
            for t in tasks:
                seen += 1
                if (t["relu_mask"] >> (t["n_layers"] - 1)) & 1:
                    ended_in_relu += 1
                    assert t["Yout"] is not None, (key, t)
    assert seen > 0 and ended_in_relu > 0       # (the pushed prefixes and the chains of Msg_last_activation="relu")


def test_fixture_holds_exactly_these_cases():
    assert sorted(_expected()["cases"]) == sorted([k for k, _, _ in FORWARD_IDS + TRAIN_IDS] + [k for k, _, _, _ in BACKWARD_IDS])


def _write():
    """One call per line: readable, and a changed launch shows as a one-line diff."""
    lines = ["{", '"fields": {']
    lines.append(",\n".join('  %s: %s' % (json.dumps(s.__name__), json.dumps([n for n, _ in s._fields_])) for s in STRUCTS))
    lines.append("},")
    lines.append('"cases": {')
    blocks = []
    runs = [(key, lambda case=case, T=T, key=key: run_case(case, T, train=key.startswith("train/")))
            for key, case, T in FORWARD_IDS + TRAIN_IDS]
    runs += [(key, lambda case=case, T=T, how=how: run_backward_case(case, T, **how)) for key, case, T, how in BACKWARD_IDS]
    for key, run in runs:
        got = run()
        head = ["  %s: %s" % (json.dumps(k), json.dumps(got[k], sort_keys=True)) for k in sorted(got) if k != "trace"]
        if "trace" in got:
            calls = ",\n".join("    " + json.dumps(c) for c in got["trace"])
            head.append('  "trace": [\n%s\n  ]' % calls if calls else '  "trace": []')
        blocks.append("%s: {\n%s\n}" % (json.dumps(key), ",\n".join(head)))
    lines.append(",\n".join(blocks))
    lines.append("}")
    lines.append("}")
    with open(FIXTURE, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    _write()
