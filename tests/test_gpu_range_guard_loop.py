"""The f16x2 range guard through the whole model, on all three drivers of the T-step loop: the stepwise launches
(persistent_loop = False), tspgnn_mp_loop_h2 (TSPGNN_LOOP_KIND=loop) and tspgnn_mp_resident_h2 (TSPGNN_LOOP_KIND=resident).
The one-launch kernels are bit-identical to the stepwise launches (tests/test_gpu_loop.py), so the guard word an UNGUARDED
forward leaves -- Session.forward_device, nothing looks at the flag in between -- must be the same bits on all three; before
this file nothing asked the two loop kernels to raise it at all.  The word is read twice per driver: after GraphNN.__call__
alone (message_passing_alone: no vote head, whose first layer splits the last E.h once more) and after the whole forward.

The cases are range_guard_cases.model_cases(); tests/test_range_guard_cases_host.py has judged each in float64: the named
operand beyond 7.0e4 with every other split operand within 6.0e4, the named gate with a row of positive variance below a
quarter of the floor with every other above four floors.
  bias cases: one bias entry of a message MLP's layer; the overflow exists at every evaluation of that layer, the plain MLP
    launch of step 0's messages included (that launch raises the word whatever the loop's launches do);
  "behind new h" cases: the same column is beyond the range only when the MLP reads a cell's OUTPUT (h'[:, j] = 3.0e4 carried
    down column j), so the word can only come from the fused cell launches or from the loop kernels' own MLP layers and
    projection -- mp_loop_h2 / mp_resident_h2's dense_layer_h2 and projection witnesses;
  h' cases: a cell's new h (the edge kernels' kept pieces of h, the vertex operand h, the next MLP's first layer, the head);
  aggregate cases: the vertex operand, the row-sum of up to 39 messages of ~3000, with the 40-vertex graph first, last and
    between two 20s; two 20-vertex graphs stay quiet;
  gate cases: each gate of each cell alone below the variance floor -- lstm_stage_f / _ij / _o of mp_loop_h2, lstm_gates of
    mp_resident_h2 and of the stepwise launch, all through the CENTERED LayerNorm the model runs -- bit 1 and only bit 1.
After every raising case Session.run on the same session answers on bf16x3: finite, within 1e-5 of float64, and f16x2 is
the arithmetic in force again for the next batch."""
import math

import numpy as np
import pytest
import torch

import range_guard_cases as RG
import tspgnn
from conftest import batch_from_tuple, rel_err
from oracle import torch_oracle as TO
from tspgnn import _lib

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5
DRIVERS = [None, "loop", "resident"]      # None: the stepwise launches
CASES = RG.model_cases()


def unguarded_word(case, kind, monkeypatch):
    """-> (guard word after one unguarded forward on driver `kind`, the session, the model, the feed)."""
    monkeypatch.setenv("TSPGNN_LOOP_MAX_TILES", "4")
    if kind is None:
        monkeypatch.delenv("TSPGNN_LOOP_KIND", raising=False)
    else:
        monkeypatch.setenv("TSPGNN_LOOP_KIND", kind)
    model = tspgnn.build_network(64)
    model["gnn"].persistent_loop = kind is not None
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer())
    model.store.load(case.params)
    EV, W, C, route_exists, n_vertices, n_edges = tspgnn.synthetic_batch(case.sizes, seed=3)
    feed = {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: case.T,
            model["route_exists"]: route_exists, model["n_vertices"]: n_vertices, model["n_edges"]: n_edges}
    b = sess.prepare(feed)
    assert model["gnn"].active_arith() == "h2"
    if kind is not None:
        assert b.adj.loop_plan is not None and b.adj.loop_plan[3] == kind, "no %s plan for this batch" % kind
    words = []
    for whole in (False, True):
        assert int(sess.store.h2_guard()[0].item()) == 0 and int(sess.store.h2_guard()[2].item()) == 0
        if whole:
            sess.forward_device(b)
        else:
            message_passing_alone(sess, b)
        torch.cuda.synchronize()
        assert model["gnn"].active_arith() == "h2", "the weights' packing vetoed f16x2: not the event this case is about"
        assert model["gnn"]._launched_loop == kind, "ran on %r, not on %r" % (model["gnn"]._launched_loop, kind)
        assert int(sess.store.h2_guard()[2].item()) == 0
        words.append(int(sess.store.h2_guard()[0].item()))
        assert sess.range_exceeded() == bool(words[-1])          # (clears the word)
    assert words[0] == words[1], "message passing alone left %d, the whole forward %d" % tuple(words)
    return words[0], sess, model, feed


def message_passing_alone(sess, b):
    """Session.forward_device up to and including GraphNN.__call__, without the vote head behind it: the head's first layer
    splits the last E.h again and would raise bit 0 for an h' the loop's own launches had missed."""
    m, d = sess.model, sess.model.d
    E0 = m.edge_init_MLP(b.WC)
    V0 = torch.empty((b.N, d), dtype=torch.float32, device=sess.device)
    _lib.call("tspgnn_tile_rows_f32", _lib.ptr(sess.store.view("V_init")), 1.0 / math.sqrt(float(d)), _lib.ptr(V0), b.N, d,
              _lib.current_stream())
    return m["gnn"]({"EV": b.adj}, {"V": V0, "E": E0}, b.T)


@pytest.mark.parametrize("case", CASES, ids=[c.label.replace(" ", "_") for c in CASES])
def test_guard_word_on_every_driver(cuda_device, monkeypatch, case):
    ref = None
    words = {}
    for kind in DRIVERS:
        word, sess, model, feed = unguarded_word(case, kind, monkeypatch)
        words[kind] = word
        if case.word == 0:
            continue
        # the guarded path on the same session: this batch on bf16x3, the next one on f16x2 again
        pred, last = sess.run([model["predictions"], model["last_states"]], feed_dict=feed)
        if ref is None:
            ref = TO.forward(TO.to_torch(case.params, torch.float64),
                             batch_from_tuple(tspgnn.synthetic_batch(case.sizes, seed=3)), case.T)
        got = {"pred": (pred, ref["predictions"]), "E.h": (last["E"].h, ref["last_states"]["E"][0]),
               "E.c": (last["E"].c, ref["last_states"]["E"][1]), "V.h": (last["V"].h, ref["last_states"]["V"][0]),
               "V.c": (last["V"].c, ref["last_states"]["V"][1])}
        errs = {}
        for n, (a, r) in got.items():
            assert np.all(np.isfinite(np.asarray(a))), (kind, n)
            errs[n] = rel_err(a, r.numpy())
        print(" GUARD model %s on %s: word %d, then bf16x3 %s" % (case.label, kind or "stepwise", word,
                                                                  " ".join("%s %.1e" % kv for kv in errs.items())))
        assert all(e < REL_TOL for e in errs.values()), (kind, errs)
        assert sess.last_range_bits == case.word
        assert model["gnn"].active_arith() == "h2" and not sess.range_exceeded()
    print(" GUARD model %s: words %s (design %d)" % (case.label, words, case.word))
    assert words == {kind: case.word for kind in DRIVERS}, (case.label, words, case.word)
