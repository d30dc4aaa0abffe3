"""The route head without a GPU: route_edge_marks_host on hand cases against a brute-force set-membership loop, the variable
layout of build_network(route_head=...), Session.prepare's refusals on a plumbing session, load_weights(missing_ok=True),
and the float64 reference's own consistency (tests/route_head_reference.py)."""
import numpy as np
import pytest
import torch

import tspgnn
from tspgnn import InstanceLoader, route_edge_marks_host
from tspgnn import route_head as RH

import route_head_reference as REF


def brute_force(instances):
    """marks and n_missing by set membership: the tour's unordered pairs, the closing pair (last, first) among them."""
    marks, missing = [], []
    for Ma, _, route in instances:
        route = [int(v) for v in route]
        pairs = {frozenset((a, b)) for a, b in zip(route, route[1:] + route[:1])}
        edges = [(int(i), int(j)) for i, j in zip(*np.nonzero(np.asarray(Ma)))]
        marks += [1.0 if frozenset(e) in pairs else 0.0 for e in edges]
        missing.append(sum(1 for pr in pairs if pr not in {frozenset(e) for e in edges}))
    return np.asarray(marks, dtype=np.float32), np.asarray(missing, dtype=np.int64)


def complete(n, rng):
    Ma = np.triu(np.ones((n, n), dtype=np.int64), 1)
    Mw = rng.rand(n, n)
    return Ma, Mw + Mw.T


def sparse_n12():
    """n = 12 on a ring plus chords; the tour follows the ring except that it visits 4 and 5 in swapped order, which uses
    the chords (3, 5) and (4, 6) and the ring edge (4, 5); two ring edges it then needs, (0, 11) and (8, 9), are removed:
    the tour has two pairs that are no edge."""
    n = 12
    rng = np.random.RandomState(12)
    Ma = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        a, b = sorted((i, (i + 1) % n))
        Ma[a, b] = 1
    for a, b in ((3, 5), (4, 6), (0, 6), (2, 9), (1, 7)):
        Ma[a, b] = 1
    Ma[0, 11] = 0
    Ma[8, 9] = 0
    Mw = rng.rand(n, n)
    return (Ma, Mw + Mw.T, [0, 1, 2, 3, 5, 4, 6, 7, 8, 9, 10, 11])


def hand_cases():
    rng = np.random.RandomState(5)
    n4 = complete(4, rng) + ([2, 0, 3, 1],)
    n3 = complete(3, rng) + ([1, 2, 0],)
    # closing pair: (last, first) = (4, 0) is an edge and must be marked; (last, second) = (4, 2), the pair the reference's
    # cost sum closes with, is an edge too and must not be
    n5 = complete(5, rng) + ([0, 2, 1, 3, 4],)
    return [n4, n3, sparse_n12(), n5]


def test_marks_on_hand_cases_equal_brute_force():
    cases = hand_cases()
    marks, missing = route_edge_marks_host(cases)
    ref_marks, ref_missing = brute_force(cases)
    assert marks.dtype == np.float32 and np.array_equal(marks, ref_marks)
    assert np.array_equal(missing, ref_missing)
    # edge order is create_batch's
    EV = InstanceLoader.create_batch(cases)[0]
    assert marks.shape[0] == EV.uv.shape[0]
    seg = np.concatenate([[0], np.cumsum([int(np.count_nonzero(c[0])) for c in cases])])
    per = [marks[seg[k]:seg[k + 1]] for k in range(len(cases))]
    assert per[0].sum() == 4 and missing[0] == 0                   # n = 4, complete: the 4 tour edges of 6
    assert per[1].sum() == 3 and per[1].size == 3 and missing[1] == 0   # n = 3: every pair, each once
    assert missing[2] == 2 and per[2].sum() == 12 - 2              # sparse n = 12: two tour pairs are no edge
    Ma5, _, route5 = cases[3]
    edges5 = list(zip(*np.nonzero(Ma5)))
    assert per[3][edges5.index((0, 4))] == 1.0                     # (last, first)
    assert per[3][edges5.index((2, 4))] == 0.0                     # (last, second)
    assert per[3].sum() == 5


def test_marks_refuse_what_is_no_tour():
    rng = np.random.RandomState(1)
    good = complete(5, rng) + ([0, 1, 2, 3, 4],)
    for bad_route in ([0, 1, 2, 3, 3], [0, 1, 2, 3], [0, 1, 2, 3, 5]):
        with pytest.raises(ValueError, match="instance 1"):
            route_edge_marks_host([good, good[:2] + (bad_route,)])


def names_and_offsets(store):
    store.finalize("cpu")
    return store.names(), [store.offset(n) for n in store.names()]


def test_layout_without_the_head_is_unchanged_and_a_prefix_with_it():
    plain = names_and_offsets(tspgnn.build_network(32, store=tspgnn.VariableStore()).store)
    off = names_and_offsets(tspgnn.build_network(32, store=tspgnn.VariableStore(), route_head=False).store)
    model = tspgnn.build_network(32, store=tspgnn.VariableStore(), route_head=True)
    on = names_and_offsets(model.store)
    from oracle import params as P
    assert plain[0] == P.param_names(32)            # today's variables, in today's order
    assert plain == off
    k = len(plain[0])
    assert on[0][:k] == plain[0] and on[1][:k] == plain[1]
    extra = on[0][k:]
    assert extra == ["E_route_MLP_layer_%d/%s" % (i, w) for i in (1, 2, 3, 4) for w in ("kernel", "bias")]
    assert [model.store.shape(n) for n in extra] == [(32, 32), (32,), (32, 32), (32,), (32, 32), (32,), (32, 1), (1,)]
    assert "route_edges" not in tspgnn.build_network(32, store=tspgnn.VariableStore()) and "route_edges" in model
    for key in ("E_route", "route_loss", "route_acc", "route_TP", "route_FP", "route_TN", "route_FN"):
        assert key in model
    with pytest.raises(ValueError):
        tspgnn.build_network(32, store=tspgnn.VariableStore(), route_head=True, route_pos_weight=0.0)


def plumbing(route_head=True):
    rng = np.random.RandomState(3)
    instances = [tspgnn.random_instance(n, rng) for n in (5, 6)]
    model = tspgnn.build_network(32, store=tspgnn.VariableStore(), route_head=route_head)
    sess = tspgnn.Session(model, device="cpu")
    t = InstanceLoader.create_batch(instances)
    feed = {model[k]: v for k, v in zip(("EV", "W", "C", "route_exists", "n_vertices", "n_edges"), t)}
    feed[model["time_steps"]] = 2
    return instances, model, sess, feed


def with_marks(feed, model, marks):
    out = dict(feed)
    out[model["route_edges"]] = marks
    return out


def test_prepare_takes_the_marks_and_refuses_bad_ones():
    instances, model, sess, feed = plumbing()
    marks = route_edge_marks_host(instances)[0]
    b = sess.prepare(with_marks(feed, model, marks))
    assert b.route_edges.dtype == torch.float32 and np.array_equal(b.route_edges.numpy(), marks)
    assert any(t is b.route_edges for t in b.tensors())
    other = sess.prepare(with_marks(feed, model, 1 - marks))
    b.copy_from(other)
    assert np.array_equal(b.route_edges.numpy(), 1 - marks)
    with pytest.raises(ValueError, match="route_edges.*one mark per edge"):
        sess.prepare(with_marks(feed, model, marks[:-1]))
    half = marks.copy()
    half[0] = 0.5
    with pytest.raises(ValueError, match="route_edges.*0 or 1"):
        sess.prepare(with_marks(feed, model, half))
    # without marks: the batch is prepared (inference needs none), training and the route statistics are refused
    plain = sess.prepare(feed)
    assert getattr(plain, "route_edges", None) is None
    for refused in (lambda: sess.train_step(feed), lambda: sess.train_step(plain), lambda: sess.loss_and_grads(feed),
                    lambda: sess.train_step_accumulated([plain]), lambda: sess.run(model["train_step"], feed_dict=feed),
                    lambda: sess.run(model["route_loss"], feed_dict=feed)):
        with pytest.raises(ValueError, match="route_edges"):
            refused()
    with pytest.raises(ValueError, match="differ in shape"):   # a batch with marks does not take one without
        b.copy_from(plain)


def test_a_network_without_the_head_ignores_nothing_and_needs_nothing():
    instances, model, sess, feed = plumbing(route_head=False)
    assert not model.route_head and "route_edges" not in model
    b = sess.prepare(feed)
    assert getattr(b, "route_edges", None) is None
    with pytest.raises(RuntimeError, match="plumbing only"):    # (the refusal it always gave on a CPU session)
        sess.train_step(feed)


def test_load_weights_missing_ok_starts_a_route_head_run_from_a_decision_only_checkpoint(tmp_path, capsys):
    _, model0, sess0, _ = plumbing(route_head=False)
    sess0.run(tspgnn.global_variables_initializer(seed=4))
    path = str(tmp_path / "epoch=7")
    tspgnn.save_weights(sess0, path)
    _, model1, sess1, _ = plumbing(route_head=True)
    sess1.run(tspgnn.global_variables_initializer(seed=11))
    before = model1.store.state_dict()
    with pytest.raises(KeyError, match="E_route"):
        tspgnn.load_weights(sess1, path)
    capsys.readouterr()
    assert tspgnn.load_weights(sess1, path, missing_ok=True) == 7
    printed = capsys.readouterr().out
    after, saved = model1.store.state_dict(), model0.store.state_dict()
    for name in after:
        if name.startswith("E_route"):
            assert name in printed and np.array_equal(after[name], before[name])
        else:
            assert np.array_equal(after[name], saved[name])
    assert sess1._adam is None      # (the checkpoint holds no complete set of Adam slots)


def test_device_dataset_keeps_checked_routes_on_a_plumbing_device():
    rng = np.random.RandomState(2)
    instances = [tspgnn.random_instance(n, rng) for n in (5, 7, 6)]
    ds = tspgnn.DeviceDataset(instances, device="cpu", routes=True)
    assert np.array_equal(ds._routes.numpy(), np.concatenate([r for _, _, r in instances]).astype(np.int32))
    assert np.array_equal(ds._route_v0, [0, 5, 12])
    assert tspgnn.DeviceDataset(instances, device="cpu")._routes is None
    bad = instances[:1] + [(instances[1][0], instances[1][1], [0] * 7)]
    with pytest.raises(ValueError, match="instance 1"):
        tspgnn.DeviceDataset(bad, device="cpu", routes=True)


def test_reference_gradient_matches_its_own_finite_difference():
    """route_head_reference: d route_loss / d logits by autograd equals the closed form edge_bce returns, and the weights
    follow the balanced rule."""
    rng = np.random.RandomState(8)
    n_edges = [1, 6, 10]
    x = rng.uniform(-4, 4, size=17)
    y = (rng.rand(17) < 0.3).astype(np.float64)
    y[1:7] = 0                                   # a problem without a marked edge: weights 1, k = 0
    for pw in (None, 3.0):
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        loss = REF.route_loss_torch(xt, y, n_edges, pw)
        (g,) = torch.autograd.grad(loss, xt)
        stats, dlogit = REF.edge_bce(x, y, n_edges, pw, scale=1.0)
        assert abs(stats[0] - loss.item()) < 1e-12
        assert np.abs(dlogit - g.numpy()).max() < 1e-12
        assert stats[2:].sum() == 17
    w = REF.edge_weights(y, n_edges, None)
    k = y[7:].sum()
    assert np.all(w[:7] == 1.0) and np.allclose(w[7:][y[7:] != 0], (10 - k) / max(k, 1))
    assert RH.MIN_N == 3 and RH.MAX_N == 16384


@pytest.mark.parametrize("d", [32, 64])
def test_a_network_without_the_head_makes_the_launches_it_made_before(d, monkeypatch):
    """The recorder of tests/test_launch_trace.py without a device (nothing is computed, the control flow never depends on
    a value): forward_device and loss_and_grads of route_head=False name exactly the calls recorded before the head existed,
    and route_head=True adds its own between them without moving one."""
    import json
    import os
    from conftest import GOLDEN
    from test_launch_trace import recording
    want = json.load(open(os.path.join(GOLDEN, "route_head_launch_names.json")))
    got = {}
    for head in (False, True):
        model, sess, b, _ = REF.launch_case(d, "cpu", route_head=head)
        monkeypatch.setattr(sess, "_require_gpu", lambda what: None)
        with recording(False) as trace:
            sess.forward_device(b)
        got[head, "forward"] = REF.launch_names(trace)
        with recording(False) as trace:
            sess.loss_and_grads(b)
        got[head, "loss_and_grads"] = REF.launch_names(trace)
    for what in ("forward", "loss_and_grads"):
        assert got[False, what] == want["%s_d%d" % (what, d)], what
        it = iter(got[True, what])
        assert all(name in it for name in got[False, what]), what     # the old calls, in order, inside the new sequence
        assert "tspgnn_edge_bce_f32" in got[True, what] and "tspgnn_edge_bce_f32" not in got[False, what]
