"""tspgnn_vote_scores_i32 and tspgnn_tour_beam on the GPU (csrc/tour_beam.hip, tspgnn.decode) against the NumPy
restatement of tests/beam_reference.py.  The beam tests feed integer scores straight to the kernel, so everything is
compared exactly: tours, n_missing, scores and n_closed as integers, costs bit for bit.  The sizes are those at which the
kernel changes shape -- fewer candidates than `beam`, the wave boundary of the lists, one / two / four mask words and
256 / 512 / 1 024 threads -- and the inputs those on which ties, the clamp, stranded paths and empty instances decide.
Then the Python surface end to end on tests/golden/trained_d64.npz.  Nothing here claims that beam tours are good."""
import functools
import os

import numpy as np
import pytest
import torch

import beam_cases as bc
import beam_reference as ref
import decode_cases as cases
import tspgnn
from conftest import GOLDEN
from tspgnn import _lib, decode

pytestmark = pytest.mark.gpu

SENTINEL = -77
SELECTS = ("score", "cost")


def launch(case, scores, beam, select, n_max=None, fill=None, extra=0, short=0, dev="cuda:0"):
    """The raw entry point on a decode_cases batch and its integer scores -> (status, tours, costs as uint32 bits,
    n_missing, scores, n_closed), outputs prefilled with SENTINEL.  fill: the byte the workspace is prefilled with; extra /
    short: bytes added to / withheld from what the query asks for."""
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dev) for k in ("uv", "wc", "seg", "vseg")}
    s = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.int32)).to(dev)
    if case["vote"].size == 0:
        s, t["uv"], t["wc"] = (torch.zeros(sh, dtype=d, device=dev) for sh, d in
                               (((1,), torch.int32), ((1, 2), torch.int32), ((1, 2), torch.float32)))
    B, N = len(case["n"]), int(case["vseg"][-1])
    n_max = int(case["n"].max()) if n_max is None else n_max
    need = int(_lib.lib.tspgnn_tour_beam_workspace_bytes(B, min(max(n_max, 4), 256), min(max(beam, 1), 1024)))
    ws = torch.full((max(need + extra, 16),), 0 if fill is None else fill, dtype=torch.uint8, device=dev)
    tours = torch.full((N,), SENTINEL, dtype=torch.int32, device=dev)
    costs = torch.full((B,), float(SENTINEL), dtype=torch.float32, device=dev)
    missing, out_scores, closed = (torch.full((B,), SENTINEL, dtype=torch.int32, device=dev) for _ in range(3))
    status = _lib.lib.tspgnn_tour_beam(_lib.ptr(s), _lib.ptr(t["uv"]), _lib.ptr(t["wc"]), _lib.ptr(t["seg"]),
                                       _lib.ptr(t["vseg"]), B, n_max, beam, select if isinstance(select, int) else
                                       decode.SELECT[select], _lib.ptr(ws), need + extra - short, _lib.ptr(tours),
                                       _lib.ptr(costs), _lib.ptr(missing), _lib.ptr(out_scores), _lib.ptr(closed),
                                       _lib.current_stream())
    torch.cuda.synchronize()
    return (status, tours.cpu().numpy(), costs.cpu().numpy().view(np.uint32), missing.cpu().numpy(),
            out_scores.cpu().numpy(), closed.cpu().numpy())


def compare(case, got, want):
    status, tours, costs, missing, scores, closed = got
    assert status == 0, _lib.lib.tspgnn_last_error()
    for b, w in enumerate(want):
        at = (b, int(case["n"][b]))
        assert [int(v) for v in tours[case["vseg"][b]:case["vseg"][b + 1]]] == w["tour"], at
        assert int(missing[b]) == w["n_missing"], at
        assert int(scores[b]) == w["score"] and int(closed[b]) == w["n_closed"], at
        assert int(costs[b]) == int(np.float32(w["cost"]).view(np.uint32)), (at, costs[b:b + 1].view(np.float32), w["cost"])


def check(case, scores, beam, **kw):
    """Both selects of one (batch, beam) against the restatement; and the tour chosen by cost costs no more than the one
    chosen by score wherever the final list holds a closed entry (both are then closed entries of the same list)."""
    out = {}
    for select in SELECTS:
        want = ref.beam_batch(case, scores, beam, select)
        got = launch(case, scores, beam, select, **kw)
        compare(case, got, want)
        out[select] = (got, want)
    by_score, by_cost = out["score"][0], out["cost"][0]
    for b in range(len(case["n"])):
        assert by_score[5][b] == by_cost[5][b]
        if by_cost[5][b] > 0:
            assert by_cost[2][b:b + 1].view(np.float32)[0] <= by_score[2][b:b + 1].view(np.float32)[0], b
    return out


# ------------------------------------------------------------------------------------------- the scores


def test_scores_against_the_float64_restatement(cuda_device):
    votes = np.concatenate([np.random.RandomState(31).randn(100000).astype(np.float32) * 8, cases.SPECIAL])
    want = ref.q_scores(votes).astype(np.int64)
    second = ref.q_scores_second(votes).astype(np.int64)
    # two float64 formulations differ by a few ulp of 65536 logsigmoid(v), ~1e-9: only a value that close to a half-integer
    # rounds the other way, so at most 1 entry in 10^4 may differ, and by one unit
    assert np.abs(second - want).max() <= 1 and (second != want).sum() <= len(votes) // 10000
    got = tspgnn.edge_scores(torch.from_numpy(votes).to("cuda:0"))
    assert got.dtype == torch.int32 and got.shape == (len(votes),)
    got = got.cpu().numpy().astype(np.int64)
    print("scores: %d of %d differ from the restatement, %d between its two formulations"
          % ((got != want).sum(), len(votes), (second != want).sum()))
    assert np.abs(got - want).max() <= 1
    assert (got != want).sum() <= len(votes) // 10000
    assert np.array_equal(got[-len(cases.SPECIAL):], want[-len(cases.SPECIAL):])     # the specials exactly
    assert got.min() >= -(1 << 22) and got.max() <= 0


# ------------------------------------------------------------------------------------------- the beam kernel


@pytest.mark.parametrize("n", [4, 5, 40])
def test_complete_graphs_small(cuda_device, n):
    """beam 1 .. 1024 on one mask word: fewer candidates than `beam` in the early steps (n = 4, 5: in every step), lists
    that end inside a wave (7, 65) and on its boundary (64)."""
    for beam in (1, 2, 7, 64, 65, 1024):
        out = check(cases.complete_case(n), bc.scores_of("complete_case", n), beam)
        assert out["score"][1][0]["n_missing"] == 0 and out["score"][1][0]["stranded"] is None


@pytest.mark.parametrize("n", [64, 65, 128, 129, 256])
def test_complete_graphs_at_the_mask_and_workgroup_boundaries(cuda_device, n):
    for beam in (1, 64):
        check(cases.complete_case(n), bc.scores_of("complete_case", n), beam)


def test_complete_graph_129_at_beam_300(cuda_device):
    check(cases.complete_case(129), bc.scores_of("complete_case", 129), 300)


def test_all_scores_equal(cuda_device):
    """n = 5 and 70 with one score everywhere: the (i, u) order decides every step."""
    scores = bc.scores_of("ties_case")
    assert len(set(scores.tolist())) == 1
    for beam in (1, 3, 64, 200):
        check(cases.ties_case(), scores, beam)


def test_scores_at_the_clamp(cuda_device):
    case, scores = bc.clamp_case()
    assert scores.min() < -(1 << 22) and scores.max() > 0
    for beam in (1, 16, 100):
        check(case, scores, beam)
    clamped = np.clip(scores, -(1 << 22), 0)
    for a, b in zip(launch(case, scores, 16, "cost")[1:], launch(case, clamped, 16, "cost")[1:]):
        assert np.array_equal(a, b)


def test_sparse_graphs_strand_and_mix_closed_with_unclosed(cuda_device):
    case, scores = cases.sparse_case(), bc.scores_of("sparse_case")
    seen = []
    for beam in bc.SPARSE_BEAMS:
        out = check(case, scores, beam)
        seen += [(w["stranded"] is not None, w["n_closed"], w["n_final"]) for w in out["score"][1]]
    assert sum(s for s, _, _ in seen) == 11                              # the stranded path and its fill
    assert seen[8][:2] == (False, 10) and seen[8][2] > 10                # n = 12 at beam 64: closed and unclosed entries


def test_untouched_vertex_no_edges_bad_edges_and_surplus_edges(cuda_device):
    case, scores = cases.odd_case(), bc.scores_of("odd_case")
    for beam in (1, 5, 64):
        out = check(case, scores, beam)
        lonely, empty, junk, multi = out["score"][1]
        assert lonely["stranded"] is not None and lonely["n_missing"] >= 2
        assert empty["tour"] == list(range(6)) and empty["n_missing"] == 6 and empty["score"] == 0
        assert junk["tour"] == [0, 1, 2, 3] and junk["n_missing"] == 3
        assert multi["n_missing"] == 0 and multi["stranded"] is None


def test_the_exhaustive_beam_on_the_device(cuda_device):
    case = bc.exhaustive_case()
    scores = ref.q_scores(case["vote"])
    for beam in (720, 1024):
        out = check(case, scores, beam)
        want = out["cost"][1][0]
        assert want["tour"] == bc.EXHAUSTIVE_TOUR and want["cost"] == bc.EXHAUSTIVE_COST and want["n_closed"] == 720
        assert out["cost"][0][2].view(np.float32)[0] == bc.EXHAUSTIVE_COST


@functools.lru_cache(maxsize=None)
def ragged_expected(beam, select):
    return ref.beam_batch(cases.ragged_case(), bc.scores_of("ragged_case"), beam, select)


def test_ragged_batch_equals_each_instance_alone(cuda_device):
    case, scores = cases.ragged_case(), bc.scores_of("ragged_case")
    beam = 33
    for select in SELECTS:
        want = ragged_expected(beam, select)
        first = launch(case, scores, beam, select)
        compare(case, first, want)
        for kw in (dict(n_max=256), dict(fill=0xFF), dict(extra=4096, fill=0xFF), {}):    # {}: the same launch again
            again = launch(case, scores, beam, select, **kw)
            assert again[0] == 0
            assert all(np.array_equal(a, b) for a, b in zip(first[1:], again[1:])), kw
        for k, inst in enumerate(cases.ragged_instances()):
            alone = cases.batch([inst])
            sl = slice(case["seg"][k], case["seg"][k + 1])
            compare(alone, launch(alone, scores[sl], beam, select), [want[k]])
            if inst[0] <= 128:      # another workgroup shape and mask width, the same result
                compare(alone, launch(alone, scores[sl], beam, select, n_max=2 * inst[0] + 1), [want[k]])


def test_refusals_leave_the_outputs_untouched(cuda_device):
    case, scores = cases.complete_case(5), bc.scores_of("complete_case", 5)
    for kw, code in ((dict(n_max=257), -2), (dict(beam=1025), -2), (dict(n_max=3), -1), (dict(beam=0), -1),
                     (dict(select=2), -1), (dict(select=-1), -1), (dict(short=1), -1)):
        args = dict(beam=4, select="score")
        args.update(kw)
        status, tours, costs, missing, out_scores, closed = launch(case, scores, **args)
        assert status == code, kw
        assert (tours == SENTINEL).all() and (missing == SENTINEL).all() and (costs.view(np.float32) == SENTINEL).all()
        assert (out_scores == SENTINEL).all() and (closed == SENTINEL).all()
    out = torch.full((64,), SENTINEL, dtype=torch.int32, device="cuda:0")
    p = _lib.ptr(out)
    for k in (0, 9, 15):
        args = [p, p, p, p, p, 1, 5, 4, 0, p, 1 << 30, p, p, p, p, p, _lib.current_stream()]
        args[k] = None
        assert _lib.lib.tspgnn_tour_beam(*args) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()


# ------------------------------------------------------------------------------------------- the Python surface

T = 8
TARGET = 0.2


@functools.lru_cache(maxsize=None)
def trained():
    z = np.load(os.path.join(GOLDEN, "trained_d64.npz"))
    model = tspgnn.build_network(64)
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer())
    model.store.load({k: z[k].astype(np.float64) for k in z.files})
    rng = np.random.RandomState(5)
    instances = [tspgnn.random_instance(20, rng) for _ in range(5)]
    return model, sess, instances


def prepared():
    model, sess, instances = trained()
    EV, W, C, route_exists, n_vertices, n_edges = tspgnn.InstanceLoader.create_batch(instances, target_cost=TARGET)
    feed = {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: T, model["route_exists"]: route_exists,
            model["n_vertices"]: n_vertices, model["n_edges"]: n_edges}
    return sess.prepare(feed), EV, n_vertices


@functools.lru_cache(maxsize=None)
def decoded():
    model, sess, instances = trained()
    return tspgnn.decode_tours(sess, model, instances, T, target_costs=[TARGET] * len(instances), beam=16, select="cost",
                               polish=True)


def test_decode_tours_with_a_beam_end_to_end(cuda_device):
    model, sess, instances = trained()
    res = decoded()
    for (Ma, Mw, _), r in zip(instances, res):
        n = Ma.shape[0]
        assert isinstance(r, tspgnn.BeamTour) and r[:8] == tspgnn.DecodedTour(*r[:8])
        assert sorted(r.tour) == list(range(n)) and r.tour[0] == 0 and r.tour[1] < r.tour[-1]
        A = (Ma + Ma.T) != 0
        pairs = list(zip(r.tour, r.tour[1:] + r.tour[:1]))
        assert r.n_missing == sum(1 for a, b in pairs if not A[a, b])
        assert r.feasible == (r.n_missing == 0)
        cost = np.float32(0)
        for a, b in pairs:
            if A[a, b]:
                cost = np.float32(cost + np.float32(Mw[min(a, b), max(a, b)]))
        assert np.float32(r.cost) == cost
        assert r.target_cost == TARGET and 0.0 <= r.prediction <= 1.0
        assert -(1 << 22) * n <= r.score <= 0 and 0 < r.n_closed <= 16         # complete graphs: every entry closes
        assert sorted(r.polished_tour) == list(range(n))
        assert r.polished_cost <= r.cost * (1 + 2 * n * 2.0 ** -24)             # as for the greedy decoder's polish
        print("n=%d beam-16 cost %.4f  polished %.4f  score %d  closed %d" % (n, r.cost, r.polished_cost, r.score, r.n_closed))


def test_the_restatement_reproduces_the_device_tours_from_its_scores(cuda_device):
    model, sess, instances = trained()
    b, EV, n_vertices = prepared()
    out = sess.forward_device(b)
    torch.cuda.synchronize()
    scores = tspgnn.edge_scores(out["E_vote"])
    slow = tspgnn.beam_tours(b, scores, 16, "cost")
    torch.cuda.synchronize()
    want = [x.cpu().numpy() for x in slow[:5]]
    votes = out["E_vote"].cpu().numpy()
    assert np.abs(scores.cpu().numpy().astype(np.int64) - ref.q_scores(votes)).max() <= 1
    case = {"n": n_vertices.astype(np.int32), "seg": b.seg.cpu().numpy(), "vseg": slow.vseg.cpu().numpy(), "uv": EV.uv,
            "wc": b.WC.cpu().numpy(), "vote": votes}
    compare(case, (0, want[0], want[1].view(np.uint32), want[2], want[3], want[4]),
            ref.beam_batch(case, scores.cpu().numpy(), 16, "cost"))
    # decode_tours at the same targets is this pipeline
    for k, r in enumerate(decoded()):
        v0 = case["vseg"][k]
        assert r.tour == [int(v) for v in want[0][v0:v0 + 20]] and np.float32(r.cost) == want[1][k]
        assert r.score == int(want[3][k]) and r.n_closed == int(want[4][k])
    # enqueued behind the forward without a host synchronisation: the same tensors
    out = sess.forward_device(b)
    fast = tspgnn.beam_tours(b, tspgnn.edge_scores(out["E_vote"]), 16, "cost")
    assert all(np.array_equal(x.cpu().numpy().view(np.int32), w.view(np.int32)) for x, w in zip(fast[:5], want))
    # a cap that forces one launch per instance, and one per two
    per = int(_lib.lib.tspgnn_tour_beam_workspace_bytes(1, 20, 16))
    for cap, launches in ((per, 5), (2 * per + 1, 3), (1, 5)):
        assert len(decode.beam_ranges(5, 20, 16, cap)[0]) == launches
        split = tspgnn.beam_tours(b, scores, 16, "cost", workspace_bytes=cap)
        assert all(np.array_equal(x.cpu().numpy().view(np.int32), w.view(np.int32)) for x, w in zip(split[:5], want))
    assert len(decode.beam_ranges(5, 20, 16)[0]) == 1


def test_chunks_selects_and_the_greedy_default(cuda_device):
    model, sess, instances = trained()
    targets = [TARGET] * len(instances)
    res = decoded()
    again = tspgnn.decode_tours(sess, model, instances, T, target_costs=targets, beam=16, select="cost", max_graphs=2,
                                workspace_bytes=1)
    for a, c in zip(res, again):
        assert a[:6] == c[:6] and a[8:] == c[8:] and c.polished_tour is None
    by_score = tspgnn.decode_tours(sess, model, instances, T, target_costs=targets, beam=16)
    for a, c in zip(res, by_score):
        assert a.n_closed == c.n_closed and a.cost <= c.cost and c.score >= a.score
    # without beam: the greedy decoder's records, as before
    b, EV, n_vertices = prepared()
    dec = tspgnn.tours_from_votes(b, sess.forward_device(b)["E_vote"])
    tours, costs, missing = (x.cpu().numpy() for x in dec[:3])
    greedy = tspgnn.decode_tours(sess, model, instances, T, target_costs=targets)
    for k, r in enumerate(greedy):
        assert type(r) is tspgnn.DecodedTour and len(r) == 8
        assert r.tour == [int(v) for v in tours[20 * k:20 * k + 20]] and np.float32(r.cost) == costs[k]
        assert r.n_missing == int(missing[k]) and r.polished_tour is None
    with pytest.raises(TypeError):
        tspgnn.decode_tours(sess, model, instances, T, target_costs=targets, select="cost")
    with pytest.raises(ValueError):
        tspgnn.decode_tours(sess, model, instances, T, target_costs=targets, beam=1025)
    with pytest.raises(ValueError):
        tspgnn.decode_tours(sess, model, instances, T, target_costs=targets, beam=4, select="best")


def test_decoded_tour_curve_forwards_beam_and_select(cuda_device):
    from tspgnn import dataset, experiments
    model, sess, instances = trained()
    devs = [0.02, 0.5, 2.0]
    Q = [dataset._target(Ma, Mw, route) for Ma, Mw, route in instances]
    res = tspgnn.decode_tours(sess, model, instances, T, beam=16, select="cost")
    got = experiments.decoded_tour_curve(sess, model, instances, T, devs, beam=16, select="cost")
    want = experiments.curve_from_costs([r.cost for r in res], [True] * len(res), Q, devs)
    for k in ("tpr", "fpr", "acc"):
        assert np.array_equal(got[k], want[k]), k
