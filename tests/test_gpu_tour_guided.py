"""The vote-guided tour search on the GPU: tspgnn_vote_neighbors (csrc/tour_guided.hip) against the NumPy restatement of
tests/guided_reference.py byte for byte; tspgnn_tour_search_cand / _cand_tri (csrc/tour_search.hip) against
tspgnn_tour_search_knn bit for bit on the table that entry point builds, against the restatement tour for tour on
arbitrary tables, and against each other; the argument checks; label_tours(candidates=) under chunking; and
decode_tours(..., polish=True, guide=) against its pieces composed by hand on tests/golden/trained_d64.npz.  Nothing here
claims that guided tours are good."""
import functools
import os

import numpy as np
import pytest
import torch

import decode_cases as cases
import guided_reference as gref
import knn_search_reference as ref
import tspgnn
from baseline_reference import cost64, euclidean, packed, sparse_planted
from conftest import GOLDEN
from tspgnn import _lib, dataset
from test_gpu_tour_knn import _integer, _same

pytestmark = pytest.mark.gpu

SENTINEL = 201
KS = ((1, 0), (5, 0), (0, 5), (3, 4), (32, 0), (16, 16))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ------------------------------------------------------------------------------------------- tspgnn_vote_neighbors
def rows_launch(case, k_vote, k_near, n_max=None):
    """The raw entry point on a decode_cases batch with the CSR of guided_reference.vertex_csr -> (status, uint8 [N, K]),
    the table prefilled with SENTINEL."""
    rowptr, eid = gref.vertex_csr(case)
    t = {k: _dev(case[k]) for k in ("vote", "uv", "wc", "seg", "vseg")}
    t["rowptr"], t["eid"] = _dev(rowptr), _dev(eid)
    if case["vote"].size == 0:
        t["vote"], t["uv"], t["wc"], t["eid"] = (torch.zeros(s, dtype=d, device="cuda:0") for s, d in (
            ((1,), torch.float32), ((1, 2), torch.int32), ((1, 2), torch.float32), ((1,), torch.int32)))
    B, N = len(case["n"]), int(case["vseg"][-1])
    tab = torch.full((N, max(k_vote + k_near, 1)), SENTINEL, dtype=torch.uint8, device="cuda:0")
    status = _lib.lib.tspgnn_vote_neighbors(_lib.ptr(t["vote"]), _lib.ptr(t["uv"]), _lib.ptr(t["wc"]), _lib.ptr(t["seg"]),
                                            _lib.ptr(t["vseg"]), _lib.ptr(t["rowptr"]), _lib.ptr(t["eid"]), B,
                                            int(case["n"].max()) if n_max is None else n_max, k_vote, k_near,
                                            _lib.ptr(tab), _lib.current_stream())
    torch.cuda.synchronize()
    return status, tab.cpu().numpy()


@functools.lru_cache(maxsize=None)
def want_rows(name, k_vote, k_near, *args):
    return gref.case_rows(getattr(cases, name)(*args), k_vote, k_near)


def check_rows(name, *args):
    case = getattr(cases, name)(*args)
    for kv, kn in KS:
        status, tab = rows_launch(case, kv, kn)
        assert status == 0, _lib.lib.tspgnn_last_error()
        want = want_rows(name, kv, kn, *args)
        assert np.array_equal(tab, want), (kv, kn, np.argwhere(tab != want)[:4])


@pytest.mark.parametrize("n", [4, 5, 40, 64, 65, 128, 129, 256])
def test_rows_on_complete_graphs(cuda_device, n):
    check_rows("complete_case", n)


@pytest.mark.parametrize("name", ["ties_case", "special_case", "sparse_case", "odd_case", "ragged_case"])
def test_rows_where_ties_special_values_and_missing_edges_decide(cuda_device, name):
    check_rows(name)


def test_rows_of_a_ragged_batch_equal_each_instance_alone(cuda_device):
    v = cases.ragged_case()["vseg"]
    for kv, kn in ((3, 4), (16, 16)):
        want = want_rows("ragged_case", kv, kn)
        status, tab = rows_launch(cases.ragged_case(), kv, kn, n_max=256)
        assert status == 0 and np.array_equal(tab, want)
        for k, inst in enumerate(cases.ragged_instances()):
            alone = cases.batch([inst])
            for n_max in (None, min(256, 2 * inst[0] + 1)):     # the other workgroup shape where there is one
                status, tab = rows_launch(alone, kv, kn, n_max=n_max)
                assert status == 0 and np.array_equal(tab, want[v[k]:v[k + 1]]), (k, n_max)


def test_rows_refusals_leave_the_table_untouched(cuda_device):
    case = cases.complete_case(5)
    for n_max, kv, kn, code in ((257, 4, 4, -2), (3, 4, 4, -1), (5, -1, 4, -1), (5, 4, -1, -1), (5, 0, 0, -1),
                                (5, 33, 0, -1), (5, 17, 16, -1)):
        status, tab = rows_launch(case, kv, kn, n_max=n_max)
        assert status == code, (n_max, kv, kn)
        assert (tab == SENTINEL).all()
    out = torch.full((40,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    p = _lib.ptr(out)
    assert _lib.lib.tspgnn_vote_neighbors(p, p, p, p, p, None, p, 1, 5, 4, 4, p, _lib.current_stream()) == -1
    assert _lib.lib.tspgnn_vote_neighbors(p, p, p, p, p, p, p, 0, 5, 4, 4, p, _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()


# ------------------------------------------------------------------------------------------- tspgnn_tour_search_cand
def _search(insts, inits, tri, seed, restarts, kicks, tables=None, neighbors=None, n_max=None, raw=False):
    """One launch of the candidate-list search of one layout straight through the C ABI: tables (one [n, K] array per
    instance) -> the _cand entry point, else neighbors=K -> the _knn one.  -> (tours split per instance, fp32 costs); with
    raw=True (status, flat tours, costs), the outputs prefilled with SENTINEL."""
    ns = np.array([m.shape[0] for m, _ in insts], dtype=np.int32)
    sizes = ns.astype(np.int64) * (ns - 1) // 2 if tri else ns.astype(np.int64) ** 2
    w_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    t_off = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    packs = []
    for (Ma, Mw) in insts:
        A = dataset._edge_mask(Ma)[None]
        W = np.asarray(Mw, dtype=np.float64)[None]
        packs.append((dataset._penalised_tri if tri else dataset._penalised)(A, W).reshape(-1))
    d = {k: _dev(v) for k, v in (("W", np.concatenate(packs)), ("w_off", w_off), ("t_off", t_off), ("n", ns))}
    init = None if inits is None else _dev(np.concatenate([np.asarray(it) for it in inits]).astype(np.int32))
    tours = torch.full((int(ns.sum()),), SENTINEL, dtype=torch.int32, device="cuda:0")
    costs = torch.full((len(insts),), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    if tables is not None:
        K = tables[0].shape[1]
        cand = _dev(np.concatenate([np.asarray(t, dtype=np.uint8).reshape(-1) for t in tables]))
        c_off = _dev((t_off * K).astype(np.int64))
        name, extra, knn = "tspgnn_tour_search_cand", (_lib.ptr(cand), _lib.ptr(c_off)), (K,)
    else:
        name, extra, knn = "tspgnn_tour_search_knn", (), (neighbors,)
    status = getattr(_lib.lib, name + ("_tri" if tri else ""))(
        _lib.ptr(d["W"]), _lib.ptr(d["w_off"]), _lib.ptr(d["n"]), _lib.ptr(init), _lib.ptr(d["t_off"]), None, *extra,
        len(insts), int(ns.max()) if n_max is None else n_max, restarts, kicks, *knn, seed, _lib.ptr(tours),
        _lib.ptr(costs), _lib.current_stream())
    torch.cuda.synchronize()
    if raw:
        return status, tours.cpu().numpy(), costs.cpu().numpy()
    assert status == 0, _lib.lib.tspgnn_last_error()
    return np.split(tours.cpu().numpy(), np.cumsum(ns)[:-1]), costs.cpu().numpy()


def _knn_table(W32, K):
    """The table tspgnn_tour_search_knn builds, in K columns: the min(K, n-1) nearest by (w, y), then skips."""
    n = W32.shape[0]
    N = ref.neighbor_sets(W32, K)
    tab = np.repeat(np.arange(n)[:, None], K, axis=1)
    tab[:, :N.shape[1]] = N
    return tab.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def knn_instances(tri):
    """Every maker of test_gpu_tour_knn.py at every size of the layout, with a random starting tour each."""
    rng = np.random.RandomState(80 + tri)
    insts, inits = [], []
    for n in ((65, 129, 200, 256) if tri else (4, 5, 7, 12, 33, 64, 65, 128)):
        for make in (euclidean, sparse_planted, _integer):
            insts.append(make(rng, n))
            inits.append(rng.permutation(n))
    return insts, inits, [packed(Ma, Mw) for Ma, Mw in insts]


@pytest.mark.parametrize("K", [1, 5, 10, 32])
@pytest.mark.parametrize("tri", [False, True], ids=["square", "tri"])
def test_cand_with_the_knn_table_equals_knn_bitwise(cuda_device, tri, K):
    insts, inits, W32 = knn_instances(tri)
    tables = [_knn_table(W, K) for W in W32]
    for given in (inits, None):
        knn = _search(insts, given, tri, 23, 2, 4, neighbors=K)
        cand = _search(insts, given, tri, 23, 2, 4, tables=tables)
        assert _same(knn, cand)
        for (Ma, _), t in zip(insts, cand[0]):
            assert sorted(t) == list(range(Ma.shape[0]))


@pytest.mark.parametrize("kind", gref.TABLES)
@pytest.mark.parametrize("layout", ["square", "tri"])
def test_cand_with_arbitrary_tables_equals_the_restatement(cuda_device, layout, kind):
    sizes = ref.TRI_N if layout == "tri" else ref.SQUARE_N
    found = [ref.instance(layout, n) for n in sizes]
    insts, inits = [(Ma, Mw) for Ma, Mw, _ in found], [init for _, _, init in found]
    tables = [gref.table(layout, n, kind) for n in sizes]
    for kicks in gref.KICKS:
        tours, costs = _search(insts, inits, layout == "tri", gref.SEED, 1, kicks, tables=tables)
        for n, (Ma, Mw), init, t, c in zip(sizes, insts, inits, tours, costs):
            want = gref.expected(layout, n, kind)[0][kicks]
            assert t.tolist() == want, (n, kicks)
            W = packed(Ma, Mw)
            c64 = cost64(W, want)
            assert abs(float(c) - c64) <= n * 2.0 ** -23 * c64, (n, kicks, float(c), c64)
            if kind == "skip" and kicks == 0:       # no pair at all: the start comes back, with the cost the chain summed
                assert want == ref.canonical(init)
                assert np.float32(c).view(np.uint32) == np.float32(ref.cost32(W, init)).view(np.uint32)


def test_cand_tri_equals_cand_bitwise_with_8_columns(cuda_device):
    rng = np.random.RandomState(61)         # the sizes of test_tri_equals_square_bitwise_with_neighbors_8
    sizes = [4, 5, 9, 64, 65, 127, 128] + [int(v) for v in rng.randint(6, 128, size=9)]
    insts, inits, tables = [], [], []
    for k, n in enumerate(sizes):
        insts.append((euclidean, sparse_planted, _integer)[k % 3](rng, n))
        inits.append(rng.permutation(n))
        tables.append(rng.randint(0, n + (k % 4 == 0) * 9, size=(n, 8)).astype(np.uint8))   # every fourth: entries >= n too
    assert len(insts) == 16
    for restarts, kicks in ((4, 6), (1, 0)):
        sq = _search(insts, inits, False, 22, restarts, kicks, tables=tables)
        assert _same(sq, _search(insts, inits, True, 22, restarts, kicks, tables=tables))
        for n, t in zip(sizes, sq[0]):
            assert sorted(t) == list(range(n))


def test_cand_refusals_leave_the_outputs_untouched(cuda_device):
    rng = np.random.RandomState(81)
    insts = [euclidean(rng, 6), euclidean(rng, 9)]

    def refused(tri, code, needle=None, **kw):
        args = dict(tables=[np.zeros((6, 8), np.uint8), np.zeros((9, 8), np.uint8)], restarts=2, n_max=None)
        args.update(kw)
        status, tours, costs = _search(insts, None, tri, 5, args["restarts"], 3, tables=args["tables"], n_max=args["n_max"],
                                       raw=True)
        assert status == code, (tri, kw, status)
        assert needle is None or needle in _lib.lib.tspgnn_last_error()
        assert (tours == SENTINEL).all() and (costs == SENTINEL).all()

    for tri in (False, True):
        refused(tri, -1, b"columns=33", tables=[np.zeros((6, 33), np.uint8), np.zeros((9, 33), np.uint8)])
    refused(True, -1, b"at most 9", restarts=10, n_max=256)
    refused(False, -2, b"129", n_max=129)
    refused(True, -2, b"257", n_max=257)
    # columns = 0, a null table and an empty launch: straight at the entry points
    out = torch.full((64,), SENTINEL, dtype=torch.int32, device="cuda:0")
    p, st = _lib.ptr(out), _lib.current_stream()
    for fn in (_lib.lib.tspgnn_tour_search_cand, _lib.lib.tspgnn_tour_search_cand_tri):
        assert fn(p, p, p, None, p, None, p, p, 2, 9, 2, 3, 0, 5, p, p, st) == -1
        assert b"columns=0" in _lib.lib.tspgnn_last_error()
        assert fn(p, p, p, None, p, None, None, p, 2, 9, 2, 3, 8, 5, p, p, st) == -1
        assert b"null pointer" in _lib.lib.tspgnn_last_error()
        assert fn(p, p, p, None, p, None, p, p, 0, 9, 2, 3, 8, 5, p, p, st) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()


# ------------------------------------------------------------------------------------------- label_tours(candidates=)
def test_label_tours_with_candidates_is_invariant_to_chunking(cuda_device):
    rng = np.random.RandomState(82)
    insts, inits, tables = [], [], []
    for k in range(24):
        n = int(rng.randint(12, 41))
        insts.append((euclidean, sparse_planted, _integer)[k % 3](rng, n))
        inits.append([int(v) for v in rng.permutation(n)] if k % 2 else None)
        if k % 4 == 0:
            tab = _knn_table(packed(*insts[-1]), 6)                          # the nearest six
        elif k % 4 == 1:
            tab = rng.randint(0, 256, size=(n, 6))                          # mostly entries >= n
        elif k % 4 == 2:
            tab = rng.randint(0, n, size=(n, 6))
        else:
            tab = np.repeat(np.arange(n)[:, None], 6, axis=1)               # no pair at all
        tables.append(tab)
    kw = dict(restarts=3, kicks=5, seed=4, lower_bound=False)
    r1 = dataset.label_tours(insts, init_tours=inits, candidates=tables, **kw)
    assert len(r1) == 24
    for (Ma, _), r in zip(insts, r1):
        assert sorted(r.tour) == list(range(Ma.shape[0])) and r.tour[0] == 0 and r.tour[1] < r.tour[-1]
    strip = lambda rs: [(r.tour, r.cost, r.feasible) for r in rs]   # noqa: E731  (lb is nan without the bound)
    for chunk in (5, 24):
        assert strip(dataset.label_tours(insts, init_tours=inits, candidates=tables, chunk=chunk, **kw)) == strip(r1)
    sub = [3, 8, 12, 23]
    alone = dataset.label_tours([insts[k] for k in sub], init_tours=[inits[k] for k in sub],
                                candidates=[tables[k] for k in sub], index=sub, **kw)
    assert strip(alone) == strip([r1[k] for k in sub])
    # the tables are what the search descends over: the nearest six everywhere give other tours
    knn = dataset.label_tours(insts, init_tours=inits, neighbors=6, **kw)
    assert [a.tour == b.tour for a, b in zip(r1, knn)][::4] == [True] * 6 and strip(knn) != strip(r1)


# ------------------------------------------------------------------------------------------- decode_tours(guide=)
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


@pytest.mark.parametrize("beam", [None, 16])
def test_decode_tours_with_a_guide_equals_its_pieces(cuda_device, beam):
    model, sess, instances = trained()
    targets = [TARGET] * len(instances)
    kw = {} if beam is None else {"beam": beam}
    res = tspgnn.decode_tours(sess, model, instances, T, target_costs=targets, polish=True, guide=(4, 4), **kw)
    # by hand: prepare -> forward_device -> decoder + vote_neighbors -> label_tours(init_tours, candidates)
    EV, W, C, route_exists, n_vertices, n_edges = tspgnn.InstanceLoader.create_batch(instances, target_cost=TARGET)
    feed = {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: T, model["route_exists"]: route_exists,
            model["n_vertices"]: n_vertices, model["n_edges"]: n_edges}
    b = sess.prepare(feed)
    out = sess.forward_device(b)
    tab = tspgnn.vote_neighbors(b, out["E_vote"], 4, 4)
    if beam is None:
        dec = tspgnn.tours_from_votes(b, out["E_vote"])
    else:
        dec = tspgnn.beam_tours(b, tspgnn.edge_scores(out["E_vote"]), beam)
    assert tab.dtype == torch.uint8 and tuple(tab.shape) == (b.N, 8)
    tab, tours = tab.cpu().numpy(), dec.tours.cpu().numpy()
    costs, missing, pred = dec.costs.cpu().numpy(), dec.n_missing.cpu().numpy(), out["predictions"].cpu().numpy()
    v0 = np.concatenate([[0], np.cumsum(n_vertices)])
    case = {"n": n_vertices.astype(np.int32), "seg": b.seg.cpu().numpy(), "vseg": v0.astype(np.int32), "uv": EV.uv,
            "wc": b.WC.cpu().numpy(), "vote": out["E_vote"].cpu().numpy()}
    assert np.array_equal(tab, gref.case_rows(case, 4, 4))
    decoded = [[int(v) for v in tours[v0[i]:v0[i + 1]]] for i in range(len(instances))]
    tables = [tab[v0[i]:v0[i + 1]] for i in range(len(instances))]
    lab = tspgnn.label_tours([(Ma, Mw) for Ma, Mw, _ in instances], init_tours=decoded, candidates=tables, restarts=1,
                             kicks=0, lower_bound=False)
    plain = tspgnn.decode_tours(sess, model, instances, T, target_costs=targets, polish=True, **kw)
    for i, (r, p) in enumerate(zip(res, plain)):
        assert r.tour == decoded[i] and np.float32(r.cost) == costs[i] and r.n_missing == int(missing[i])
        assert r.feasible == (missing[i] == 0) and r.prediction == float(pred[i]) and r.target_cost == TARGET
        assert r.polished_tour == lab[i].tour and r.polished_cost == lab[i].cost
        assert type(r) is type(p) and r[:6] == p[:6] and r[8:] == p[8:]        # the guide changes the polish alone
        assert lab[i].feasible and sorted(r.polished_tour) == list(range(20))
        Mw = np.asarray(instances[i][1], dtype=np.float64)
        assert r.polished_cost <= dataset._cycle_cost(Mw[None], np.array([decoded[i]]))[0]     # both fp64, one summation
        print("n=20 decoded %.4f  guided polish %.4f  full-scan polish %.4f" % (r.cost, r.polished_cost, p.polished_cost))
    # guide=K is (K, 0), and decoded_tour_curve hands guide through
    a = tspgnn.decode_tours(sess, model, instances, T, target_costs=targets, polish=True, guide=8, **kw)
    c = tspgnn.decode_tours(sess, model, instances, T, target_costs=targets, polish=True, guide=(8, 0), max_graphs=2, **kw)
    assert a == c
    from tspgnn import experiments
    Q = [dataset._target(Ma, Mw, route) for Ma, Mw, route in instances]
    got = experiments.decoded_tour_curve(sess, model, instances, T, [0.02, 0.5], polish=True, guide=(4, 4), **kw)
    want = experiments.curve_from_costs([r.polished_cost for r in res], [True] * len(res), Q, [0.02, 0.5])
    assert all(np.array_equal(got[k], want[k]) for k in ("tpr", "fpr", "acc"))
