"""``build_network(d)`` and ``Session``: the operator surface of the reference's model.py
(/root/reference/model.py:9-171) on the MI355X-native path.

``build_network`` returns a dict with the reference's keys (model.py:97-104,123,147-157,167):
placeholders ``EV, W, C, time_steps, route_exists, n_vertices, n_edges`` and fetches
``last_states, predictions, TP, FP, TN, FN, acc, loss, train_step`` plus ``gnn``.  Callers do
exactly what train.py:25-42 does:

    model = build_network(64)
    sess = Session(); sess.run(global_variables_initializer())
    loss, acc, pred, TP, FP, TN, FN = sess.run([model['loss'], ...], feed_dict={model['EV']: EV, ...})

``model['EV']`` accepts the reference's dense float64/float32 matrix (converted once to index
form; it must be a 0/1 matrix with two ones per row, which is what create_batch emits) or a
``SparseEV`` that never materialises the dense matrix.
"""
import math
import threading
import zlib

import numpy as np
import torch

from . import _lib
from . import variables as V
from .graphnn import GEMM_ARITH, GraphNN, LSTMStateTuple, to_f32
from .instance_loader import SparseEV
from .mlp import Mlp
from .range_guard import decode, flag_bits
from . import route_head as RH

LEARNING_RATE = 2e-5          # model.py:13
L2NORM_SCALING = 1e-10        # model.py:14
GLOBAL_NORM_CLIP = 0.65       # model.py:15
STAT_FETCHES = ("loss", "acc", "TP", "FP", "TN", "FN")
ROUTE_STAT_FETCHES = ("route_loss", "route_acc", "route_TP", "route_FP", "route_TN", "route_FN")   # out["route_stats"]


class Placeholder(object):
    def __init__(self, name, dtype, ndim):
        self.name, self.dtype, self.ndim = name, dtype, ndim

    def __repr__(self):
        return "<tspgnn placeholder %s>" % self.name


class Fetch(object):
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "<tspgnn fetch %s>" % self.name


class _InitOp(Fetch):
    pass


def global_variables_initializer(seed=0):
    """Fetchable like tf.global_variables_initializer(): ``sess.run(global_variables_initializer())``."""
    op = _InitOp("init")
    op.seed = seed
    return op


class DeviceBatch(object):
    """One packed batch resident on the device (see Session.prepare)."""

    def copy_from(self, other):
        """Overwrite this batch's device tensors with ``other``'s (same shapes: same numbers of graphs, vertices and
        edges) -- lets a captured forward graph, which is bound to THIS batch's buffers, serve a stream of batches."""
        mine, theirs = self.tensors(), other.tensors()
        groups = [None if b.adj.loop_plan is None else b.adj.loop_plan[1:] for b in (self, other)]
        if (self.M, self.N, self.B, self.T) != (other.M, other.N, other.B, other.T) or len(mine) != len(theirs) \
                or groups[0] != groups[1] \
                or any(a.shape != b.shape or a.dtype != b.dtype for a, b in zip(mine, theirs)):
            raise ValueError("copy_from: the batches differ in shape")
        for a, b in zip(mine, theirs):
            a.copy_(b, non_blocking=True)
        return self

    def tensors(self):
        """Every device tensor of the batch (for stream bookkeeping when it was uploaded on another stream)."""
        out = [getattr(self, k, None) for k in ("WC", "labels", "seg", "route_edges")]   # (route_edges: a route-head batch)
        adj = getattr(self, "adj", None)
        if adj is not None:
            out.append(adj.uv)
            for csr in (adj.csr, adj.csr_t):
                out.extend(csr)
            if adj.loop_plan is not None:    # (the one-launch loop's work plan follows the batch's block structure)
                out.append(adj.loop_plan[0])
        return [t for t in out if torch.is_tensor(t)]


class Network(dict):
    """The dict build_network returns, plus the objects Session needs."""


def build_network(d, store=None, float_dtype=torch.float32, MLP_depth=3, Msg_last_activation=None, route_head=False,
                  route_loss=1.0, route_pos_weight=None):
    """model.py:9-170.  ``float_dtype=torch.bfloat16`` (the reference GraphNN's own float_dtype argument,
    graphnn.py:18) stores the embeddings as bf16 with fp32 accumulation (BASELINE config 5); training in that mode is
    mixed precision: bf16 tape, fp32 gradients and fp32 master variables (GraphNN.backward).  ``MLP_depth`` and
    ``Msg_last_activation`` are GraphNN's own (graphnn.py:15-16): hidden layers of the message MLPs, and the activation of
    their last layer.

    ``route_head=True`` adds a second per-edge head next to E_vote (which the network only ever averages into the decision
    logit): ``E_route``, an Mlp of E_vote's shape on the same final edge states, declared AFTER every other variable (the
    flat layout of a network without it is a prefix), trained with a per-edge sigmoid cross entropy against the placeholder
    ``route_edges`` (float32 [M], 1 where the edge lies on the instance's labelled tour: route_head.py).  ``train_step``
    then optimises loss + ``route_loss`` * route_loss + L2; the ``loss`` fetch stays the decision loss.  The edge loss is a
    mean over a problem's edges and then over the problems, a marked edge weighing ``route_pos_weight`` (None: balanced,
    (m - k) / max(k, 1) per problem of m edges with k marked).  New fetches: ``E_route`` (the per-edge logits),
    ``route_loss``, ``route_acc`` (the mean over the problems of the fraction of edges whose logit > 0 agrees with the
    mark), ``route_TP / FP / TN / FN`` (edge counts at that threshold).  Without ``route_head`` nothing changes: the same
    variables, launches and numbers."""
    d = int(d)
    store = store if store is not None else V.reset_default_store()
    GNN = Network()
    GNN.d = d
    GNN.float_dtype = float_dtype
    GNN.store = store
    # placeholders (model.py:18-29)
    GNN["route_exists"] = Placeholder("route_exists", np.float32, 1)
    GNN["n_vertices"] = Placeholder("n_vertices", np.int32, 1)
    GNN["n_edges"] = Placeholder("edges", np.int32, 1)
    GNN["EV"] = Placeholder("EV", np.float32, 2)
    GNN["W"] = Placeholder("edge_weight", np.float32, 2)
    GNN["C"] = Placeholder("target_cost", np.float32, 2)
    GNN["time_steps"] = Placeholder("time_steps", np.int32, 0)
    # model.py:33-43
    GNN.edge_init_MLP = Mlp(
        layer_sizes=[d / 8, d / 4, d / 2],
        activations=["relu" for _ in range(3)],
        output_size=d,
        name="E_init_MLP",
        name_internal_layers=True,
        kernel_initializer=V.xavier_uniform,
        bias_initializer=V.zeros_init,
        input_size=2,
        store=store,
    )
    # model.py:47
    store.declare("V_init", (1, d), V.normal_init)
    # model.py:57-94
    GNN["gnn"] = GraphNN(
        {"V": d, "E": d},
        {"EV": ("E", "V")},
        {"V_msg_E": ("V", "E"), "E_msg_V": ("E", "V")},
        {
            "V": [{"mat": "EV", "msg": "E_msg_V", "transpose?": True, "var": "E"}],
            "E": [{"mat": "EV", "msg": "V_msg_E", "var": "V"}],
        },
        name="TSP",
        MLP_depth=MLP_depth,
        Msg_last_activation=Msg_last_activation,
        float_dtype=float_dtype,
        store=store,
    )
    # model.py:107-115
    GNN.E_vote_MLP = Mlp(
        layer_sizes=[d for _ in range(3)],
        activations=["relu" for _ in range(3)],
        output_size=1,
        name="E_vote",
        name_internal_layers=True,
        kernel_initializer=V.xavier_uniform,
        bias_initializer=V.zeros_init,
        input_size=d,
        store=store,
    )
    for key in ("last_states", "predictions", "TP", "FP", "TN", "FN", "acc", "loss", "train_step"):
        GNN[key] = Fetch(key)
    GNN.route_head = bool(route_head)
    if GNN.route_head:
        GNN.route_loss_weight = float(route_loss)
        GNN.route_pos_weight = 0.0 if route_pos_weight is None else float(route_pos_weight)   # 0: the balanced rule
        weight_ok = route_pos_weight is None or (math.isfinite(GNN.route_pos_weight) and GNN.route_pos_weight > 0)
        if not math.isfinite(GNN.route_loss_weight) or not weight_ok:
            raise ValueError("build_network: route_loss=%r must be finite and route_pos_weight=%r positive (or None)"
                             % (route_loss, route_pos_weight))
        GNN.E_route_MLP = Mlp(
            layer_sizes=[d for _ in range(3)],
            activations=["relu" for _ in range(3)],
            output_size=1,
            name="E_route",
            name_internal_layers=True,
            kernel_initializer=V.xavier_uniform,
            bias_initializer=V.zeros_init,
            input_size=d,
            store=store,
        )
        GNN["route_edges"] = Placeholder("route_edges", np.float32, 1)
        for key in ("E_route",) + ROUTE_STAT_FETCHES:
            GNN[key] = Fetch(key)
    build_network.last = GNN
    return GNN


build_network.last = None


class Session(object):
    """Executes fetches of a network built by build_network on one MI355X.

    ``Session(model=None, device='cuda:0')``: without ``model`` it binds to the most recently
    built network (the TF default-graph behaviour train.py:202-206 relies on).

    There is no CPU compute path.  ``device='cpu'`` is accepted for PLUMBING ONLY -- the variable store, feed
    validation and the data-parallel collectives (which is how the gloo tests exercise them without a GPU); every
    fetch that would launch a kernel raises.

    Data parallelism: when ``torch.distributed`` is initialised (or ``process_group`` is given) with
    more than one rank, ``train_step`` all-reduces ONE bucket -- the flat gradient plus the batch statistics --
    and the fetched loss / acc / TP / FP / TN / FN are those of the global batch; replicas are made identical by a
    broadcast of the variables from rank 0 before the first training step."""

    def __init__(self, model=None, device=None, process_group=None):
        self.model = model if model is not None else build_network.last
        if self.model is None:
            raise RuntimeError("Session: call build_network(d) first")
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("tspgnn.Session needs an MI355X (no HIP device visible); there is no CPU path")
            device = "cuda:%d" % torch.cuda.current_device()
        self.device = torch.device(device)
        self.store = self.model.store
        if not self.store.finalized:
            self.store.finalize(self.device)
        self._adj_cache = threading.local()   # per thread: BatchPrefetcher prepares batches on a worker thread
        self._adam = None
        self.process_group = process_group
        self._replicas_synced = False
        self._synced_assignments = -1
        self._ever_synced = False     # data-parallel: the first train_step broadcasts unconditionally (train_step)
        self.last_range_bits = 0     # the f16x2 guard bits (1 overflow, 2 underflow) of the last flagged batch: diagnostics

    @property
    def world_size(self):
        """Ranks of the data-parallel group (1 without an initialised torch.distributed)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return 1
        return dist.get_world_size(self.process_group)

    def _require_gpu(self, what):
        if self.device.type != "cuda":
            raise RuntimeError("tspgnn.Session(device=%r) is plumbing only: %s launches HIP kernels and needs an MI355X; "
                               "there is no CPU path" % (str(self.device), what))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def close(self):
        pass

    # ------------------------------------------------------------------ feeding
    def _f32(self, a, pinned=False):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        if pinned and self.device.type == "cuda":
            return t.pin_memory().to(self.device, non_blocking=True)
        return t.to(self.device)

    def _adjacency(self, EV, remember=True):
        """Device adjacency of a feed.  A ``DeviceAdjacency`` is used as is; a ``SparseEV`` is uploaded (CSR built)
        and remembered under a fingerprint of its CONTENT -- shape + CRC of the endpoint array, ~0.3 ms at C2 --
        so a caller that re-feeds the same edges (get_cost's probe loop) pays once while one that refills the
        array in place gets the new graph, as TF re-reads every feed; a dense matrix is converted every time."""
        from .graphnn import DeviceAdjacency
        if isinstance(EV, DeviceAdjacency):
            return EV
        if not isinstance(EV, SparseEV):
            try:
                return DeviceAdjacency.from_sparse_ev(SparseEV.fromdense(EV), self.device)
            except ValueError as e:
                raise ValueError("feed for model['EV']: %s" % e)
        if not remember:     # a stream of fresh batches (BatchPrefetcher): nothing to recognise, skip the fingerprint
            return DeviceAdjacency.from_sparse_ev(EV, self.device)
        uv = np.ascontiguousarray(EV.uv)
        key = (tuple(EV.shape), uv.shape, zlib.crc32(uv.view(np.uint8).reshape(-1)))
        cache = self._adj_cache
        if getattr(cache, "key", None) == key:
            return cache.adj
        adj = DeviceAdjacency.from_sparse_ev(EV, self.device)
        cache.key, cache.adj = key, adj
        return adj

    # ------------------------------------------------------------------ forward
    def prepare(self, feed, pinned=False, remember_adjacency=True):
        """Validates a feed_dict and makes the batch resident in HBM (adjacency in index/CSR form,
        (W,C) pairs, labels, segment offsets).  The returned DeviceBatch can be run many times.
        ``pinned``: stage through pinned host memory with non-blocking copies on the current stream
        (used by parallel.BatchPrefetcher on its side stream).  ``remember_adjacency=False`` skips the content fingerprint under
        which the uploaded adjacency is remembered (_adjacency): a stream of fresh batches never repeats one."""
        m = self.model
        adj = self._adjacency(feed[m["EV"]], remember=remember_adjacency)
        M, N = adj.shape
        W = np.asarray(feed[m["W"]], dtype=np.float32).reshape(-1)
        C = np.asarray(feed[m["C"]], dtype=np.float32).reshape(-1)
        if W.shape[0] != M or C.shape[0] != M:
            raise ValueError("W and C must have one row per edge (%d), got %d and %d" % (M, W.shape[0], C.shape[0]))
        marks = self._route_marks(feed, M)
        n_edges = np.asarray(feed[m["n_edges"]]).astype(np.int64).reshape(-1)
        n_vertices = np.asarray(feed[m["n_vertices"]]).astype(np.int64).reshape(-1)
        B = n_vertices.shape[0]
        labels = self._f32(np.asarray(feed[m["route_exists"]]).reshape(-1), pinned)
        if n_edges.shape[0] != B or labels.shape[0] != B:
            raise ValueError("route_exists, n_vertices and n_edges must have one entry per problem")
        if int(n_edges.sum()) != M:
            raise ValueError("sum(n_edges)=%d does not match the %d rows of EV" % (int(n_edges.sum()), M))
        if int(n_vertices.sum()) != N:
            raise ValueError("sum(n_vertices)=%d does not match the %d columns of EV" % (int(n_vertices.sum()), N))
        b = DeviceBatch()
        b.adj, b.M, b.N, b.B = adj, M, N, B
        b.T = int(feed[m["time_steps"]])
        b.WC = self._f32(np.stack([W, C], axis=1), pinned)
        b.labels = labels
        b.seg = torch.from_numpy(np.concatenate([[0], np.cumsum(n_edges)]).astype(np.int32)).to(self.device)
        b.n_vertices, b.n_edges = n_vertices, n_edges   # host int64, as DeviceDataset.batch leaves them
        if marks is not None:
            b.route_edges = self._f32(marks, pinned)
        return b

    def _route_marks(self, feed, M):
        """The feed of model['route_edges'] as a float32 host array of M zeros and ones, or None when the network has no
        route head or the feed no marks."""
        m = self.model
        if not getattr(m, "route_head", False) or m["route_edges"] not in feed:
            return None
        marks = np.array(feed[m["route_edges"]], dtype=np.float32).reshape(-1)    # (a copy: never the caller's memory)
        if marks.shape[0] != M:
            raise ValueError("feed for model['route_edges']: one mark per edge (%d), got %d" % (M, marks.shape[0]))
        if not np.all((marks == 0) | (marks == 1)):
            raise ValueError("feed for model['route_edges']: the marks are 0 or 1")
        return marks

    def mark_routes(self, batch, tours):
        """The marks of a resident DeviceBatch from its instances' tours, by tspgnn_route_edge_marks (route_head.py):
        ``tours`` a list of one sequence of local vertex ids per instance, or the tuple (int32 array, offsets[B + 1]).  Sets
        ``batch.route_edges`` (refilled in place when the batch already has them) and returns n_missing, the tour pairs
        per instance that are no edge of its graph.  ValueError naming the instance for a tour that is no permutation."""
        self._require_gpu("mark_routes")
        return RH.mark_routes(batch, tours)

    def _has_marks(self, feed):
        if isinstance(feed, DeviceBatch):
            return getattr(feed, "route_edges", None) is not None
        return self.model["route_edges"] in feed

    def _require_marks(self, feed, what):
        """A route-head network trains on marks: ``what`` without them is refused, naming the placeholder."""
        if getattr(self.model, "route_head", False) and not self._has_marks(feed):
            raise ValueError("%s of a route-head network: You must feed a value for placeholder route_edges "
                             "(model['route_edges']: route_edge_marks_host, or Session.mark_routes on a resident batch)"
                             % what)

    def forward(self, feed, global_stats=False):
        """Runs model.py:33-157 on the device; returns a dict of device tensors.  Rank-local by default, like the
        reference's inference path (no cross-process coupling: ranks may evaluate different numbers of batches, as
        binary_search.get_cost does).  ``global_stats=True`` is a COLLECTIVE call: every rank of a data-parallel
        session must make it, and loss / acc / TP / FP / TN / FN become those of the global batch (8 floats, one
        all-reduce)."""
        b = feed if isinstance(feed, DeviceBatch) else self.prepare(feed)
        out = self.forward_device(b)
        if global_stats and self.world_size > 1:
            self._reduce_stats_only(out["stats"], b.B)
        return out

    def forward_device(self, b):
        self._require_gpu("a forward pass")
        m, d = self.model, self.model.d
        st = _lib.current_stream()
        E0 = m.edge_init_MLP(b.WC)                                            # model.py:43
        V0 = torch.empty((b.N, d), dtype=torch.float32, device=self.device)  # model.py:48-51
        _lib.call("tspgnn_tile_rows_f32", _lib.ptr(self.store.view("V_init")), 1.0 / math.sqrt(float(d)),
                  _lib.ptr(V0), b.N, d, st)
        last = m["gnn"]({"EV": b.adj}, {"V": V0, "E": E0}, b.T)               # model.py:118-122
        Eh = to_f32(last["E"].h)                                              # (bf16 storage: widened once)
        arith = m["gnn"].active_arith()
        heads = [m.E_vote_MLP] + ([m.E_route_MLP] if m.route_head else [])    # (the route head takes the vote head's path)
        votes = [(h.forward_split(Eh, arith) if arith else h(Eh)).view(-1) for h in heads]       # model.py:128
        if arith == "h2" and not m["gnn"].check_h2_weights():     # (a head's packing vetoed f16x2: bf16x3)
            votes = [h.forward_split(Eh, m["gnn"].active_arith()).view(-1) for h in heads]
        vote = votes[0]
        logits = torch.empty(b.B, dtype=torch.float32, device=self.device)
        _lib.call("tspgnn_segment_mean_f32", _lib.ptr(vote), _lib.ptr(b.seg), _lib.ptr(logits), b.B, st)
        pred = torch.empty(b.B, dtype=torch.float32, device=self.device)
        stats = torch.empty(6, dtype=torch.float32, device=self.device)
        _lib.call("tspgnn_bce_metrics_f32", _lib.ptr(logits), _lib.ptr(b.labels), _lib.ptr(pred), _lib.ptr(stats),
                  b.B, st)
        out = {"last_states": last, "E_vote": vote, "logits": logits, "predictions": pred, "stats": stats,
               "range_guard": self.store.h2_guard()}
        if m.route_head:
            out["E_route"] = votes[1]
            marks = getattr(b, "route_edges", None)
            if marks is not None and b.M:
                out["route_stats"] = RH.edge_bce(votes[1], marks, b.seg, b.B, m.route_pos_weight, 0.0, False)[1]
        return out

    # ---- f16x2 range guard (GraphNN.active_arith): the default arithmetic's fp16 pieces overflow where the reference's
    # fp32 does not.  Weights are vetted when they are packed; an ACTIVATION that leaves the range sets bit 0 of the
    # guard word on the device, which every synchronous entry point (run) reads next to the values it fetches anyway
    # and answers by re-running the batch on bf16x3.  forward() / forward_device() / capture_forward() return device
    # tensors without synchronising: their callers get the word as out["range_guard"] and range_exceeded().
    def range_exceeded(self, clear=True):
        """True if an f16x2 launch since the last call flagged an operand outside the fp16 range (synchronises)."""
        if self.device.type != "cuda":
            return False
        guard = self.store.guard
        words = guard.peek()
        if words.status:                    # tspgnn_mp_loop_h2 gave up waiting: its workgroups were not all resident
            guard.clear_status()
            raise RuntimeError("tspgnn_mp_loop_h2: a wait inside the one-launch loop timed out (status %d); the launch's "
                               "outputs are invalid -- set TSPGNN_LOOP=0 to run the stepwise launches" % words.status)
        if words.activation:                # bit 0: an operand beyond fp16's largest value; bit 1: a gate row whose spread
            self.last_range_bits = words.activation   # is below the absolute error of its operands' fp16 pieces (h2_tile.h)
            if clear:
                guard.clear_flags()
        return bool(words.activation)

    def _on_bf16x3_if_flagged(self, do, then=lambda out: out):
        """``then(do())``; if do() raised the range flags (one look: range_exceeded), do() again and then() with f16x2 forced
        off -- this batch on bf16x3, which has fp32's range."""
        out = do()
        if not self.range_exceeded():
            return then(out)
        with self.model["gnn"].forced_off_h2():
            return then(do())

    def capture_forward(self, batch, epilogue=None):
        """Captures one forward pass over a resident batch into a HIP graph (hipStreamBeginCapture via
        torch.cuda.CUDAGraph: every libtspgnn launch goes to torch's current stream, so the capture sees
        all of them) and returns ``replay() -> outputs``.  The T-step loop is ~200 launches of 5-90 us
        kernels; replaying the graph removes the per-launch host cost.  The captured graph reads the
        packed weights that were current at capture time: re-capture after the variables change.
        ``epilogue(outputs)``, if given, enqueues more work on the current stream after the forward: it is
        captured into the same graph (the warm-up passes do not run it) -- get_costs' bracket update."""
        b = batch if isinstance(batch, DeviceBatch) else self.prepare(batch)
        # warm-up: builds packed-weight caches (and vets their range) outside the capture; a batch whose activations leave
        # the f16x2 range is warmed up again and captured on bf16x3
        return self._on_bf16x3_if_flagged(lambda: self.forward_device(b), lambda _: self._capture_forward(b, epilogue))

    def _capture_forward(self, b, epilogue):
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.forward_device(b)
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(graph):
            out = self.forward_device(b)
            if epilogue is not None:
                epilogue(out)
        version = self.store.version

        def replay():
            if self.store.version != version:
                raise RuntimeError("variables changed since capture_forward(): capture again")
            graph.replay()
            return out
        replay.graph = graph
        replay.batch = b    # the graph reads THIS batch's device buffers on every replay: they live as long as the closure does
        replay.range_exceeded = self.range_exceeded   # (synchronising) did a replay leave the f16x2 range? see run()
        return replay

    # ------------------------------------------------------------------ run
    def run(self, fetches, feed_dict=None):
        single = not isinstance(fetches, (list, tuple))
        flist = [fetches] if single else list(fetches)
        for f in flist:
            if isinstance(f, _InitOp):
                self.store.initialize(seed=f.seed)
                self._reset_optimizer_slots()   # tf.global_variables_initializer also resets <var>/Adam, beta powers
        names = [f.name for f in flist if isinstance(f, Fetch) and not isinstance(f, _InitOp)]
        out = None
        if names:
            if feed_dict is None:
                raise ValueError("these fetches depend on placeholders: feed_dict is required")
            missing = [k for k in ("EV", "W", "C", "time_steps", "route_exists", "n_vertices", "n_edges")
                       if self.model[k] not in feed_dict]
            if missing:
                raise ValueError("You must feed a value for placeholder(s) %s" % ", ".join(missing))
            if any(n in ROUTE_STAT_FETCHES for n in names):
                self._require_marks(feed_dict, "fetching " + ", ".join(n for n in names if n in ROUTE_STAT_FETCHES))
            if "train_step" in names:
                out = self.train_step(feed_dict)   # (looks after the f16x2 range flag itself)
            else:
                # a statistic of the batch is a statistic of the GLOBAL batch in a data-parallel session (collective:
                # every rank fetches it, as run_batch does); predictions / last_states alone stay rank-local
                gs = any(n in STAT_FETCHES for n in names)
                out = self._on_bf16x3_if_flagged(lambda: self.forward(feed_dict, global_stats=gs))
        results = []
        stats = None
        for f in flist:
            if isinstance(f, _InitOp) or f.name == "train_step":
                results.append(None)
                continue
            if stats is None:
                stats = out["stats"].cpu().numpy()
            if f.name == "predictions":
                results.append(out["predictions"].cpu().numpy())
            elif f.name == "E_route":
                results.append(out["E_route"].cpu().numpy())
            elif f.name in ROUTE_STAT_FETCHES:     # (of the local batch, in a data-parallel session too)
                results.append(np.float32(out["route_stats"].cpu().numpy()[ROUTE_STAT_FETCHES.index(f.name)]))
            elif f.name == "last_states":
                results.append({v: LSTMStateTuple(c=s.c.cpu().numpy(), h=s.h.to(torch.float32).cpu().numpy())
                                for v, s in out["last_states"].items()})
            else:
                idx = {"loss": 0, "acc": 1, "TP": 2, "FP": 3, "TN": 4, "FN": 5}[f.name]
                results.append(np.float32(stats[idx]))
        return results[0] if single else results

    # ------------------------------------------------------------------ training (model.py:160-167)
    def loss_and_grads(self, feed, keep_tape=False):
        """Forward + backward of ``loss`` (the L2 term is added by the optimiser kernel).  Leaves the
        gradient of the local mean loss in ``store.grad``; returns the forward outputs (``keep_tape``: plus the
        message passing's tape under "tape", for inspection -- it holds every step's states)."""
        self._require_marks(feed, "the gradient")
        self._require_gpu("a training step")
        m, d, st = self.model, self.model.d, _lib.current_stream()
        m["gnn"].check_training()     # (a network that does not train is refused before the gradients are zeroed)
        b = feed if isinstance(feed, DeviceBatch) else self.prepare(feed)
        store = self.store
        store.zero_grad()
        f32 = dict(dtype=torch.float32, device=self.device)
        E0 = m.edge_init_MLP(b.WC)
        V0 = torch.empty((b.N, d), **f32)
        _lib.call("tspgnn_tile_rows_f32", _lib.ptr(store.view("V_init")), 1.0 / math.sqrt(float(d)), _lib.ptr(V0),
                  b.N, d, st)
        last, tape = m["gnn"].forward_train({"EV": b.adj}, {"V": V0, "E": E0}, b.T)
        # vote head: three relu Dense(d) + Dense(1) (model.py:107-115,128), keeping the hidden activations
        mv = m.E_vote_MLP
        n_sq = mv.n_square
        EhT = to_f32(last["E"].h)                # (bf16 storage: widened once; the vote head is fp32)
        Y3 = torch.empty((b.M, d), **f32)
        acts = torch.empty((max(n_sq - 1, 1), b.M, d), **f32)
        mv.forward_saving(EhT, Y3, acts, acts.stride(0))
        head = mv.layer_names[-1]
        vote = torch.empty(b.M, **f32)
        _lib.call("tspgnn_rowdot_f32", _lib.ptr(Y3), _lib.ptr(store.view(head + "/kernel")),
                  _lib.ptr(store.view(head + "/bias")), _lib.ptr(vote), b.M, d, st)
        logits = torch.empty(b.B, **f32)
        _lib.call("tspgnn_segment_mean_f32", _lib.ptr(vote), _lib.ptr(b.seg), _lib.ptr(logits), b.B, st)
        pred = torch.empty(b.B, **f32)
        stats = torch.empty(6, **f32)
        _lib.call("tspgnn_bce_metrics_f32", _lib.ptr(logits), _lib.ptr(b.labels), _lib.ptr(pred), _lib.ptr(stats), b.B,
                  st)
        # ---- backward: loss -> votes -> vote head -> message passing -> initial embeddings
        dvote = torch.empty(b.M, **f32)
        _lib.call("tspgnn_vote_grad_f32", _lib.ptr(logits), _lib.ptr(b.labels), _lib.ptr(b.seg), _lib.ptr(dvote), b.B,
                  st)
        dY3 = torch.empty((b.M, d), **f32)
        _lib.call("tspgnn_rowdot_bwd_f32", _lib.ptr(dvote), _lib.ptr(store.view(head + "/kernel")), _lib.ptr(dY3), b.M,
                  d, st)
        ws = _lib.workspace("tspgnn_wcolsum_workspace_floats", b.M, d, device=self.device)
        _lib.call("tspgnn_wcolsum_f32", _lib.ptr(Y3), _lib.ptr(dvote), b.M, d, 1.0,
                  _lib.ptr(store.grad_view(head + "/kernel")), _lib.ptr(store.grad_view(head + "/bias")), _lib.ptr(ws),
                  st)
        dpre = torch.empty((n_sq, b.M, d), **f32)
        dEh = torch.empty((b.M, d), **f32)
        mv.backward_data(dY3, acts, acts.stride(0), Y3, dpre, dpre.stride(0), dEh, accumulate=False)
        mv.backward_weights([EhT] + [acts[l] for l in range(n_sq - 1)], [dpre[l] for l in range(n_sq)], b.M)
        route = self._route_head_grads(b, EhT, dEh) if m.route_head else None
        d0 = m["gnn"].backward(tape, {"E": (dEh, None)})
        dE0, dV0 = d0["E"][0], d0["V"][0]
        mi = m.edge_init_MLP
        ws = _lib.workspace("tspgnn_einit_bwd_workspace_floats", b.M, d, device=self.device)
        _lib.call("tspgnn_einit_bwd_f32", _lib.ptr(b.WC), _lib.ptr(mi.wb()), _lib.ptr(dE0),
                  _lib.ptr(store.grad_span(mi.layer_names[0] + "/kernel", mi.layer_names[-1] + "/bias")), _lib.ptr(ws),
                  b.M, d, st)
        if dV0 is not None:   # None: zero message-passing steps, the loss does not see V_init
            ws = _lib.workspace("tspgnn_wcolsum_workspace_floats", b.N, d, device=self.device)
            _lib.call("tspgnn_wcolsum_f32", _lib.ptr(dV0), None, b.N, d, 1.0 / math.sqrt(float(d)),
                      _lib.ptr(store.grad_view("V_init")), None, _lib.ptr(ws), st)
        out = {"last_states": last, "E_vote": vote, "logits": logits, "predictions": pred, "stats": stats, "batch": b}
        if route is not None:
            out["E_route"], out["route_stats"] = route
        if keep_tape:
            out["tape"] = tape
        return out

    def _route_head_grads(self, b, EhT, dEh):
        """The route head's part of loss_and_grads, along the lines the vote head takes: its forward on the final edge
        states keeping the hidden activations, the per-edge cross entropy against ``b.route_edges`` with the gradient
        scaled by the network's route_loss weight (tspgnn_edge_bce_f32), the head's weight gradients, and its data gradient
        ADDED to ``dEh`` -- so the message passing's backward sees d(loss + route_loss_weight * route_loss) / d E.h.
        -> (E_route logits [M], route_stats [6]: route_loss, route_acc, TP, FP, TN, FN of this batch)."""
        m, d, st, store = self.model, self.model.d, _lib.current_stream(), self.store
        f32 = dict(dtype=torch.float32, device=self.device)
        mr = m.E_route_MLP
        n_sq = mr.n_square
        Y3 = torch.empty((b.M, d), **f32)
        acts = torch.empty((max(n_sq - 1, 1), b.M, d), **f32)
        mr.forward_saving(EhT, Y3, acts, acts.stride(0))
        head = mr.layer_names[-1]
        logit = torch.empty(b.M, **f32)
        _lib.call("tspgnn_rowdot_f32", _lib.ptr(Y3), _lib.ptr(store.view(head + "/kernel")),
                  _lib.ptr(store.view(head + "/bias")), _lib.ptr(logit), b.M, d, st)
        dlogit, stats = RH.edge_bce(logit, b.route_edges, b.seg, b.B, m.route_pos_weight, m.route_loss_weight, True)
        dY3 = torch.empty((b.M, d), **f32)
        _lib.call("tspgnn_rowdot_bwd_f32", _lib.ptr(dlogit), _lib.ptr(store.view(head + "/kernel")), _lib.ptr(dY3), b.M,
                  d, st)
        ws = _lib.workspace("tspgnn_wcolsum_workspace_floats", b.M, d, device=self.device)
        _lib.call("tspgnn_wcolsum_f32", _lib.ptr(Y3), _lib.ptr(dlogit), b.M, d, 1.0,
                  _lib.ptr(store.grad_view(head + "/kernel")), _lib.ptr(store.grad_view(head + "/bias")), _lib.ptr(ws),
                  st)
        dpre = torch.empty((n_sq, b.M, d), **f32)
        mr.backward_data(dY3, acts, acts.stride(0), Y3, dpre, dpre.stride(0), dEh, accumulate=True)
        mr.backward_weights([EhT] + [acts[l] for l in range(n_sq - 1)], [dpre[l] for l in range(n_sq)], b.M)
        return logit, stats

    # The data-parallel step.  The loss is a mean over the GLOBAL batch (model.py:157), so rank r's
    # gradient of its local mean counts with weight B_r / B.  Everything that must cross ranks rides in ONE bucket:
    #   bucket = [ B_r * grad_r | B_r, B_r*loss_r, B_r*acc_r, TP_r, FP_r, TN_r, FN_r, guard bits 0, 1, 2 ]  (VariableStore.bucket)
    # one all-reduce(sum) of it (RCCL over xGMI with the 'nccl' backend; 462 KB at d=64), then every rank divides by the
    # reduced B on the device: no host round trip, so the two HIP graphs of capture_train_step run back to back around
    # the collective.  The L2 term, the clip by the GLOBAL norm and Adam follow on the reduced gradient, identically
    # on every rank (model.py:163-167).  Tensor ops only (device-agnostic): the gloo tests run this on CPU.
    def _pack_bucket(self, local_batch, stats, with_grad):
        store = self.store
        if store.grad is None:
            store.zero_grad()
        nb = float(local_batch)
        n = store.theta.numel()
        tail = store.bucket[n:]
        if self.device.type == "cuda":     # one launch (tspgnn_bucket_pack_f32): no at::native node in the captured step
            _lib.call("tspgnn_bucket_pack_f32", _lib.ptr(store.bucket), n, 1 if with_grad else 0, nb, _lib.ptr(stats),
                      store.guard.flag_ptr(), _lib.current_stream())
            return tail
        # device="cpu" (plumbing: the gloo tests): the same arithmetic as tensor ops
        if with_grad:
            store.grad.mul_(nb)
        return self._fill_tail(tail, nb, stats)

    def _fill_tail(self, tail, nb, stats):
        """The bucket's tail of a rank (or a micro-batch) of ``nb`` graphs, as bucket_pack_kernel writes it: tensor ops."""
        tail.zero_()
        tail[0:1].fill_(nb)
        if stats is not None:
            tail[1:3].copy_(stats[0:2])
            tail[1:3].mul_(nb)
            tail[3:7].copy_(stats[2:6])
        self.store.guard.flags_to_bucket(tail)   # one slot per bit
        return tail

    def _unpack_bucket(self, stats, with_grad):
        store = self.store
        n = store.theta.numel()
        if self.device.type == "cuda":
            _lib.call("tspgnn_bucket_unpack_f32", _lib.ptr(store.bucket), n, 1 if with_grad else 0, _lib.ptr(stats),
                      store.guard.flag_ptr(), _lib.current_stream())
            return
        tail = store.bucket[n:]
        inv = torch.reciprocal(tail[0:1])
        if with_grad:
            store.grad.mul_(inv)
        if stats is not None:
            stats[0:2].copy_(tail[1:3] * inv)
            stats[2:6].copy_(tail[3:7])
        store.guard.flags_from_bucket(tail)

    def allreduce_grads(self, local_batch, stats=None):
        """One all-reduce of [gradient | batch size, statistics]; afterwards ``store.grad`` holds the gradient of
        the global mean loss and ``stats`` (the 6-vector loss, acc, TP, FP, TN, FN of bce_metrics; optional) the
        statistics of the global batch.  No-op with a single rank."""
        if self.world_size == 1:
            return
        import torch.distributed as dist
        self._pack_bucket(local_batch, stats, True)
        dist.all_reduce(self.store.bucket, group=self.process_group)
        self._unpack_bucket(stats, True)

    def _reduce_stats_only(self, stats, local_batch):
        import torch.distributed as dist
        tail = self._pack_bucket(local_batch, stats, False)
        dist.all_reduce(tail, group=self.process_group)
        self._unpack_bucket(stats, False)

    # Gradient accumulation: a micro-batch is a rank that runs later.  Its gradient and statistics enter a second bucket
    # (VariableStore.accum_bucket) with the weights _pack_bucket gives a rank; the sum is handed to ``store.bucket``,
    # all-reduced ONCE when there are ranks, and unpacked like any reduced bucket.
    def accumulate_grads(self, local_batch, stats=None, first=False):
        """Folds ``store.grad`` -- the gradient of the mean loss of a micro-batch of ``local_batch`` graphs -- and its
        tail (batch size, ``stats``, guard bits) into the accumulation bucket: accum = B_k * [grad | ...] when ``first``
        (whatever the buffer held is gone), accum += B_k * [grad | ...] otherwise.  ``store.grad`` is not modified.  The
        product and the sum are rounded separately, on the GPU (tspgnn_bucket_accumulate_f32) as in the tensor ops of a
        ``device='cpu'`` session."""
        store = self.store
        if store.grad is None:
            store.zero_grad()
        nb = float(local_batch)
        n = store.theta.numel()
        accum = store.accum_bucket()
        if self.device.type == "cuda":
            _lib.call("tspgnn_bucket_accumulate_f32", _lib.ptr(accum), _lib.ptr(store.grad), n, 1 if first else 0, nb,
                      _lib.ptr(stats), store.guard.flag_ptr(), _lib.current_stream())
            return
        term = torch.empty_like(accum)
        torch.mul(store.grad, nb, out=term[:n])
        self._fill_tail(term[n:], nb, stats)
        if first:
            accum.copy_(term)
        else:
            accum.add_(term)

    def reduce_accumulated(self, stats=None):
        """Finishes what accumulate_grads summed: the accumulated bucket becomes ``store.bucket``, ONE all-reduce follows
        when there are ranks, then the unpack -- always, also with one rank: ``store.grad`` holds the gradient of the mean
        loss over every micro-batch (of every rank), ``stats`` (optional 6-vector) the statistics of their union, and the
        guard word is rebuilt from the summed flag slots."""
        store = self.store
        if store.grad is None:
            store.zero_grad()
        store.bucket.copy_(store.accum_bucket())
        if self.world_size > 1:
            import torch.distributed as dist
            dist.all_reduce(store.bucket, group=self.process_group)
        self._unpack_bucket(stats, True)

    def allreduce_host_sums(self, values):
        """Sum of a small float64 host vector over the ranks (run_batch's label / prediction means)."""
        v = np.asarray(values, dtype=np.float64)
        if self.world_size == 1:
            return v
        import torch.distributed as dist
        t = torch.from_numpy(v.copy()).to(self.device)
        dist.all_reduce(t, group=self.process_group)
        return t.cpu().numpy()

    def broadcast_variables(self, src=0):
        """Replicas start identical: theta AND the optimiser slots (m, v, step counter) from rank ``src`` to every
        rank.  Every rank issues the same four broadcasts whether or not it already holds optimiser state (a
        checkpoint restored on rank 0 only creates the slots there), so the collective sequence never depends on
        the rank."""
        if self.world_size == 1:
            self._synced_assignments = self.store.assignments
            return
        import torch.distributed as dist
        self._ensure_adam()
        group_src = src if self.process_group is None else dist.get_global_rank(self.process_group, src)
        dist.broadcast(self.store.theta, src=group_src, group=self.process_group)
        for k in ("m", "v", "t"):
            dist.broadcast(self._adam[k], src=group_src, group=self.process_group)
        self._adam["step"] = int(self._adam["t"].item())   # host mirror (save_weights' beta powers)
        self.store.touch()
        self._replicas_synced = True
        self._synced_assignments = self.store.assignments

    def _sync_replicas_once(self):
        """Broadcast before the first training step and again after every outside assignment of the variables
        (initialiser, load_weights / store.load) -- those happen on every rank or on rank 0 only, and either way the
        replicas must leave this call identical.  Collective when it fires: assignments must be made (or not made)
        at the same points of the program on every rank, like the training steps themselves."""
        need = not self._replicas_synced or self._synced_assignments != self.store.assignments
        if self.world_size > 1:
            # the decision is made TOGETHER (one 1-int all-reduce): a restore on rank 0 only bumps rank 0's counter alone,
            # and a rank that broadcast while its peers went on to the gradient all-reduce would hang the job
            import torch.distributed as dist
            flag = torch.tensor([1 if need else 0], dtype=torch.int32, device=self.device)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=self.process_group)
            need = bool(int(flag.item()))
        if need:
            self.broadcast_variables(0)

    def apply_gradients(self):
        """g += 1e-10*theta; clip_by_global_norm(0.65); Adam(lr=2e-5) -- one fused pass over theta."""
        store = self.store
        self._ensure_adam()
        a = self._adam
        a["step"] += 1   # host mirror; the device counter a["t"] is what the kernel uses (graph-replayable)
        b1, b2, eps = 0.9, 0.999, 1e-8     # tf.train.AdamOptimizer defaults
        _lib.call("tspgnn_adam_clip_step_f32", _lib.ptr(store.theta), _lib.ptr(store.grad), _lib.ptr(a["m"]),
                  _lib.ptr(a["v"]), store.theta.numel(), L2NORM_SCALING, GLOBAL_NORM_CLIP, LEARNING_RATE, b1, b2, eps,
                  _lib.ptr(a["gnorm"]), _lib.ptr(a["ws"]), _lib.ptr(a["t"]),
                  store.guard.flag_ptr() if self.device.type == "cuda" else None, _lib.current_stream())
        store.touch()
        return a["gnorm"]

    def _ensure_adam(self):
        store = self.store
        if self._adam is None:
            self._adam = {"m": torch.zeros_like(store.theta), "v": torch.zeros_like(store.theta), "step": 0,
                          "gnorm": torch.zeros(1, dtype=torch.float32, device=self.device),
                          "t": torch.zeros(1, dtype=torch.int32, device=self.device),
                          "ws": _lib.workspace("tspgnn_adam_workspace_floats", device=self.device)}

    def _reset_optimizer_slots(self):
        """Adam's m, v and step counter back to zero, in place (captured graphs keep pointing at the same tensors)."""
        if self._adam is not None:
            for k in ("m", "v", "t", "gnorm"):
                self._adam[k].zero_()
            self._adam["step"] = 0
        self._replicas_synced = False

    def train_step(self, feed):
        """One ``sess.run(train_step)``: forward, backward, (all-reduce), L2 + clip + Adam.

        The guard word is this call's business, whoever the caller is: it is cleared first (a flag left behind by an
        earlier, unchecked forward() must not make the optimiser kernel skip this step -- and every later one), read
        once after the optimiser launch (one blocking 4-byte read per eager step), and a flagged step -- which the
        optimiser kernel skipped on the device -- is repeated: on bf16x3 when an f16x2 launch left its range (bits 0 / 1),
        after a broadcast of rank 0's variables when some rank's variables were assigned since the replicas were last
        made identical (bit 2).  In a data-parallel session the word every rank reads is the all-reduced one, so all ranks
        repeat together -- and the "do we need to re-synchronise?" question rides in the step's ONE all-reduce instead of
        a collective and a host round trip of its own before every step: the price is one wasted forward +
        backward in the step after a checkpoint restore.

        A route-head network needs its marks (model['route_edges'] in the feed, or ``route_edges`` on the DeviceBatch) and
        steps on loss + route_loss_weight * route_loss; ``out["route_stats"]`` are those of THIS rank's batch -- they do
        not ride in the all-reduced bucket, whose layout is unchanged."""
        self._require_marks(feed, "train_step")
        return self._guarded_step(lambda: self._train_step_once(feed))

    def _guarded_step(self, once):
        """train_step's guard and retry rules around ``once()``, one whole optimiser step (train_step: one batch;
        train_step_accumulated: every micro-batch of the step)."""
        on_gpu = self.device.type == "cuda"
        dp = self.world_size > 1
        if dp and not self._ever_synced:
            # the session's first training step: every rank is here for the first time, the broadcast needs no agreement
            self.broadcast_variables(0)
            self._ever_synced = True
        need = dp and (not self._replicas_synced or self._synced_assignments != self.store.assignments)
        h2 = on_gpu and self.model["gnn"].active_arith() == "h2"   # (only f16x2 launches raise bits 0 / 1)
        guard = self.store.guard
        if on_gpu:
            guard.arm(need)     # always: the optimiser kernel skips on a non-zero word
        out = once()
        act, resync = flag_bits(guard.take_flags()) if on_gpu and (h2 or dp) else (0, False)
        if resync:   # skipped everywhere: some replica had been assigned to.  Make them identical, then take the step.
            self._adam["step"] -= 1
            self.broadcast_variables(0)
            out = once()
            act = flag_bits(guard.take_flags())[0] if h2 else 0
        if act:
            self.last_range_bits = act
            self._adam["step"] -= 1     # (Adam skipped the update on the device: theta, m, v and t are untouched)
            with self.model["gnn"].forced_off_h2():
                out = once()
        return out

    def _train_step_once(self, feed):
        out = self.loss_and_grads(feed)
        self.allreduce_grads(out["batch"].B, out["stats"])
        out["global_norm"] = self.apply_gradients()
        return out

    def train_step_accumulated(self, feeds):
        """ONE optimiser step over the micro-batches ``feeds`` (a non-empty sequence of feeds or DeviceBatches; their
        time steps may differ): the step ``train_step`` would take on their union, shard after shard, so the batch of a
        step is not bounded by what one training tape holds.  Per micro-batch: forward + backward, then its gradient
        enters the accumulation bucket with weight B_k (accumulate_grads).  Then ONE all-reduce when there are ranks
        (their numbers of micro-batches may differ: it is the only collective), the division by the summed batch size,
        and L2 + clip + Adam once -- the variables, and with them every packed-weight copy, do not change in between.

        Returns the last micro-batch's outputs with ``stats`` those of the union (the global ones in a data-parallel
        session), ``global_norm`` the optimiser launch's, ``predictions`` the list of the micro-batches' prediction
        tensors and ``batches`` the list of their DeviceBatches.  train_step's guard rules hold for the WHOLE step: the
        word is armed once before the first micro-batch, read once after the optimiser launch, and a flagged (skipped)
        step is repeated from its first micro-batch.  With a route head the gradient of the route loss accumulates like the
        decision loss's (both are means over problems, so the B_k weights are right as they stand); ``route_stats`` and
        ``E_route`` are the LAST micro-batch's (of this rank)."""
        feeds = list(feeds)
        if not feeds:
            raise ValueError("train_step_accumulated: an optimiser step needs at least one micro-batch")
        for f in feeds:
            self._require_marks(f, "train_step_accumulated")
        self._require_gpu("a training step")
        batches = [f if isinstance(f, DeviceBatch) else self.prepare(f) for f in feeds]
        return self._guarded_step(lambda: self._accumulated_step_once(batches))

    def _accumulated_step_once(self, batches):
        predictions = []
        for k, b in enumerate(batches):
            out = self.loss_and_grads(b)
            self.accumulate_grads(b.B, out["stats"], first=(k == 0))
            predictions.append(out["predictions"])
        self.reduce_accumulated(out["stats"])
        out["global_norm"] = self.apply_gradients()
        out["predictions"], out["batches"] = predictions, batches
        return out

    def capture_train_step(self, batch, micro_batches=None):
        """HIP-graph replay of the training step on a resident batch: graph A = zero grads + forward +
        backward (+ re-packing of the weights, which change every step), then the gradient all-reduce
        (eager: RCCL), then graph B = L2 + clip + Adam with the step counter on the device.  ~600 kernel
        launches per step stop costing host time.  Returns ``replay() -> outputs``.

        ``micro_batches=K``: the same two graphs, and ``replay(refill=None)`` is ONE optimiser step over K micro-batches
        (train_step_accumulated's arithmetic): for k in range(K) ``refill(k)`` if given, graph A, the accumulate launch;
        then the accumulated bucket's hand-over, the all-reduce, the unpack and graph B.  ``refill(k)`` is where the
        caller writes micro-batch k into the captured batch's buffers -- ``ds.batch(ids_k, ..., out=batch)``, which
        refuses other shapes; without it the resident batch is taken K times (timing only).  ``out["stats"]`` are the
        union's; ``out["predictions"]`` are the last micro-batch's.  A route-head batch carries its marks
        (``batch.route_edges``; Session.mark_routes and DeviceDataset.batch(out=) refill them in place), and
        ``out["route_stats"]`` are the local batch's, with micro-batches the last one's."""
        if micro_batches is not None and int(micro_batches) < 1:
            raise ValueError("capture_train_step: micro_batches=%r must be at least 1" % (micro_batches,))
        b = batch if isinstance(batch, DeviceBatch) else self.prepare(batch)
        self._ensure_adam()
        self._sync_replicas_once()
        gnn, store, guard = self.model["gnn"], self.store, self.store.guard
        guard.clear_flags()                   # (a flag left by an earlier unchecked forward() is not this capture's)
        self.loss_and_grads(b)                # warm-up outside the capture (allocator, caches)
        torch.cuda.synchronize()
        # did the warm-up leave the f16x2 range?  Then the step is captured on bf16x3 (and stays there for these
        # variables).  Decided together in a data-parallel session: the ranks' batches differ, their graphs must not.
        bits = guard.peek().activation
        if self.world_size > 1:
            import torch.distributed as dist
            agreed = torch.tensor([bits], dtype=torch.int32, device=self.device)
            dist.all_reduce(agreed, op=dist.ReduceOp.MAX, group=self.process_group)
            bits = int(agreed.item())
        if bits and gnn.active_arith() == "h2":
            self.last_range_bits = bits
            guard.clear_flags()
            gnn.leave_h2()
            return self.capture_train_step(b, micro_batches)
        side = torch.cuda.Stream(device=self.device)
        ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        self.store.version += 1               # force every packed-weight copy to be rebuilt INSIDE graph A
        with torch.cuda.graph(ga, stream=side):
            out = self.loss_and_grads(b)
        with torch.cuda.graph(gb, stream=side):
            gnorm = self.apply_gradients()
        self._adam["step"] -= 1               # capture does not execute: undo the host mirror's increment
        out["global_norm"] = gnorm

        # f16x2 range guard under replay: the packings happen inside graph A, so the guard words are looked at LATE --
        # replay i looks at the words as replay i - LAG left them, through a pinned copy and an event recorded then (long
        # complete: no stall).  A FIXED lag, not "whenever the copy happens to have landed": the flag word rides in the
        # all-reduced bucket and the weights are replicated, so every rank of a data-parallel session sees the same words
        # at the same replay index and raises at the same index -- no rank is left alone in the next all-reduce.  Looking
        # late is safe: the weight word trips at half the fp16 range (Adam moves a weight by ~lr per step), and a flagged
        # step -- and every step after it, the flag stays up -- was skipped by the optimiser kernel on the device.
        LAG = 2
        ring = [torch.zeros(4, dtype=torch.int32).pin_memory() for _ in range(LAG + 1)]
        inflight = []                         # [(event, pinned words)] of the last LAG replays, oldest first
        count = [0]

        dead = [None]    # once the guard has fired this closure is finished: graph A holds the f16x2 kernels

        def look():      # before a replay enqueues anything: the words as replay i - LAG left them
            if dead[0] is not None:
                raise RuntimeError(dead[0])
            if len(inflight) >= LAG:
                ev, words = inflight.pop(0)
                ev.synchronize()
                seen = decode(words)
                act = seen.activation
                if act or seen.weight_over:
                    torch.cuda.synchronize()
                    self.last_range_bits = act
                    gnn.leave_h2()
                    guard.clear()
                    del inflight[:]
                    self._adam["step"] = int(self._adam["t"].item())   # the device counter did not count the skipped steps
                    if act:
                        why = ("an activation left the fp16 range of the f16x2 split (guard bits %d): that step and the "
                               "replays after it were skipped by the optimiser kernel, the variables are those of the "
                               "last clean step" % act)
                    else:
                        why = ("a weight passed half the fp16 range of the f16x2 packing: the steps so far WERE applied, "
                               "the next ones would not be safe")
                    dead[0] = ("f16x2 range exceeded during replayed training steps: %s.  This replay closure is finished "
                               "(its graph holds the f16x2 kernels): call capture_train_step() again -- it will run on "
                               "bf16x3 (bf16 storage: with the message MLPs' backward on the fp32 matrix instruction)" % why)
                    raise RuntimeError(dead[0])

        def done():      # after graph B: this replay's words start their way to the host, the host mirrors move on
            if gnn.training_packs_h2():
                words = ring[count[0] % (LAG + 1)]
                count[0] += 1
                words.copy_(guard.words, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                inflight.append((ev, words))
            self._adam["step"] += 1
            self.store.touch()
            return out

        if micro_batches is None:
            def replay():
                look()
                ga.replay()
                self.allreduce_grads(b.B, out["stats"])   # device-side only: no host sync between the two graphs
                gb.replay()
                return done()
        else:
            K = int(micro_batches)
            store.accum_bucket()

            def replay(refill=None):
                look()
                for k in range(K):
                    if refill is not None:
                        refill(k)         # micro-batch k into b's buffers, on this stream: graph A reads them next
                    ga.replay()
                    self.accumulate_grads(b.B, out["stats"], first=(k == 0))
                self.reduce_accumulated(out["stats"])
                gb.replay()
                return done()
        replay.graphs = (ga, gb)
        return replay
