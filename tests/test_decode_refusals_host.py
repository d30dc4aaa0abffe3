"""Every refusal tspgnn/decode.py makes in Python, before its first call into the library: tours_from_votes,
vote_neighbors, edge_scores, beam_tours and decode_tours against a stub batch and a stub session.  The type of the
exception and the distinguishing words of its message, and for decode_tours the order in which the checks come.
(decode_tours' "guide only applies with polish=True" and "exclusive" cases: tests/test_guided_host.py.)  No GPU."""
import types

import numpy as np
import pytest
import torch

from tspgnn import decode


def _batch(sizes=(4, 5), carry=True):
    """A resident batch as decode.py sees it, on the CPU: complete graphs of `sizes` vertices, every tensor zero."""
    B, N, M = len(sizes), int(sum(sizes)), int(sum(n * (n - 1) // 2 for n in sizes))
    adj = types.SimpleNamespace(uv=torch.zeros((M, 2), dtype=torch.int32),
                                csr_t=(torch.zeros(N + 1, dtype=torch.int32), torch.zeros(2 * M, dtype=torch.int32)))
    b = types.SimpleNamespace(B=B, N=N, M=M, seg=torch.zeros(B + 1, dtype=torch.int32), adj=adj,
                              WC=torch.zeros((M, 2), dtype=torch.float32))
    if carry:
        b.n_vertices = np.asarray(sizes, dtype=np.int32)
    return b


class _Session:
    device = "cpu"

    def __init__(self):
        self.asked = []

    def _require_gpu(self, what):
        self.asked.append(what)


def _inst(n):
    return np.triu(np.ones((n, n)), 1), np.ones((n, n)), None


# the three launch wrappers: the dtype of the per-edge tensor, what the messages call it, the call with that tensor
WRAPPERS = {
    "tours_from_votes": (torch.float32, "vote", lambda b, x, **kw: decode.tours_from_votes(b, x, **kw)),
    "vote_neighbors": (torch.float32, "vote", lambda b, x, **kw: decode.vote_neighbors(b, x, 4, 4, **kw)),
    "beam_tours": (torch.int32, "score", lambda b, x, **kw: decode.beam_tours(b, x, 16, **kw)),
}
KIND = {torch.float32: "a float32", torch.int32: "an int32"}


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_launch_wrappers_refuse_a_bad_per_edge_tensor(name):
    dtype, word, call = WRAPPERS[name]
    b = _batch()
    tensor = "%s: %ss must be %s tensor on the batch's device" % (name, word, KIND[dtype])
    other = torch.float64 if dtype == torch.float32 else torch.int64
    for bad in (None, np.zeros(b.M, dtype=np.float32), [0.0] * b.M,          # not a tensor
                torch.zeros(b.M, dtype=other),                              # wrong dtype
                torch.zeros(b.M, dtype=torch.int32 if dtype == torch.float32 else torch.float32),
                torch.zeros(b.M, dtype=dtype, device="meta")):              # wrong device
        with pytest.raises(ValueError) as err:
            call(b, bad)
        assert str(err.value) == tensor
    for bad, got in ((torch.zeros(b.M + 1, dtype=dtype), b.M + 1),           # wrong length
                     (torch.zeros(b.M - 1, dtype=dtype), b.M - 1),
                     (torch.zeros((b.M, 2), dtype=dtype), 2 * b.M),
                     (torch.zeros(0, dtype=dtype), 0),
                     (torch.zeros(2 * b.M, dtype=dtype)[::2], b.M),          # not contiguous
                     (torch.zeros((b.M, 2), dtype=dtype)[:, 0], b.M)):
        with pytest.raises(ValueError) as err:
            call(b, bad)
        assert str(err.value) == "%s: one contiguous %s per edge (%d), got %d" % (name, word, b.M, got)


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_launch_wrappers_refuse_bad_vertex_counts(name):
    dtype, _, call = WRAPPERS[name]

    def refused(b, match, **kw):
        with pytest.raises(ValueError, match=match):
            call(b, torch.zeros(b.M, dtype=dtype), **kw)
        assert not hasattr(b, "_decode_vseg")

    refused(_batch(carry=False), "does not carry n_vertices; pass it")
    b = _batch()
    b.n_vertices = None
    refused(b, "does not carry n_vertices; pass it")
    for carry in (True, False):
        count_or_sum = "n_vertices must hold one entry per graph and sum to the batch's 9 vertices"
        refused(_batch(carry=carry), count_or_sum, n_vertices=[9])                   # wrong count
        refused(_batch(carry=carry), count_or_sum, n_vertices=[4, 4, 1])
        refused(_batch(carry=carry), count_or_sum, n_vertices=[4, 4])                # wrong sum
        refused(_batch(carry=carry), count_or_sum, n_vertices=[5, 5])
    refused(_batch((3, 5)), "instances of 3..5 vertices; the decoder takes 4 <= n <= 256")
    refused(_batch((4, 5)), "instances of 3..6 vertices; the decoder takes 4 <= n <= 256", n_vertices=[3, 6])
    refused(_batch((257, 4)), "instances of 4..257 vertices; the decoder takes 4 <= n <= 256")
    refused(_batch((4, 5)), "one entry per graph", n_vertices=[[4, 5], [0, 0]])      # flattened, then counted


def test_per_edge_tensor_comes_before_the_vertex_counts():
    b = _batch(carry=False)
    for name in sorted(WRAPPERS):
        with pytest.raises(ValueError, match="tensor on the batch's device"):
            WRAPPERS[name][2](b, None)


BAD_COUNTS = [(-1, 4), (4, -1), (-1, -1), (0, 0), (33, 0), (0, 33), (17, 16), (True, 1), (1, False), (2.5, 1), (4, 4.0),
              ("4", 0), (None, 4)]


def test_vote_neighbors_refuses_bad_counts_first():
    b = _batch()
    for kv, kn in BAD_COUNTS:
        with pytest.raises(ValueError) as err:
            decode.vote_neighbors(b, None, kv, kn)           # (the votes would be refused next)
        assert str(err.value) == ("vote_neighbors: k_vote, k_near: %r; the rows take k_vote >= 0 and k_near >= 0 with "
                                  "1 <= k_vote + k_near <= 32" % ((kv, kn),))
    for kv, kn in ((32, 0), (0, 32), (16, 16), (1, 0), (np.int64(3), np.int32(2))):
        with pytest.raises(ValueError, match="votes must be a float32 tensor"):
            decode.vote_neighbors(b, None, kv, kn)
    with pytest.raises(ValueError, match="votes must be a float32 tensor"):
        decode.vote_neighbors(b, None, 8)                    # k_near = 0


def test_guide_is_a_count_or_a_pair():
    assert decode._guide_counts(8, "w") == (8, 0) and decode._guide_counts(np.int64(32), "w") == (32, 0)
    assert decode._guide_counts((4, 3), "w") == (4, 3) and decode._guide_counts([0, 1], "w") == (0, 1)
    got = decode._guide_counts((np.int32(2), np.int64(5)), "w")
    assert got == (2, 5) and all(type(k) is int for k in got)
    for bad in (0, 33, -1, True, 2.5, "4", None, (4,), (4, 4, 4), (1, 2.0)) + tuple(BAD_COUNTS):
        with pytest.raises(ValueError) as err:
            decode._guide_counts(bad, "here: guide")
        assert str(err.value).startswith("here: guide: %r; the rows take" % (bad,))
        assert "1 <= k_vote + k_near <= %d" % decode.MAX_GUIDE in str(err.value)


def test_edge_scores_refuses_what_is_not_a_float32_tensor_on_a_gpu():
    for bad in (None, np.zeros(3, dtype=np.float32),                                  # not a tensor
                torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32),   # wrong dtype
                torch.zeros(3, dtype=torch.float32), torch.zeros(3, dtype=torch.float32, device="meta")):   # no GPU
        with pytest.raises(ValueError) as err:
            decode.edge_scores(bad)
        assert str(err.value) == "edge_scores: votes must be a float32 tensor on a GPU"


def test_beam_tours_refuses_select_then_beam_then_the_scores():
    b = _batch()
    good = torch.zeros(b.M, dtype=torch.int32)
    for select in ("best", "", None, 0, "Score"):
        with pytest.raises(ValueError) as err:
            decode.beam_tours(b, None, 0, select=select)
        assert str(err.value) == "beam_tours: select must be 'score' or 'cost', got %r" % (select,)
    for beam in (0, 1025, -1, 1 << 20):
        for select in ("score", "cost"):
            with pytest.raises(ValueError) as err:
                decode.beam_tours(b, None, beam, select)
            assert str(err.value) == "beam_tours: beam=%d; the decoder takes 1 <= beam <= 1024" % beam
    for beam in (1, 1024):
        with pytest.raises(ValueError, match="scores must be an int32 tensor"):
            decode.beam_tours(b, None, beam)
        with pytest.raises(ValueError, match="does not carry n_vertices"):
            decode.beam_tours(_batch(carry=False), good, beam)


# ------------------------------------------------------------------------------------------------------ decode_tours
def _decode(sess=None, instances=(4, 5), **kw):
    kw.setdefault("target_costs", [1.0] * len(instances))
    return decode.decode_tours(sess or _Session(), None, [_inst(n) for n in instances], 4, **kw)


def test_decode_tours_checks_the_guide_before_it_asks_for_a_gpu():
    sess = _Session()
    for kw, exc, match in ((dict(guide=4), TypeError, "guide only applies with polish=True"),
                           (dict(guide=4, polish=True, neighbors=8), ValueError, "exclusive"),
                           (dict(guide=4, polish=True, candidates=[None, None]), ValueError, "exclusive"),
                           (dict(guide=(0, 0), polish=True), ValueError, r"decode_tours: guide: \(0, 0\); the rows take"),
                           (dict(guide=33, polish=True), ValueError, "decode_tours: guide: 33; the rows take")):
        with pytest.raises(exc, match=match):
            _decode(sess, instances=(3, 257), beam=0, select="best", **kw)   # (everything later is wrong as well)
    assert sess.asked == []
    with pytest.raises(ValueError, match="instance 0 has 3 vertices"):
        _decode(sess, instances=(3, 257), polish=True, guide=(4, 4))
    assert sess.asked == ["decode_tours"]


def test_decode_tours_refusals_in_their_order():
    size = "decode_tours: instance %d has %d vertices; the decoder takes 4 <= n <= 256"
    only_beam = "decode_tours: select and workspace_bytes only apply with beam=K"
    select = "decode_tours: select must be 'score' or 'cost', got 'best'"
    beam = "decode_tours: beam=%d; the decoder takes 1 <= beam <= 1024"
    only_polish = "decode_tours: %s only apply with polish=True"
    count = "decode_tours: target_costs must hold one cost per instance"
    later = dict(kicks=2, restarts=3, target_costs=[1.0])     # refused by the last two checks
    for kw, exc, message in (
            # the sizes, in instance order, ahead of everything that follows
            (dict(instances=(3, 5), select="cost", **later), ValueError, size % (0, 3)),
            (dict(instances=(4, 257), beam=0, select="best", **later), ValueError, size % (1, 257)),
            (dict(instances=(257, 3), **later), ValueError, size % (0, 257)),
            # without a beam
            (dict(select="cost", **later), TypeError, only_beam),
            (dict(select="best", **later), TypeError, only_beam),
            (dict(workspace_bytes=1 << 20, **later), TypeError, only_beam),
            (dict(workspace_bytes=0), TypeError, only_beam),
            # with one: select, then the width
            (dict(beam=0, select="best", **later), ValueError, select),
            (dict(beam=16, select="best"), ValueError, select),
            (dict(beam=0, **later), ValueError, beam % 0),
            (dict(beam=1025, select="cost", workspace_bytes=1, **later), ValueError, beam % 1025),
            (dict(beam=-1), ValueError, beam % -1),
            # search settings without a polish, then the targets
            (dict(**later), TypeError, only_polish % "kicks, restarts"),
            (dict(beam=16, select="cost", neighbors=8, target_costs=[1.0]), TypeError, only_polish % "neighbors"),
            (dict(target_costs=[1.0]), ValueError, count),
            (dict(target_costs=[1.0, 2.0, 3.0], beam=1024), ValueError, count),
            (dict(target_costs=np.ones((3, 1)), polish=True, kicks=2), ValueError, count)):
        sess = _Session()
        with pytest.raises(exc) as err:
            _decode(sess, **kw)
        assert type(err.value) is exc and str(err.value) == message, kw
        assert sess.asked == ["decode_tours"]
