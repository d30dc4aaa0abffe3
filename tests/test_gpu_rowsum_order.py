"""The CSR row-sum's summation order, bit for bit.

The order the kernels document (csr_rowsum_body in aggregate.hip, csr_rowsum_bf16_kernel in bf16.hip) and the one-launch
loops restate: a wavefront sums one vertex; LPR lanes cover one source row, so RPW = 64 / LPR lane groups work side by side;
group s starts from +0 and adds the rows k = s (mod RPW) of the vertex's list in ascending k, straight across the 64-edge
id batches; the groups are then folded by the xor butterfly (distance 1, 2, 4 ... RPW/2 in group units), every group adding
its partner's value, and group 0 stores.  A row outside the vertex's list never enters the sum, however the kernel
schedules its loads.

Every fp32 addition is one IEEE round-to-nearest-even operation, which NumPy's float32 arithmetic reproduces exactly, so
the comparison is on the bit patterns.  The one thing IEEE leaves open is the sign and payload of a NaN: both sides must
agree on WHERE the NaNs are, and every other element must have identical bits (which tells +0 from -0)."""
import numpy as np
import pytest
import torch

from tspgnn import _lib

pytestmark = pytest.mark.gpu

DEGREES = [0, 1, 3, 39, 63, 64, 65, 199]
M_ROWS = 1003            # source rows; the last three are special
ROW_NEG0, ROW_INF, ROW_NAN = M_ROWS - 3, M_ROWS - 2, M_ROWS - 1

_KEEP = []


def dev(a, device, dtype):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release_uploads():
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


def ragged_csr(rng):
    """Every degree of DEGREES in four flavours -- ordinary rows only, with the Inf row, with the NaN row, with the -0 row
    (and nothing else but -0 / +0 rows for the short ones) -- each list fenced on both sides by a two-entry "poison" vertex
    (NaN row, Inf row): a load that strays one or more entries past either end of a list fetches poison.  Returns rowptr,
    eid and the indices of the vertices whose own lists hold only finite rows."""
    poison = [ROW_NAN, ROW_INF]
    lists, finite = [list(poison)], []
    for flavour in ("plain", "inf", "nan", "neg0"):
        for deg in DEGREES:
            e = list(rng.randint(0, ROW_NEG0, deg))
            if deg and flavour == "inf":
                e[rng.randint(deg)] = ROW_INF
            if deg and flavour == "nan":
                e[rng.randint(deg)] = ROW_NAN
            if deg and flavour == "neg0":
                e = [ROW_NEG0] * deg if deg < 4 else e
                e[0] = e[-1] = ROW_NEG0
            if flavour in ("plain", "neg0") or deg == 0:
                finite.append(len(lists))
            lists.append(e)
            lists.append(list(poison))
    rowptr = np.zeros(len(lists) + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum([len(e) for e in lists])
    eid = np.array([x for e in lists for x in e], dtype=np.int32)
    assert (len(lists) % 4) != 0          # N is not a multiple of the 4 wavefronts of a workgroup
    return rowptr, eid, np.array(finite)


def source_rows(rng, d):
    """fp32 rows over ~24 binades (so a different order of additions gives different bits), exact +0 and -0 entries
    sprinkled in, one all -0 row, one +-Inf row, one NaN row."""
    X = (rng.randn(M_ROWS, d) * np.exp2(rng.randint(-12, 12, (M_ROWS, d)))).astype(np.float32)
    z = rng.rand(M_ROWS, d)
    X[z < 0.03] = 0.0
    X[z > 0.97] = -0.0
    X[ROW_NEG0] = -0.0
    X[ROW_INF] = np.where(np.arange(d) % 2 == 0, np.inf, -np.inf)
    X[ROW_NAN] = np.nan
    return X


def documented_order(rowptr, eid, X, rpw, w=None):
    """NumPy float32 restatement: per lane group ascending, then the butterfly.  `w` (optional, per list entry) scales
    the row first; with power-of-two weights the product is exact, so fmaf(w, x, acc) is the same single rounding."""
    N, d = rowptr.size - 1, X.shape[1]
    out = np.empty((N, d), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in range(N):
            acc = np.zeros((rpw, d), dtype=np.float32)          # +0
            for k in range(rowptr[v + 1] - rowptr[v]):          # 64 % rpw == 0: the id batches do not disturb k mod rpw
                row = X[eid[rowptr[v] + k]]
                if w is not None:
                    row = row * w[rowptr[v] + k]
                acc[k % rpw] = acc[k % rpw] + row
            off = 1
            while off < rpw:
                acc = acc + acc[np.arange(rpw) ^ off]
                off <<= 1
            out[v] = acc[0]
    assert out.dtype == np.float32
    return out


def assert_same_bits(got, ref, finite, view):
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), "NaNs in different places"
    assert np.isfinite(ref[finite]).all()                   # the restatement's own sums of finite rows are finite
    assert np.isfinite(got[finite]).all(), "a row outside a vertex's list reached its sum"
    g, r = got.view(view), ref.view(view)
    bad = (g != r) & ~rn
    assert not bad.any(), "%d elements differ, first at %s" % (bad.sum(), np.argwhere(bad)[0])


@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_rowsum_f32_bits_follow_the_documented_order(cuda_device, d):
    rng = np.random.RandomState(100 + d)
    rowptr, eid, finite = ragged_csr(rng)
    X = source_rows(rng, d)
    N = rowptr.size - 1
    out = torch.full((N, d), 7.0, dtype=torch.float32, device=cuda_device)
    _lib.call("tspgnn_csr_rowsum_f32", _lib.ptr(dev(rowptr, cuda_device, np.int32)), _lib.ptr(dev(eid, cuda_device, np.int32)),
              _lib.ptr(dev(X, cuda_device, np.float32)), _lib.ptr(out), N, M_ROWS, d, None)
    torch.cuda.synchronize()
    lpr = min(d // 4, 16)                                      # wider rows are split into column blocks of 16 lanes
    ref = documented_order(rowptr, eid, X, 64 // lpr)
    assert_same_bits(out.cpu().numpy(), ref, finite, np.uint32)


@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_spmm_pair_rowsum_half_has_the_same_bits(cuda_device, d):
    rng = np.random.RandomState(200 + d)
    rowptr, eid, finite = ragged_csr(rng)
    X = source_rows(rng, d)
    N = rowptr.size - 1
    uv = rng.randint(0, N, (M_ROWS, 2)).astype(np.int32)
    Xv = dev(rng.randn(N, d), cuda_device, np.float32)
    Ye = torch.empty((M_ROWS, d), dtype=torch.float32, device=cuda_device)
    out = torch.full((N, d), 7.0, dtype=torch.float32, device=cuda_device)
    _lib.call("tspgnn_spmm_pair_f32", _lib.ptr(dev(uv, cuda_device, np.int32)), _lib.ptr(Xv), _lib.ptr(Ye),
              _lib.ptr(dev(rowptr, cuda_device, np.int32)), _lib.ptr(dev(eid, cuda_device, np.int32)),
              _lib.ptr(dev(X, cuda_device, np.float32)), _lib.ptr(out), M_ROWS, N, d, None)
    torch.cuda.synchronize()
    lpr = min(d // 4, 16)
    assert_same_bits(out.cpu().numpy(), documented_order(rowptr, eid, X, 64 // lpr), finite, np.uint32)


@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_csr_spmm_valued_bits_with_exact_weights(cuda_device, d):
    rng = np.random.RandomState(300 + d)
    rowptr, eid, finite = ragged_csr(rng)
    X = source_rows(rng, d)
    N = rowptr.size - 1
    w = np.array([0.5, 1.0, 2.0, -1.0, -4.0], dtype=np.float32)[rng.randint(0, 5, eid.size)]
    out = torch.full((N, d), 7.0, dtype=torch.float32, device=cuda_device)
    _lib.call("tspgnn_csr_spmm_f32", _lib.ptr(dev(rowptr, cuda_device, np.int32)), _lib.ptr(dev(eid, cuda_device, np.int32)),
              _lib.ptr(dev(w, cuda_device, np.float32)), _lib.ptr(dev(X, cuda_device, np.float32)), _lib.ptr(out), N, M_ROWS, d,
              None)
    torch.cuda.synchronize()
    lpr = min(d // 4, 16)
    assert_same_bits(out.cpu().numpy(), documented_order(rowptr, eid, X, 64 // lpr, w), finite, np.uint32)


@pytest.mark.parametrize("d", [32, 64, 128, 256, 512])
def test_rowsum_bf16_bits_follow_the_documented_order(cuda_device, d):
    rng = np.random.RandomState(400 + d)
    rowptr, eid, finite = ragged_csr(rng)
    Xb = torch.from_numpy(source_rows(rng, d)).to(torch.bfloat16)       # the stored operand
    N = rowptr.size - 1
    xd = Xb.to(cuda_device)
    _KEEP.append(xd)
    out = torch.full((N, d), 7.0, dtype=torch.bfloat16, device=cuda_device)
    _lib.call("tspgnn_csr_rowsum_bf16", _lib.ptr(dev(rowptr, cuda_device, np.int32)), _lib.ptr(dev(eid, cuda_device, np.int32)),
              _lib.ptr(xd), _lib.ptr(out), N, M_ROWS, d, None)
    torch.cuda.synchronize()
    ref32 = documented_order(rowptr, eid, Xb.to(torch.float32).numpy(), 64 // (d // 8))   # fp32 accumulation ...
    ref = torch.from_numpy(ref32).to(torch.bfloat16)                                      # ... one final rounding (RNE)
    assert_same_bits(out.cpu().to(torch.float32).numpy(), ref.to(torch.float32).numpy(), finite, np.uint32)   # exact widening
