"""The device reader of .graph files (csrc/graph_parse.hip, graph_text.read_files, DeviceDataset.from_directory(reader=
'device')) against the host reader: the token parser against the host build of the same routine, the committed fixtures,
a ragged directory across tile and chunk borders, layout variants, one doctored file per status, and the round trips
through the device writer.  Every comparison is exact."""
import os
import random

import numpy as np
import pytest
import torch

import graph_parse_cases as cases
from conftest import GOLDEN
from tspgnn import _lib
from tspgnn.device_dataset import DeviceDataset
from tspgnn.graph_text import READ_STATUS, host_f64_parse, token_arrays
from tspgnn.instance_loader import random_instance, read_graph, write_graph

pytestmark = pytest.mark.gpu

FIXTURES = ("hand_n4", "binned_n6", "full_n7", "sparse_n12")
KW = dict(restarts=2, kicks=4, lb_iters=20)   # the labels' quality is not under test


def fixture(name):
    z = np.load(os.path.join(GOLDEN, "graph_%s.npz" % name))
    return str(z["text"]), z["Ma"], z["Mw"], z["route"]


def put(path, name, text):
    os.makedirs(str(path), exist_ok=True)
    with open(os.path.join(str(path), name), "wb") as f:
        f.write(text if isinstance(text, bytes) else text.encode("ascii"))


def same_dataset(got, want):
    assert np.array_equal(got.n, want.n) and np.array_equal(got.m, want.m)
    for name in ("_inst", "_uv", "_w", "_rowptr", "_eid", "_cost"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name


def equals_host_reader(path, dev, **kw):
    got = DeviceDataset.from_directory(str(path), device=dev, reader="device", **kw)
    same_dataset(got, DeviceDataset.from_directory(str(path), device=dev))
    return got


def graph_text(inst, tmp_path, **kw):
    Ma, Mw, tour = inst
    p = str(tmp_path / "one.graph")
    write_graph(Ma, Mw, p, route=tour, **kw)
    with open(p) as f:
        text = f.read()
    os.remove(p)
    return text


# ------------------------------------------------------------------------------------------------- 1. the tokens
@pytest.mark.parametrize("mode", [0, 1])
def test_f64_parse_matches_the_host_routine(cuda_device, mode):
    toks = cases.accepted() + [t for t, _ in cases.REFUSALS]
    want, want_status = host_f64_parse(toks, mode)
    assert np.array_equal(want[:len(cases.accepted())], cases.expected_bits())
    buf, off, length = token_arrays(toks)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda_device)
    d_buf, d_off, d_len = up(buf), up(off), up(length)
    d_bits = torch.full((len(toks) + 1,), 0x55, dtype=torch.int64, device=cuda_device)
    d_status = torch.full((len(toks) + 1,), 0x55, dtype=torch.uint8, device=cuda_device)
    _lib.call("tspgnn_f64_parse", _lib.ptr(d_buf), buf.size, _lib.ptr(d_off), _lib.ptr(d_len), len(toks), mode,
              _lib.ptr(d_bits), _lib.ptr(d_status), _lib.current_stream())
    bits, status = d_bits.cpu().numpy().view(np.uint64), d_status.cpu().numpy()
    assert bits[-1] == 0x55 and status[-1] == 0x55   # one thread per token, none beyond
    assert np.array_equal(status[:-1], want_status)
    wrong = np.flatnonzero(bits[:-1] != want)
    assert wrong.size == 0, [(toks[k], hex(int(bits[k])), hex(int(want[k]))) for k in wrong[:10]]
    _lib.call("tspgnn_f64_parse", None, 0, None, None, 0, mode, None, None, _lib.current_stream())   # count == 0: no-op


# ---------------------------------------------------------------------------------------------- 2. the fixtures
def test_committed_fixtures(cuda_device, tmp_path):
    for k, name in enumerate(FIXTURES):
        put(tmp_path, "%d.graph" % k, fixture(name)[0])
    got = equals_host_reader(tmp_path, cuda_device, keep_matrices=True)
    assert [int(n) for n in got.n] == [4, 6, 7, 12]
    (kept,) = got._matrices
    A, Mw, tours = kept.A.cpu().numpy(), kept.Mw.cpu().numpy(), kept.tours.cpu().numpy()
    for k, name in enumerate(FIXTURES):
        _, Ma, W, route = fixture(name)
        n, c0, t0 = Ma.shape[0], int(kept.c_off[k]), int(kept.t_off[k])
        assert np.array_equal(A[c0:c0 + n * n].reshape(n, n), (Ma + Ma.T) != 0) and not np.tril(Ma).any()
        assert np.array_equal(Mw[c0:c0 + n * n].reshape(n, n).view(np.uint64), W.view(np.uint64))
        assert np.array_equal(tours[t0:t0 + n], route)
    _, Ma, W, _ = fixture("binned_n6")
    assert (W[Ma == 0] != 0).any() and np.array_equal(W, np.round(W))   # integer weights, non-zero off the edge set


def test_kernels_at_odd_offsets_keep_to_their_rows(cuda_device):
    """Both launches called directly on two fixtures at byte offsets 3 and 14 mod 16, with sentinels around every output."""
    texts = [fixture(name)[0].encode("ascii") for name in ("sparse_n12", "hand_n4")]
    b0 = np.array([3, 3 + len(texts[0]) + 18], dtype=np.int64)
    assert b0[0] % 16 == 3 and b0[1] % 16 == 14
    size = np.array([len(t) for t in texts], dtype=np.int64)
    raw = np.full(int(b0[1] + size[1]) + 7, ord("1"), dtype=np.uint8)   # digits all around: a read outside shows
    for b, t in zip(b0, texts):
        raw[b:b + len(t)] = np.frombuffer(t, dtype=np.uint8)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda_device)
    d_text = up(raw)
    tab2 = np.ascontiguousarray(np.stack([b0, size], axis=1))
    d_info = torch.full((3, 8), -7, dtype=torch.int32, device=cuda_device)
    st = _lib.current_stream()
    _lib.call("tspgnn_graph_text_scan", tab2.ctypes.data, _lib.ptr(up(tab2)), _lib.ptr(d_text), raw.size, 2,
              _lib.ptr(d_info), st)
    info = d_info.cpu().numpy()
    assert (info[2] == -7).all() and info[:, 0].tolist()[:2] == [0, 0] and info[:2, 1].tolist() == [12, 4]
    assert info[:2, 2].tolist() == [12, 4] and info[1, 6] == int(np.count_nonzero(fixture("hand_n4")[1]))
    for row, t in zip(info[:2], texts):
        assert t[row[3] - 19:row[3]] == b"EDGE_DATA_SECTION:\n" and t[row[5] - 14:row[5]] == b"TOUR_SECTION:\n"
        assert t[row[4] - 21:row[4]] == b"EDGE_WEIGHT_SECTION:\n"
    pad = 5
    nc = np.array([12, 4], dtype=np.int64)
    c_off, t_off = np.array([pad, pad + 144 + pad]), np.array([pad, pad + 12 + pad])
    n_cells, n_tour = int(c_off[1] + 16 + pad), int(t_off[1] + 4 + pad)
    d_A = torch.full((n_cells,), 9, dtype=torch.uint8, device=cuda_device)
    d_Mw = torch.full((n_cells,), -3.0, dtype=torch.float64, device=cuda_device)
    d_tours = torch.full((n_tour,), -9, dtype=torch.int32, device=cuda_device)
    d_ms = torch.full((2, 3), -7, dtype=torch.int32, device=cuda_device)
    tab5 = np.ascontiguousarray(np.stack([b0, size, nc, c_off, t_off], axis=1))
    _lib.call("tspgnn_graph_text_parse", tab5.ctypes.data, _lib.ptr(up(tab5)), _lib.ptr(d_text), raw.size, 2, 12, n_cells,
              n_tour, _lib.ptr(d_A), _lib.ptr(d_Mw), _lib.ptr(d_tours), _lib.ptr(d_ms[0]), _lib.ptr(d_ms[1]), st)
    A, Mw, tours, ms = d_A.cpu().numpy(), d_Mw.cpu().numpy(), d_tours.cpu().numpy(), d_ms.cpu().numpy()
    assert ms[:, 2].tolist() == [-7, -7] and ms[1, :2].tolist() == [0, 0]
    inside_c, inside_t = np.zeros(n_cells, dtype=bool), np.zeros(n_tour, dtype=bool)
    for k, name in enumerate(("sparse_n12", "hand_n4")):
        _, Ma, W, route = fixture(name)
        n = Ma.shape[0]
        inside_c[c_off[k]:c_off[k] + n * n] = True
        inside_t[t_off[k]:t_off[k] + n] = True
        assert np.array_equal(A[c_off[k]:c_off[k] + n * n].reshape(n, n), (Ma + Ma.T) != 0)
        assert np.array_equal(Mw[c_off[k]:c_off[k] + n * n].reshape(n, n), W)
        assert np.array_equal(tours[t_off[k]:t_off[k] + n], route) and ms[0, k] == np.count_nonzero(Ma)
    assert (A[~inside_c] == 9).all() and (Mw[~inside_c] == -3.0).all() and (tours[~inside_t] == -9).all()


# ------------------------------------------------------------------------------------------ 3. a ragged directory
def test_ragged_directory_and_chunking(cuda_device, tmp_path):
    rng = np.random.RandomState(5)
    insts = [random_instance(4, rng), random_instance(5, rng, 0.6), random_instance(20, rng), random_instance(64, rng, 0.1),
             random_instance(256, rng, 0.5), random_instance(9, rng)]
    for k, (Ma, Mw, tour) in enumerate(insts):
        write_graph(Ma, Mw, str(tmp_path / ("%d.graph" % k)), route=tour)
    with open(str(tmp_path / "2.graph")) as f:
        text = f.read()
    weights = text[text.index("EDGE_WEIGHT_SECTION"):text.index("TOUR_SECTION")]
    assert len(weights) > 4096 and max(len(t) for t in weights.split()) >= 19   # above one tile, 17-digit weights
    with open(str(tmp_path / "4.graph")) as f:
        assert "\n100 " in f.read(2 ** 18)   # three-digit ids among the pair lines
    whole = equals_host_reader(tmp_path, cuda_device)
    same_dataset(equals_host_reader(tmp_path, cuda_device, text_bytes=1), whole)       # one file per chunk
    same_dataset(equals_host_reader(tmp_path, cuda_device, text_bytes=30000), whole)   # the small files together
    assert whole.read_times["bytes"] == sum(os.path.getsize(str(tmp_path / f)) for f in os.listdir(str(tmp_path)))
    b = whole.batch([0, 4, 2], time_steps=2)   # the read dataset serves batches
    assert b.n_vertices.tolist() == [4, 256, 20]


# --------------------------------------------------------------------------------------------- 4. layout variants
def test_layout_variants(cuda_device, tmp_path):
    rng = np.random.RandomState(6)
    text = graph_text(random_instance(5, rng, 0.7), tmp_path)
    head, rest = text.split("EDGE_WEIGHT_SECTION:\n")
    rows, tail = rest.split("TOUR_SECTION:\n")
    lines = rows.split("\n")
    pair = head.split("EDGE_DATA_SECTION:\n")[1].split("\n")[1]
    variants = {
        "crlf": text.replace("\n", "\r\n"),
        "tabs": text.replace(" ", "\t"),
        "no_final_newline": text[:-1],
        "ends_with_the_tour": text[:-len("EOF\n") - 1],
        "blank_lines": head + "EDGE_WEIGHT_SECTION:\n\n" + "\n\n \n".join(lines) + "\nTOUR_SECTION:\n" + tail,
        "extra_tokens": head + "EDGE_WEIGHT_SECTION:\n" + rows + "9.5 8.25 7\n" + "TOUR_SECTION:\n" + tail,
        "duplicated_pair": text.replace(pair + "\n", pair + "\n" + pair + "\n", 1),
        "one_weight_per_line": head + "EDGE_WEIGHT_SECTION:\n" + "\n".join(rows.split()) + "\nTOUR_SECTION:\n" + tail,
        "formfeed_and_vt": head + "EDGE_WEIGHT_SECTION:\n" + rows.replace(" ", "\x0b\x0c") + "TOUR_SECTION:\n" + tail,
    }
    assert variants["duplicated_pair"].count(pair + "\n") == 2
    base = tmp_path / "base"
    put(base, "0.graph", text)
    want = DeviceDataset.from_directory(str(base), device=cuda_device)
    for name, body in variants.items():
        put(tmp_path / name, "0.graph", body)
        same_dataset(equals_host_reader(tmp_path / name, cuda_device), want)
    put(tmp_path / "all", "a.graph", text)
    for name, body in variants.items():
        put(tmp_path / "all", "b_%s.graph" % name, body)
    assert len(equals_host_reader(tmp_path / "all", cuda_device)) == 1 + len(variants)


# --------------------------------------------------------------------------------------------- 5. the refusals
def test_one_doctored_file_per_status(cuda_device, tmp_path):
    rng = np.random.RandomState(7)
    inst = random_instance(5, rng, 1.0)
    text = graph_text(inst, tmp_path)
    good = graph_text(random_instance(6, rng), tmp_path)
    tour = " ".join(str(x) for x in inst[2])
    weight = repr(float(inst[1][0, 1]))
    swap = lambda a, b: (lambda t: (t.replace(a, b, 1), t.count(a))[0])
    doctored = [
        (3, swap("DIMENSION", "DIMENSIO")),
        (3, swap("DIMENSION: 5", "DIMENSION: 0")),
        (4, swap("TOUR_SECTION", "TOUR_SECTIO")),
        (4, swap("EDGE_WEIGHT_SECTION", "EDGE_WEIGHT_SECTIO")),
        (5, swap("\n0 1\n", "\n0 7\n")),
        (5, swap("\n0 1\n", "\n0\n")),
        (6, swap(weight, "abc")),
        (6, swap(weight + " ", "")),
        (7, swap("\n" + tour + "\n", "\n" + tour.replace(str(inst[2][2]), "9", 1) + "\n")),
        (8, lambda t: graph_text(random_instance(3, np.random.RandomState(8)), tmp_path)),
        (8, swap("DIMENSION: 5", "DIMENSION: 300")),
        (9, swap("\n0 1\n", "\n1 0\n")),
        (9, swap("\n0 1\n", "\n2 2\n")),
        (10, swap("\n" + tour + "\n", "\n" + tour[:tour.rindex(" ")] + "\n")),
        (10, swap("\n" + tour + "\n", "\n" + tour + " 0\n")),
        (11, swap(weight, "0.12345678901234567890")),
        (11, swap(weight, "0x1p-1")),
    ]
    assert sorted(set(c for c, _ in doctored)) == list(range(3, 12))
    for k, (code, change) in enumerate(doctored):
        d = tmp_path / ("case%d" % k)
        body = change(text)
        assert body != text
        put(d, "0.graph", good)
        put(d, "1_doctored.graph", body)
        put(d, "2.graph", good)
        with pytest.raises(ValueError) as err:
            DeviceDataset.from_directory(str(d), device=cuda_device, reader="device")
        message = str(err.value)
        assert "1_doctored.graph" in message and "status %d" % code in message and READ_STATUS[code] in message, message
        assert ("reader='host'" in message) == (code >= 8), message
        if code >= 9 and "DIMENSION: 300" not in body:
            read_graph(os.path.join(str(d), "1_doctored.graph"))   # the host reader does read it
    big = tmp_path / "big"
    put(big, "0.graph", b" " * ((1 << 24) + 1))
    with pytest.raises(ValueError, match="0.graph"):
        DeviceDataset.from_directory(str(big), device=cuda_device, reader="device")


# --------------------------------------------------------------------------------------------- 6, 7. round trips
def test_round_trip_through_the_device_writer(cuda_device, tmp_path):
    random.seed(3)
    np.random.seed(3)
    made = DeviceDataset.generate(8, 4, 24, conn_min=0.5, conn_max=1, device=cuda_device, seed=3, **KW)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    made.write_directory(a)
    back = equals_host_reader(a, cuda_device, keep_matrices=True)
    back.write_directory(b)
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(a)) == 8
    for name in os.listdir(a):
        with open(os.path.join(a, name), "rb") as fa, open(os.path.join(b, name), "rb") as fb:
            assert fa.read() == fb.read(), name
    # to_instances() of the read dataset: what read_graph gives per file, Ma as the 0/1 pattern
    files = [os.path.join(a, f) for f in sorted(os.listdir(a))]
    for (Ma, Mw, route), f in zip(back.to_instances(), files):
        hMa, hMw, hroute = read_graph(f)
        assert np.array_equal(Ma, np.asarray(hMa) != 0) and np.array_equal(Mw.view(np.uint64), hMw.view(np.uint64))
        assert [int(x) for x in route] == [int(x) for x in hroute]
    plain = DeviceDataset.from_directory(a, device=cuda_device, reader="device")
    assert plain._matrices is None and plain.tours is None
    with pytest.raises(RuntimeError):
        plain.to_instances()
