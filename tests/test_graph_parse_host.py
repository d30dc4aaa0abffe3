"""tspgnn_host_f64_parse (csrc/graph_parse.hip) against Python's float(token): the host build of the routine the device
reader of .graph files runs per weight, in both modes; the refusals; the table's generator; and the arguments
DeviceDataset.from_directory refuses before it needs a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import graph_parse_cases as cases
from tspgnn import _lib
from tspgnn.device_dataset import DeviceDataset
from tspgnn.graph_text import host_f64_parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", [0, 1])
def test_accepted_tokens_match_float(mode):
    toks = cases.accepted()
    assert len(toks) > 530000
    bits, status = host_f64_parse(toks, mode)
    bad = np.flatnonzero(status)
    assert bad.size == 0, [(toks[k], int(status[k])) for k in bad[:10]]
    want = cases.expected_bits()
    wrong = np.flatnonzero(bits != want)
    assert wrong.size == 0, [(toks[k], hex(int(bits[k])), hex(int(want[k]))) for k in wrong[:10]]


def test_case_list_has_what_it_names():
    toks = cases.accepted()
    assert all(len(t) <= 48 for t in toks)
    assert max(len(t.lstrip("+-0.").split("e")[0].replace(".", "")) for t in toks if t[-1].isdigit()) == 19
    want = cases.expected_bits()
    as_float = want.view(np.float64)
    assert np.isinf(as_float).any() and np.isnan(as_float).any() and (want == 1 << 63).any()   # -0.0
    sub = (want & np.uint64(0x7ff0000000000000)) == 0
    assert sub.sum() > 1000   # subnormals and zeros
    # the exact ties are ties: 9007199254740993 lies halfway and goes to the even neighbour
    assert float("9007199254740993") == 9007199254740992.0 and float("9007199254740995") == 9007199254740996.0


@pytest.mark.parametrize("mode", [0, 1])
def test_refusals(mode):
    toks = [t for t, _ in cases.REFUSALS]
    bits, status = host_f64_parse(toks, mode)
    assert [int(s) for s in status] == [s for _, s in cases.REFUSALS], list(zip(toks, status))
    assert not bits.any()
    for t, s in cases.REFUSALS:
        if s == 1:
            with pytest.raises(ValueError):
                float(t)
    assert len("1" + "0" * 48) == 49 and any(len(t) == 49 for t in toks)


def test_mixed_tokens_and_buffer_extent():
    bits, status = host_f64_parse([b"1.5", b"abc", b"-0.0", b"0x1p3", b"2.5e-1"])
    assert list(status) == [0, 1, 0, 2, 0]
    assert list(bits.view(np.float64)[[0, 4]]) == [1.5, 0.25] and bits[2] == 1 << 63
    # a token that leaves the buffer is malformed, nothing outside is read
    buf = np.frombuffer(b"12345678", dtype=np.uint8)
    off = np.array([0, 4, 6, -1, 8], dtype=np.int64)
    length = np.array([8, 4, 4, 2, 0], dtype=np.int32)
    out, st = np.zeros(5, dtype=np.uint64), np.zeros(5, dtype=np.uint8)
    f = _lib.lib.tspgnn_host_f64_parse
    assert f(buf.ctypes.data, 8, off.ctypes.data, length.ctypes.data, 5, 0, out.ctypes.data, st.ctypes.data) == 0
    assert list(st) == [0, 0, 1, 1, 1] and list(out.view(np.float64)[:2]) == [12345678.0, 5678.0]


def test_invalid_arguments():
    f, g = _lib.lib.tspgnn_host_f64_parse, _lib.lib.tspgnn_f64_parse
    assert f(None, 0, None, None, 0, 0, None, None) == 0 and g(None, 0, None, None, 0, 0, None, None, None) == 0
    assert f(None, 0, None, None, 3, 0, None, None) == -1 and b"null" in _lib.lib.tspgnn_last_error()
    assert f(None, 0, None, None, -1, 0, None, None) == -1
    assert g(None, 0, None, None, 3, 0, None, None, None) == -1 and g(None, 0, None, None, -1, 0, None, None, None) == -1
    scan, parse = _lib.lib.tspgnn_graph_text_scan, _lib.lib.tspgnn_graph_text_parse
    assert scan(None, None, None, 0, 0, None, None) == 0
    assert parse(None, None, None, 0, 0, 8, 0, 0, None, None, None, None, None, None) == 0
    assert scan(None, None, None, 0, -1, None, None) == -1 and scan(None, None, None, 0, 1, None, None) == -1
    assert parse(None, None, None, 0, 0, 3, 0, 0, None, None, None, None, None, None) == -1
    assert parse(None, None, None, 0, 0, 257, 0, 0, None, None, None, None, None, None) == -1
    assert parse(None, None, None, 0, 1, 8, 0, 0, None, None, None, None, None, None) == -1
    # rows that leave their arrays are refused on the host, before any launch: the pointers are never followed
    P = 1 << 20
    row2 = lambda *r: np.array([r], dtype=np.int64)
    for tab in (row2(0, 101), row2(-1, 10), row2(96, 8), row2(0, (1 << 30) + 1)):
        assert scan(tab.ctypes.data, P, P, 100, 1, P, None) == -1 and b"leave" in _lib.lib.tspgnn_last_error(), tab
    for tab in (row2(0, 101, 5, 0, 0), row2(0, 50, 3, 0, 0), row2(0, 50, 9, 0, 0), row2(0, 50, 5, 1, 0),
                row2(0, 50, 5, 0, 1), row2(0, 50, 5, -1, 0)):
        assert parse(tab.ctypes.data, P, P, 100, 1, 8, 25, 5, P, P, P, P, P, None) == -1, tab


def test_table_generator_check():
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_parse_table.py"), "--check"])


def test_from_directory_refuses_before_the_gpu(tmp_path):
    with pytest.raises(ValueError, match="reader"):
        DeviceDataset.from_directory(str(tmp_path), device="cpu", reader="bogus")
    with pytest.raises(ValueError, match="HIP kernels"):
        DeviceDataset.from_directory(str(tmp_path), device="cpu", reader="device")
    assert len(DeviceDataset.from_directory(str(tmp_path), device="cpu")) == 0   # the host reader, as before
