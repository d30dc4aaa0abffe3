"""tspgnn_host_f64_repr (csrc/graph_text.hip) against Python's repr(float): the host build of the routine the device
writer formats every weight with.  Every comparison is exact."""
import struct

import numpy as np
import pytest

import graph_text_cases as cases
from tspgnn import _lib
from tspgnn.graph_text import REPR_BYTES, host_f64_repr


def check(values):
    values = np.asarray(values, dtype=np.float64)
    got, length = host_f64_repr(values)
    want = cases.expected(values)
    wrong = [(v.hex(), g, w) for v, g, w in zip(values.tolist(), got, want) if g != w]
    assert not wrong, "%d of %d differ from repr, first: %s" % (len(wrong), len(values), wrong[:5])
    assert int(length.max()) <= REPR_BYTES and [len(s) for s in got] == length.tolist()
    back = np.array([float(s) for s in got])
    finite = ~np.isnan(values)
    assert back[finite].tobytes() == values[finite].tobytes() and np.isnan(back[~finite]).all()


def test_fixed_list():
    for x, s in cases.QUOTED.items():
        assert repr(x) == s
    check(cases.FIXED)
    got, length = host_f64_repr([-2.2250738585072014e-308, float("nan"), -0.0])
    assert got == ["-2.2250738585072014e-308", "nan", "-0.0"] and length.tolist() == [24, 3, 4]
    negative_nan = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000001))[0]
    assert host_f64_repr([negative_nan])[0] == ["nan"]


def test_every_power_of_two_with_its_neighbours():
    check(cases.powers_of_two())


def test_every_power_of_ten_with_its_neighbours():
    check(cases.powers_of_ten())


def test_uniform_doubles_of_the_datasets_range():
    check(cases.uniform_sample())


def test_random_bit_patterns():
    v = cases.bit_patterns()
    check(v)
    check(-np.abs(cases.uniform_sample(1000, seed=5)))


def test_short_decimals():
    v = cases.short_decimals()
    assert len({len(s) for s in cases.expected(v[:1000])}) > 10   # every digit count occurs
    check(v)


def test_bytes_past_a_value_are_left_alone():
    x = np.array([0.5, 1e-5, 1 / 3])
    text = np.full(REPR_BYTES * 3, 0x7E, dtype=np.uint8)
    length = np.zeros(3, dtype=np.uint8)
    assert _lib.lib.tspgnn_host_f64_repr(x.ctypes.data, 3, text.ctypes.data, length.ctypes.data) == 0
    for i, s in enumerate(("0.5", "1e-05", "0.3333333333333333")):
        cell = text[REPR_BYTES * i:REPR_BYTES * (i + 1)].tobytes()
        assert cell == s.encode() + b"~" * (REPR_BYTES - len(s)) and length[i] == len(s)


def test_argument_errors():
    x = np.array([1.0])
    text, length = np.zeros(REPR_BYTES, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
    f = _lib.lib.tspgnn_host_f64_repr
    assert f(None, 1, text.ctypes.data, length.ctypes.data) == -1
    assert f(x.ctypes.data, 1, None, length.ctypes.data) == -1
    assert f(x.ctypes.data, 1, text.ctypes.data, None) == -1
    assert f(x.ctypes.data, -1, text.ctypes.data, length.ctypes.data) == -1
    assert b"count" in _lib.lib.tspgnn_last_error()
    assert f(None, 0, None, None) == 0 and not text.any()
    # the device entry points answer before any launch, so they can be asked here
    g = _lib.lib.tspgnn_f64_repr
    assert g(None, 1, None, None, None) == -1 and g(None, -1, None, None, None) == -1 and g(None, 0, None, None, None) == 0
    tab = np.array([[5, 0, 0, 0]], dtype=np.int64)
    one = np.zeros(1, dtype=np.int64)
    p = tab.ctypes.data
    sizes, write = _lib.lib.tspgnn_graph_text_sizes, _lib.lib.tspgnn_graph_text_write
    assert sizes(None, None, None, None, None, 0, 8, 0, 0, None, None) == 0
    assert sizes(None, None, None, None, None, 1, 8, 25, 5, None, None) == -1
    assert sizes(p, p, p, p, p, -1, 8, 25, 5, p, None) == -1
    for n_max in (3, 257):
        assert sizes(p, p, p, p, p, 1, n_max, 25, 5, p, None) == -1
    assert sizes(p, p, p, p, p, 1, 4, 25, 5, p, None) == -1          # n = 5 > n_max
    assert sizes(p, p, p, p, p, 1, 8, 24, 5, p, None) == -1          # the matrix leaves its array
    assert sizes(p, p, p, p, p, 1, 8, 25, 4, p, None) == -1          # the tour leaves its array
    assert write(None, None, None, None, None, 0, 8, 0, 0, None, None, None, 0, None, None) == 0
    assert write(p, p, p, p, p, 1, 8, 25, 5, p, None, p, 100, p, None) == -1
    one[0] = 101
    assert write(p, p, p, p, p, 1, 8, 25, 5, p, one.ctypes.data, p, 100, p, None) == -1   # the file leaves the text
    assert b"leave the text" in _lib.lib.tspgnn_last_error()
    tab[0, 3] = -1
    one[0] = 10
    assert write(p, p, p, p, p, 1, 8, 25, 5, p, one.ctypes.data, p, 100, p, None) == -1   # b0 < 0


@pytest.mark.parametrize("text_bytes, runs", [(10, [(0, 1), (1, 2), (2, 3), (3, 4)]), (29, [(0, 1), (1, 2), (2, 3), (3, 4)]),
                                              (30, [(0, 2), (2, 4)]), (1000, [(0, 4)])])
def test_text_chunks_hold_at_most_text_bytes_and_at_least_one_file(text_bytes, runs):
    from tspgnn.graph_text import _text_chunks
    assert _text_chunks([12, 18, 25, 5], text_bytes) == runs
