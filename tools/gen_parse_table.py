"""Writes tsp-gnn_amd/csrc/graph_parse_pow10.inc: the 128-bit powers of ten of csrc/graph_parse.hip.

Row e - E_MIN holds t(e) = floor(10^e / 2^(floor(log2 10^e) - 127)) as {high word, low word}: 2^127 <= t < 2^128, exact when
10^e fits 128 bits (0 <= e <= 55) and the truncation otherwise, so 10^e = (t + theta) 2^(floor(log2 10^e) - 127) with
0 <= theta < 1.  e runs over every decimal exponent at which a mantissa of at most 19 digits is neither certainly zero nor
certainly infinite as a double.  The script also checks the fixed-point logarithm and the power of five the routine uses
against exact integer arithmetic, and the two ends of the range.

    python tools/gen_parse_table.py            # rewrites the table
    python tools/gen_parse_table.py --check    # compares the committed table, writes nothing
"""
import os
import sys

E_MIN, E_MAX = -342, 308
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tsp-gnn_amd", "csrc", "graph_parse_pow10.inc")


def floor_log2_pow10(e):
    """floor(log2(10^e)), exactly."""
    if e >= 0:
        return (10 ** e).bit_length() - 1
    p = 10 ** -e   # 10^e = 1 / p, never a power of two: floor(log2(1 / p)) = -ceil(log2 p) = -bit_length(p)
    return -p.bit_length()


def t(e):
    r = floor_log2_pow10(e) - 127
    if e >= 0:
        p = 10 ** e
        v = p << -r if r <= 0 else p >> r
    else:
        v = (1 << -r) // 10 ** -e
    assert 1 << 127 <= v < 1 << 128, e
    return v


def check():
    for e in range(E_MIN, E_MAX + 1):
        assert (e * 1741647) >> 19 == floor_log2_pow10(e), e
    # the ends: the largest 19-digit mantissa one row below the table is below half the smallest subnormal, and the
    # smallest mantissa one row above it is beyond the largest double's rounding range
    assert (10 ** 19 - 1) * 2 ** 1075 < 10 ** -(E_MIN - 1)
    assert 10 ** (E_MAX + 1) >= 2 ** 1024
    # the exact comparison: 5^27 fits a 64-bit multiplier, 13 of them reach 5^342, and the words suffice
    assert 5 ** 27 < 1 << 64 and 13 * 27 >= max(-E_MIN, E_MAX)
    assert (5 ** -E_MIN).bit_length() + 64 + 56 <= 32 * 40
    assert (5 ** E_MAX).bit_length() + 64 + 56 + E_MAX <= 32 * 40


def text():
    lines = ["// 10^e, e = %d .. %d, as 128-bit truncations {high, low}: written by tools/gen_parse_table.py, do not edit."
             % (E_MIN, E_MAX)]
    for e in range(E_MIN, E_MAX + 1):
        v = t(e)
        lines.append("{0x%016xull, 0x%016xull},  // %d" % (v >> 64, v & ((1 << 64) - 1), e))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    check()
    if "--check" in sys.argv[1:]:
        assert open(OUT).read() == text(), "graph_parse_pow10.inc is not what this script writes"
    else:
        with open(OUT, "w") as f:
            f.write(text())
