"""Writes tsp-gnn_amd/csrc/graph_text_pow10.inc: the 128-bit powers of ten of csrc/graph_text.hip.

Row e - E_MIN holds g(e) = ceil(10^e / 2^(floor(log2 10^e) - 127)) as {high word, low word}: 2^127 <= g < 2^128, exact when
10^e fits 128 bits and one above the truncation otherwise.  e runs over -k for every decimal exponent k = floor(log10 2^q)
(or floor(log10 (3/4) 2^q)) of a double's binary exponent q in [-1074, 971].  The script also checks the three
fixed-point logarithms the routine uses against exact integer arithmetic over the whole range.

    python tools/gen_pow10_table.py            # rewrites the table
    python tools/gen_pow10_table.py --check    # compares the committed table, writes nothing
"""
import os
import sys

E_MIN, E_MAX = -292, 324
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tsp-gnn_amd", "csrc", "graph_text_pow10.inc")


def floor_log2_pow10(e):
    """floor(log2(10^e)), exactly."""
    if e >= 0:
        return (10 ** e).bit_length() - 1
    p = 10 ** -e   # 10^e = 1 / p, never a power of two: floor(log2(1 / p)) = -ceil(log2 p) = -bit_length(p)
    return -p.bit_length()


def g(e):
    r = floor_log2_pow10(e) - 127
    if e >= 0:
        p = 10 ** e
        v = p << -r if r <= 0 else -((-p) >> r)   # ceiling
    else:
        p = 10 ** -e
        v = -((-(1 << -r)) // p)
    assert 1 << 127 <= v < 1 << 128, e
    return v


def floor_log10(num, den):
    """floor(log10(num / den)), exactly."""
    k = 0
    while num >= 10 * den:
        den *= 10
        k += 1
    while num < den:
        num *= 10
        k -= 1
    return k


def check_logs():
    for e in range(E_MIN, E_MAX + 1):
        assert (e * 1741647) >> 19 == floor_log2_pow10(e), e
    ks = set()
    for q in range(-1074, 972):
        two = (2 ** q, 1) if q >= 0 else (1, 2 ** -q)
        k = floor_log10(*two)
        assert (q * 1262611) >> 22 == k, q
        k34 = floor_log10(3 * two[0], 4 * two[1])
        assert (q * 1262611 - 524031) >> 22 == k34, q
        ks.update((-k, -k34))
        for kk in (k, k34):   # the left shift of the routine: h = q + floor(log2 10^-k) + 1 in [1, 4]
            assert 1 <= q + floor_log2_pow10(-kk) + 1 <= 4, q
    assert min(ks) == E_MIN and max(ks) == E_MAX, (min(ks), max(ks))


def text():
    lines = ["// 10^e, e = %d .. %d, as 128-bit ceilings {high, low}: written by tools/gen_pow10_table.py, do not edit."
             % (E_MIN, E_MAX)]
    for e in range(E_MIN, E_MAX + 1):
        v = g(e)
        lines.append("{0x%016xull, 0x%016xull},  // %d" % (v >> 64, v & ((1 << 64) - 1), e))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    check_logs()
    if "--check" in sys.argv[1:]:
        assert open(OUT).read() == text(), "graph_text_pow10.inc is not what this script writes"
    else:
        with open(OUT, "w") as f:
            f.write(text())
