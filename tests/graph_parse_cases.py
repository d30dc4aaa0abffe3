"""The tokens tests/test_graph_parse_host.py and tests/test_gpu_graph_read.py parse: the seeded samples, the sweeps, the
spellings, the ties and boundaries, and the refusals with their statuses.  Python's float(token) is the reference for
every token of ``accepted()``; the list is built once per process."""
import functools
from fractions import Fraction

import numpy as np

SEED = 20

SPELLINGS = ["0", "0.0", "-0.0", "+1", ".5", "5.", "-.5", "+5.", "00012.50", "0.000", "-0", "1e-05", "1E5", "1e+5", "1.e3",
             ".5e1", "1e0005", "1e-0005", "12e+007", "1e00000", "1e12345", "1e-12345", "-1e99999", "3e-99999", "0e99999",
             "0.0e-99999", "1e309", "1e-400", "-1e-400", "1e400",
             "1234567890123456789", "9999999999999999999", "0.1234567890123456789", "12345678901.23456789e-30",
             "000000000000000000000000000001234567890123456789", "0.0000000000000000000000000001234567890123456789",
             "9007199254740993", "9007199254740992", "9007199254740994", "9007199254740995", "1844674407370955161",
             "inf", "-inf", "+inf", "nan"]

# both sides of the largest double and of the overflow threshold, the smallest normal, the smallest subnormal and half of it
BOUNDARIES = ["1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308",
              "17976931348623158e292", "1797693134862315807e290", "1797693134862315808e290",
              "2.2250738585072014e-308", "2.2250738585072013e-308", "2.2250738585072011e-308", "2.2250738585072009e-308",
              "4.9e-324", "5e-324", "4.9406564584124654e-324", "7.4109846876186981e-324", "7.4109846876186982e-324",
              "2.4703282292062327e-324", "2.4703282292062328e-324",
              "2.470328229206232720e-324", "2.470328229206232721e-324", "1e-323", "1e-324", "3e-324", "1e-342", "9e-343",
              "9999999999999999999e-343", "1e-343"]

# token -> status: 1 malformed (float() raises too), 2 outside the device grammar
REFUSALS = [("", 1), ("1-2", 1), ("1.5abc", 1), ("e5", 1), ("--1", 1), (".", 1), ("+", 1), ("1e", 1), ("1e+", 1), ("1.2.3", 1),
            ("1_", 1), ("_1", 1), ("1__0", 1), ("0x", 1), ("in", 1), ("nane", 1), ("1 2", 1),
            ("0x10", 2), ("Infinity", 2), ("infinity", 2), ("NaN", 2), ("INF", 2), ("-nan", 2), ("1_0", 2), ("1e1_0", 2),
            ("12345678901234567890", 2), ("0.00012345678901234567890", 2), ("1" + "0" * 48, 2), ("0." + "0" * 47, 2)]


def _bit_patterns(rng, count):
    hi = rng.randint(0, 2 ** 32, size=count, dtype=np.uint64)
    lo = rng.randint(0, 2 ** 32, size=count, dtype=np.uint64)
    return ((hi << np.uint64(32)) | lo).view(np.float64)


def _truncated(value, digits=19):
    """(d, k): the positive rational ``value`` truncated to ``digits`` significant digits, d 10^k."""
    num, den = value.numerator, value.denominator
    k = int((num.bit_length() - den.bit_length()) * 0.30103) - digits
    while True:
        d = num * 10 ** -k // den if k < 0 else num // (den * 10 ** k)
        if d >= 10 ** digits:
            k += 1
        elif d < 10 ** (digits - 1):
            k -= 1
        else:
            return d, k


def _midpoints(x):
    """For the positive finite doubles x: the decimal midpoint between x and the next double, truncated to 19 digits, and
    that value +- 1 in the last digit -- the tokens nearest a rounding boundary that the grammar can spell."""
    out = []
    for v in x:
        mid = (Fraction(float(v)) + Fraction(float(np.nextafter(v, np.inf)))) / 2
        d, k = _truncated(mid)
        out += ["%de%d" % (d + s, k) for s in (0, -1, 1) if d + s < 10 ** 19]
    return out


@functools.lru_cache(maxsize=None)
def accepted():
    """The status-0 tokens (str)."""
    rng = np.random.RandomState(SEED)
    toks = [repr(float(v)) for v in _bit_patterns(rng, 250000)]
    toks += [repr(float(v)) for v in rng.uniform(0.0, 2.0, 250000)]
    toks += [repr(2.0 ** k) for k in range(-1074, 1024)]
    toks += ["1e%d" % k for k in range(0, 330)] + ["1e-%d" % k for k in range(1, 360)]
    # write_graph(int_weights=True): int(bins * w) on an edge, n * bins + 1 elsewhere
    toks += [str(int(10 ** 6 * w)) for w in rng.uniform(0.0, 1.5, 2000)] + [str(n * 10 ** 6 + 1) for n in range(4, 257)]
    toks += SPELLINGS + BOUNDARIES
    # exact ties: odd integers below 2^64 with at most 19 digits, halfway between two doubles once they pass 2^53
    odd = rng.randint(2 ** 53, 10 ** 19 - 1, size=2000, dtype=np.uint64) | np.uint64(1)
    toks += [str(int(v)) for v in odd] + [str(int(v)) + "e%d" % e for v, e in zip(odd[:500], rng.randint(-30, 31, 500))]
    x = np.abs(_bit_patterns(rng, 20000))
    x = x[np.isfinite(x) & (x < 1.7e308)][:10000]
    assert len(x) == 10000
    toks += _midpoints(x)
    sub = rng.randint(1, 2 ** 52, size=2000, dtype=np.uint64).view(np.float64)   # subnormals
    toks += [repr(float(v)) for v in sub] + _midpoints(sub[:500])
    return toks


@functools.lru_cache(maxsize=None)
def expected_bits():
    """float(token) of accepted(), as uint64."""
    return np.array([float(t) for t in accepted()], dtype=np.float64).view(np.uint64)
