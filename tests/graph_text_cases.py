"""The doubles tests/test_graph_text_host.py and tests/test_gpu_graph_text.py format: the fixed list, the two sweeps and
the seeded samples.  Python's repr(float(x)) is the reference for every one of them."""
import numpy as np

FIXED = [0.0, -0.0, 5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1.7976931348623157e308,
         1e-4, 9.999999999999999e-05, 1e-5, 1e16, 9999999999999998.0,
         1e22, 1e23, 123456789012345680.0,
         0.1, 0.3, 1 / 3,
         float("inf"), float("-inf"), float("nan"),
         2.0 ** -44,                  # the short side of a power of two: 5.684341886080802e-14
         2.0 ** 50 + 0.25,            # a tie between two 17-digit strings: the even one, ...624.2
         1.0, -1.5, 100.0, 1e15, 123.456, 0.001, 0.00012345678901234567]

# the strings the issue quotes, checked against this Python as well as against the library
QUOTED = {2.0 ** -44: "5.684341886080802e-14", 1e-5: "1e-05", 1e16: "1e+16", 5e-324: "5e-324",
          1.7976931348623157e308: "1.7976931348623157e+308", -2.2250738585072014e-308: "-2.2250738585072014e-308",
          0.0: "0.0", 1e22: "1e+22", 9999999999999998.0: "9999999999999998.0", 1e-4: "0.0001"}


def with_neighbours(values):
    v = np.asarray(values, dtype=np.float64)
    return np.concatenate([v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)])


def powers_of_two():
    return with_neighbours([2.0 ** k for k in range(-1074, 1024)])


def powers_of_ten():
    return with_neighbours([float("1e%d" % k) for k in range(-323, 309)])


def uniform_sample(count=200000, seed=11):
    return np.random.RandomState(seed).uniform(0.0, 2.0 ** 0.5, count)


def bit_patterns(count=200000, seed=12):
    rng = np.random.RandomState(seed)
    hi = rng.randint(0, 2 ** 32, size=count, dtype=np.uint64)
    lo = rng.randint(0, 2 ** 32, size=count, dtype=np.uint64)
    return ((hi << np.uint64(32)) | lo).view(np.float64)


def short_decimals(count=100000, seed=13):
    rng = np.random.RandomState(seed)
    u = rng.uniform(0.0, 1.0, count) * 10.0 ** rng.randint(-30, 31, count)
    return np.array([float("%.*g" % (1 + k % 17, x)) for k, x in enumerate(u)])


def expected(values):
    return [repr(float(x)) for x in values]
