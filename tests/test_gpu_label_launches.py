"""What the labelling and dataset host code launches, pinned: every library call of ``label_tours``, ``prove_tours``,
``solve_tours``, ``nearest_neighbor_tours``, ``anneal_tours``, ``metric_closure``, ``DeviceDataset.generate`` and
``DeviceDataset.batch`` over mixed size classes, ragged chunks and the opt-in switches is recorded -- entry point, integer
and float arguments, which pointers are null -- and compared with tests/golden/label_launches.json.  A launch loop that
chunks differently, a size class that takes the other kernel layout, a bound launch that appears or goes missing, a null
pointer that becomes an array fails its case here instead of passing a parity test by another route.

The recorder is the one of tests/test_launch_trace.py (``recording(forward=True)``): it replaces ``_lib.call`` and
``_lib.current_stream``, records and forwards, so the traces are those of launches that really ran.  Addresses are not
recorded.  Beside each trace the fixture holds what the call returned -- the tours, and the branch and bound's statuses and
node counts where there are any -- as plain lists: the kernels' results depend on (seed, index, settings) only, so they are
part of what the host code must keep feeding them.

Every case seeds ``random`` and ``np.random`` itself.  The search runs restarts=2, kicks=4, lb_iters=20 (as
tests/test_gpu_generate.py): its quality is not under test.

``python tests/test_gpu_label_launches.py`` rewrites the fixture from the code as it stands; pytest only ever compares.
"""
import json
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_launch_trace import recording

from tspgnn import baselines, dataset
from tspgnn.device_dataset import DeviceDataset

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "label_launches.json")
KW = dict(restarts=2, kicks=4, lb_iters=20)
SIZES = [3, 5, 9, 9, 12, 130, 129]      # n < 4 on the host, the square kernels, the triangle kernels
INDEX = [11, 4, 7, 0, 30, 2, 19]
IDS = [3, 3, 0, 7, 5, 5, 5, 1, 6]       # DeviceDataset.batch: a ragged index list with repeats


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def _instances(sizes=SIZES, seed=1):
    """-> ([(Ma, Mw)], planted cycles) of dataset._draw_graph at connectivity 0.7 (so the penalty is in play)."""
    _seed(seed)
    graphs = [dataset._draw_graph(n, 0.7) for n in sizes]
    return [(g[0], g[1]) for g in graphs], [g[2] for g in graphs]


def _tours(results):
    return [[int(v) for v in r.tour] for r in results]


def _stats(stats):
    return {"status": [str(s) for s in stats["status"]], "nodes": [int(x) for x in stats["nodes"]]}


def _label(chunk=2, **kw):
    inst, perms = _instances()
    perms[2] = None
    stats = {}
    with recording(forward=True) as trace:
        res = dataset.label_tours(inst, seed=3, init_tours=perms, index=INDEX, chunk=chunk, stats=stats, **dict(KW, **kw))
    out = {"tours": _tours(res), "trace": trace}
    if stats:
        out.update(_stats(stats))
    return out


def _prove():
    inst, perms = _instances()
    perms[2] = None
    res = dataset.label_tours(inst, seed=3, init_tours=perms, index=INDEX, chunk=2, **KW)
    stats = {}
    with recording(forward=True) as trace:
        out = dataset.prove_tours(inst, res, max_nodes=64, node_iters=7, root_iters=25, chunk=3, stats=stats)
    return dict(_stats(stats), tours=_tours(out), trace=trace)


def _solve():
    inst, _ = _instances(SIZES[:5])
    with recording(forward=True) as trace:
        res = dataset.solve_tours(inst, seed=3, chunk=2, **KW)
    return {"tours": _tours(res), "trace": trace}


def _nearest(start, chunk=2):
    inst, _ = _instances()
    with recording(forward=True) as trace:
        res = baselines.nearest_neighbor_tours(inst, start=start, chunk=chunk)
    return {"tours": _tours(res), "trace": trace}


def _anneal(with_init=False, **kw):
    inst, perms = _instances()
    perms[2] = None
    with recording(forward=True) as trace:
        res = baselines.anneal_tours(inst, chains=2, seed=3, init_tours=perms if with_init else None, index=INDEX, chunk=2,
                                     **kw)
    return {"tours": _tours(res), "trace": trace}


def _closure():
    _seed(5)
    mats = [np.random.rand(n, n) for n in (4, 20, 144, 150)]
    with recording(forward=True) as trace:
        out = dataset.metric_closure(mats, chunk_bytes=3000)     # each tier in two launches
    assert [m.shape for m in out] == [m.shape for m in mats]
    return {"trace": trace}


def _generate(args, **kw):
    _seed(7)
    with recording(forward=True) as trace:
        ds = DeviceDataset.generate(*args, **dict(KW, **kw))
    out = {"tours": [int(v) for v in ds.tours[0]], "n": [int(v) for v in ds.n], "trace": trace}
    if "proved" in ds.summary:
        out["proved"] = [bool(x) for x in ds.summary["proved"]]
        out["nodes"] = [int(x) for x in ds.summary["nodes"]]
    return out


RANDOM = (8, 5, 12, 0.4, 1.0, "random")     # samples, nmin, nmax, conn_min, conn_max, distances


def _batch():
    _seed(7)
    ds = DeviceDataset.generate(*RANDOM, **KW)
    with recording(forward=True) as trace:
        b = ds.batch(IDS, dev=0.02)
        ds.batch(IDS[::-1], dev=0.05, target_cost=1.5, out=ds.batch(IDS[::-1]))
    torch.cuda.synchronize()
    return {"shape": [b.M, b.N, b.B], "trace": trace}


CASES = {
    "label_tours/mixed": _label,
    "label_tours/mixed-chunk-3": lambda: _label(chunk=3),      # four square instances: launches of 3 and 1
    "label_tours/neighbors-no-bound": lambda: _label(neighbors=5, lower_bound=False),
    "label_tours/exact": lambda: _label(exact=True, max_nodes=64),
    "prove_tours": _prove,
    "solve_tours/no-init": _solve,
    "nearest_neighbor/start-0": lambda: _nearest(0),
    "nearest_neighbor/start-best": lambda: _nearest("best"),
    "nearest_neighbor/start-0-chunk-3": lambda: _nearest(0, chunk=3),
    "anneal/schedule-init": lambda: _anneal(with_init=True, levels=3, sweeps=1),
    "anneal/inv-temp-per-level": lambda: _anneal(inv_temp=[0.5, 2.0, float(2 ** 20)], per_level=[7, 9, 11, 13, 15, 17, 19]),
    "anneal/levels-0": lambda: _anneal(levels=0),
    "metric_closure": _closure,
    "generate/random-chunked": lambda: _generate(RANDOM, chunk_bytes=2000),
    "generate/both-classes": lambda: _generate((3, 127, 130)),
    "generate/random-chunked-exact": lambda: _generate(RANDOM, chunk_bytes=2000, exact=True, max_nodes=64),
    "batch/ragged": _batch,
}


def _plain(got):
    return json.loads(json.dumps(got, default=int))     # (numpy integers among the arguments)


def _expected():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("key", sorted(CASES))
def test_label_launches(key):
    want = _expected()["cases"]
    assert key in want, "no recorded trace for %s" % key
    got, exp = _plain(CASES[key]()), want[key]
    for n, (g, e) in enumerate(zip(got["trace"], exp["trace"])):
        assert g == e, "%s: call %d differs\n got      %s\n expected %s" % (key, n, json.dumps(g), json.dumps(e))
    assert len(got["trace"]) == len(exp["trace"]), "%s: %d calls, expected %d" % (key, len(got["trace"]), len(exp["trace"]))
    assert sorted(got) == sorted(exp)
    for k in exp:
        assert got[k] == exp[k], (key, k)


def test_fixture_holds_exactly_these_cases():
    assert sorted(_expected()["cases"]) == sorted(CASES)


def _write():
    """One call per line: readable, and a changed launch shows as a one-line diff."""
    blocks = []
    for key in CASES:
        got = _plain(CASES[key]())
        head = ["  %s: %s" % (json.dumps(k), json.dumps(got[k], sort_keys=True)) for k in sorted(got) if k != "trace"]
        calls = ",\n".join("    " + json.dumps(c) for c in got["trace"])
        head.append('  "trace": [\n%s\n  ]' % calls if calls else '  "trace": []')
        blocks.append("%s: {\n%s\n}" % (json.dumps(key), ",\n".join(head)))
    with open(FIXTURE, "w") as f:
        f.write('{\n"cases": {\n' + ",\n".join(blocks) + "\n}\n}\n")


if __name__ == "__main__":
    _write()
