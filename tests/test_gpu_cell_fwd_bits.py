"""The fused f16x2 forward cell launch, bit for bit against tests/golden/cell_fwd_bits.npz (recorded by
tools/record_cell_bits.py on the commit named in the fixture's "meta" entry, before the tile's f32 arithmetic got its
single-issue form).  Cases and planted rows: tests/cell_fwd_bits_cases.py.  Every output of every task, and the range_flag word,
must be numpy.array_equal to the recording."""
import json
import os

import numpy as np
import pytest

import cell_fwd_bits_cases as C
from lstm_bwd_cases import release

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cell_fwd_bits.npz")
CASES = C.cases()


@pytest.fixture(scope="module")
def recorded():
    z = np.load(GOLDEN)
    meta = json.loads(bytes(z["meta"]).decode())
    assert meta["commit"] and sorted(meta["cases"]) == sorted(c[0] for c in CASES), meta
    return z


@pytest.fixture(autouse=True)
def _release():
    yield
    release()


@pytest.mark.parametrize("name,wt,centred,build", CASES, ids=[c[0] for c in CASES])
def test_cell_forward_bits(cuda_device, recorded, name, wt, centred, build):
    got = C.run_case(build, cuda_device, wt, centred)
    keys = sorted(k[len(name) + 1:] for k in recorded.files if k.startswith(name + "/"))
    assert sorted(got) == keys, (sorted(got), keys)
    bad = []
    for k in keys:
        want = recorded[name + "/" + k]
        same = got[k].shape == want.shape and np.array_equal(got[k], want)
        if not same:
            n = int((got[k] != want).sum()) if got[k].shape == want.shape else -1
            bad.append((k, n))
    print(" CELLBITS %s: %d arrays, %d differ %s" % (name, len(keys), len(bad), bad))
    assert not bad, bad
