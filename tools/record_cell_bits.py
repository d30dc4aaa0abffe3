"""Records tests/golden/cell_fwd_bits.npz: the outputs (as uint32 bit patterns) of tspgnn_lnlstm_mlp_fwd_multi_h2 on the
seeded launches of tests/cell_fwd_bits_cases.py, for tests/test_gpu_cell_fwd_bits.py.

Run it ONCE, on the GPU, with the library of the commit the later kernels must reproduce -- never with the code under test:
    python tools/record_cell_bits.py <commit the library was built from> [output.npz]
The commit, the device and the library's path go into the fixture's "meta" entry (JSON bytes)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tsp-gnn_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

LIMIT = 300 * 1000


def main():
    import torch
    import cell_fwd_bits_cases as C
    from lstm_bwd_cases import release
    from tspgnn import _lib
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "cell_fwd_bits.npz")
    device = torch.device("cuda:0")
    arrays, names = {}, []
    for name, wt, centred, build in C.cases():
        first = C.run_case(build, device, wt, centred)
        release()
        again = C.run_case(build, device, wt, centred)      # the launch has no reduction across rows: same bits twice
        release()
        for k, a in first.items():
            assert np.array_equal(a, again[k]), (name, k)
            arrays[name + "/" + k] = a
        names.append(name)
        print("%-24s %s" % (name, " ".join("%s%s" % (k, list(a.shape)) for k, a in sorted(first.items()))))
    meta = {"commit": commit, "device": torch.cuda.get_device_name(0), "library": os.path.relpath(_lib.LIB_PATH, ROOT),
            "entry": "tspgnn_lnlstm_mlp_fwd_multi_h2", "cases": names}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(out, **arrays)
    size = os.path.getsize(out)
    print("wrote %s: %d arrays, %d bytes (limit %d), meta %s" % (out, len(arrays), size, LIMIT, json.dumps(meta)))
    assert size <= LIMIT, "fixture too large"


if __name__ == "__main__":
    main()
