"""Records tests/golden/tour_chain_bits.npz: the outputs of the tour chain kernels (the searches, the bound, nearest
neighbour, the annealing and the branch and bound) on the seeded launches of tests/tour_chain_cases.py, for
tests/test_gpu_tour_chain_bits.py.

Run it ONCE, on the GPU, with the library of the commit the later kernels must reproduce -- never with the code under test:
    python tools/record_tour_bits.py <commit the library was built from> [output.npz]
The commit, the device and the library's path go into the fixture's "meta" entry (JSON bytes)."""
import io
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
    import tour_chain_cases as C
    from tspgnn import _lib
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "tour_chain_bits.npz")
    device = torch.device("cuda:0")
    arrays, names, cases = {}, [], C.cases()
    for c in cases:
        first = C.run_case(c, device)
        again = C.run_case(c, device)      # a result depends on (seed, index, the settings) only: same bits twice
        C.check_shape_of_answers(c, C.build(c), first)
        for k, a in first.items():
            assert np.array_equal(a, again[k]), (c["name"], k)
            arrays[c["name"] + "/" + k] = a
        names.append(c["name"])
        print("%-24s %s" % (c["name"], " ".join("%s%s" % (k, list(a.shape)) for k, a in sorted(first.items()))), flush=True)
    for sq, tri in C.twins(cases):          # for n <= 128 the two layouts hold the same fp32 weights
        for k in sorted(k for k in arrays if k.startswith(sq["name"] + "/")):
            assert np.array_equal(arrays[k], arrays[tri["name"] + k[len(sq["name"]):]]), k
    meta = {"commit": commit, "device": torch.cuda.get_device_name(0), "library": os.path.relpath(_lib.LIB_PATH, ROOT),
            "cases": names}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    size = buf.getbuffer().nbytes
    assert size <= LIMIT, "fixture too large: %d bytes (limit %d); nothing written" % (size, LIMIT)
    with open(out, "wb") as f:
        f.write(buf.getvalue())
    print("wrote %s: %d arrays, %d bytes (limit %d), meta %s" % (out, len(arrays), size, LIMIT, json.dumps(meta)))


if __name__ == "__main__":
    main()
