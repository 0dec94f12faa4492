"""Generates tests/golden/reference/*.npz: the results of the reference's own
source (oracle/_ref/libref_rt.so, compiled from it where it lies by
oracle/Makefile.ref) on the cases of tests/reference_cases.py.  Each file holds
the case's inputs (camera, size, passes, options, seeds), a SHA-256 of every
scene input file, the reference's scene (hashes of triangles, KD nodes and
indices; light list and bounds) and its four G-buffer arrays after each call —
for the ray case the rays and the reference's Samples.  Run where a copy of the
reference is present:
    make -C oracle -f Makefile.ref && python tests/golden/make_reference_golden.py [case ...]
"""
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in ("isaklm-raytracer_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import oracle  # noqa: E402
import reference_cases as rc  # noqa: E402

MAX_FILE, MAX_DIR = 256 * 1024, 2 * 1024 * 1024


def main(names):
    oracle.build()
    os.makedirs(rc.GOLDEN_DIR, exist_ok=True)
    for name in names or rc.ALL_CASES:
        t = time.time()
        with tempfile.TemporaryDirectory() as d:
            case, out = rc.record(name, d)
            if name == "trap":  # the deepest path, which only the oracle counts, on frames that must agree anyway
                k = {}
                rc.run_frames(case, oracle.OracleScene(case.path), k)
                assert k["maxdepth"] >= rc.TRAP_MIN_DEPTH, k
                print(f"  trap: deepest path {k['maxdepth']} bounces")
        np.savez_compressed(rc.fixture_path(name), **out)
        size = os.path.getsize(rc.fixture_path(name))
        assert size <= MAX_FILE, (name, size)
        print(f"{name}: {size} B, {time.time() - t:.1f} s")
    total = sum(os.path.getsize(os.path.join(rc.GOLDEN_DIR, f)) for f in os.listdir(rc.GOLDEN_DIR))
    assert total <= MAX_DIR, total
    print(f"tests/golden/reference: {total} B")


if __name__ == "__main__":
    main(sys.argv[1:])
