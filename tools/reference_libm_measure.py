"""A measurement, not a test: how many pixels of a 48x36, 4 spp
frame differ between the reference's own source built with the project's
transcendentals (oracle/_ref/libref_rt.so, the pinned build) and the same
source built with the host's libm (oracle/_ref/libref_rt_glibc.so).  The count
depends on the libm's version.  Needs a copy of the reference:
    make -C oracle -f Makefile.ref all glibc && python tools/reference_libm_measure.py
"""
import os
import platform
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("isaklm-raytracer_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import reference  # noqa: E402
import reference_cases as rc  # noqa: E402


def main():
    print("libc:", " ".join(platform.libc_ver()))
    with tempfile.TemporaryDirectory() as d:
        for name in ("adversarial_near", "adversarial_far", "adversarial_tiny", "cornell", "textured", "trap"):
            dd = os.path.join(d, name)
            os.makedirs(dd)
            a = rc.Case(name, dd, reference.ReferenceScene)
            b = rc.Case(name, dd, lambda p: reference.ReferenceScene(p, reference.GLIBC_LIB_PATH))
            sa, sb = rc.scene_bytes(a.scene), rc.scene_bytes(b.scene)
            same_scene = bool((sa[0] == sb[0]).all()) and sa[1] == sb[1] and np.array_equal(sa[2], sb[2])
            a.passes = b.passes = [4]
            fa, fb = rc.run_frames(a)[-1], rc.run_frames(b)[-1]
            pixels = int((fa[0].view(np.uint32) != fb[0].view(np.uint32)).any(axis=1).sum())
            states = int((fa[3] != fb[3]).sum())
            print(f"{name}: scene bytes equal: {same_scene}; {pixels} of {len(fa[1])} pixels and {states} final RNG "
                  f"states differ")


if __name__ == "__main__":
    main()
