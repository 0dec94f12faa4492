"""rt_convergence_host under AddressSanitizer + UBSan: csrc/host/convergence_host.cpp
and a stand-alone main (tests/native/convergence_host_main.cpp) built with
-fsanitize and run as a child process — nothing sanitized is loaded into
Python.  Sizes 0, 1 and 257 on arrays exactly that long; counts of INT32_MIN,
-1, 0, 1, 2 and INT32_MAX; sums that are NaN, infinite, negative and huge;
tolerances that are NaN, infinite, negative and 1e9: the test forms no
count - 1 from a count below 0, converts no float to an int and reads nothing
at index n, and this is where that shows."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "isaklm-raytracer_amd", "csrc")
INC = os.path.join(ROOT, "include")

COUNTS = [-2**31, -1, 0, 1, 2, 3, 1000, 2**31 - 1]
MINS = [0, 1, 4, 1001, 2**31 - 1]


def test_host_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "convergence_host_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined,float-cast-overflow",
           "-fno-omit-frame-pointer", "-I" + INC, "-I" + CSRC, os.path.join(HERE, "native", "convergence_host_main.cpp"),
           os.path.join(CSRC, "host", "convergence_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr + r.stdout).lower():
        pytest.skip("sanitizer runtime not available: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l.split() for l in r.stdout.splitlines()]
    cases = [[int(v) for v in l] for l in lines[:-1]]
    assert len(cases) == 3 * 5 * 7 and {c[1] for c in cases} == {0, 1, 257}
    for rc, n, m, t, elements, n_open, below, samples, n_inf, n_nan in cases:
        assert rc == 0 and elements == n
        counts = [COUNTS[(MINS.index(m) + t) % 8]] if n == 1 else [COUNTS[i % 8] for i in range(n)]
        # the classes that need no float arithmetic: below min_samples (always open), the count sum (modulo
        # 2^64), the map's +inf for count < 2
        assert below == sum(c < m for c in counts)
        assert below <= n_open <= n
        assert samples == sum(counts) % 2**64
        assert n_inf >= sum(c < 2 for c in counts)
        if m == 2**31 - 1:
            assert n_open == below == sum(c < m for c in counts)
    # every bad argument is rejected (RT_E_INVALID = -1) before anything is read
    assert lines[-1][0] == "invalid" and lines[-1][1:] == ["-1"] * 7
