"""rt_reproject_host under AddressSanitizer + UBSan: csrc/host/reproject_host.cpp
and a stand-alone main (tests/native/reproject_host_main.cpp) built with
-fsanitize and run as a child process — nothing sanitized is loaded into
Python.  The frames hold NaN, Inf, negative and huge depths and sums and the
cameras NaN and infinite fields: the reprojection's bounds tests come before
its float-to-int conversions and its gathers, and this is where that shows."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "isaklm-raytracer_amd", "csrc")
INC = os.path.join(ROOT, "include")


def test_host_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "reproject_host_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined,float-cast-overflow",
           "-fno-omit-frame-pointer", "-I" + INC, "-I" + CSRC, os.path.join(HERE, "native", "reproject_host_main.cpp"),
           os.path.join(CSRC, "host", "reproject_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr + r.stdout).lower():
        pytest.skip("sanitizer runtime not available: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l.split() for l in r.stdout.splitlines()]
    assert len(lines) == 36 and all(l[0] == "0" and l[3] == "0" for l in lines), r.stdout
    assert [l[1] for l in lines] == ["67x45"] * 12 + ["3x2"] * 12 + ["1x1"] * 12
    kept = [int(l[4]) for l in lines[:12]]
    assert kept[0] > 0 and kept[1] > 0, "the unmoved camera keeps history under both option sets"
    assert kept[6:12] == [0] * 6, "NaN, infinite and far-away cameras keep nothing"
