"""csrc/rt_workspace.h on the CPU, under AddressSanitizer + UBSan: the per-device
slot table, the serial event's order (no wait on first use, a stream wait per
later use, a host wait before a buffer is replaced, no record after a failed
launch) and the shutdown walk (every slot released with its device current, a
device that cannot be entered skipped, the caller's device restored, the
table reusable afterwards), driven by tests/native/workspace_check.cpp with a
stub resource and stub HIP entry points — no HIP runtime is linked and
nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "isaklm-raytracer_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_slot_table_and_serial_event_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "workspace_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + CSRC,
           os.path.join(HERE, "native", "workspace_check.cpp"), "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr + r.stdout).lower():
        pytest.skip("sanitizer runtime not available: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("workspace_check OK"), r.stdout
