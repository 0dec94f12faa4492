"""The finisher's instruction budget: counter passes of ONE unchained 256-pass room2m call.

Each pass is a child process under `rocprofv3 --pmc <counters> --kernel-trace` alone (the form bench.py's
measure_pmc uses: bench.py's own --pmc-child render between two tonemap marker dispatches, no other
tracing), under its own `timeout`; the first pass that fails ends the run.  Counters are picked from what
the installed rocprofv3 lists as available (`rocprofv3-avail list` / `rocprofv3 --list-avail`); the
wanted ones it does not list are reported under "missing", not asked for.

Collected for wf_finish_bvh<false, 4>: VALU, SALU, VMEM, SMEM, LDS and flat / scratch instruction counts,
instruction fetches and the instruction cache's requests, hits and misses.  Written to OUT (JSON):
per-counter sums of the kernel, VALU (and every other) instructions per sample and per ray, the
instruction-cache miss rate, and beside them the static figures of the library that ran
(tools/kernel_resources.py: registers, spills, scratch, code bytes).

usage: python tools/fin_trip_budget.py OUT.json [--lib libisaklm_rt.so --build "commit ..."] [--passes 256] [--rays-per-sample R]
       (R: rays per sample of a counted call, bench.py --full "per_sample"; default: the last recorded one, 3.216)
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import bench  # noqa: E402  (its _window_sums / _collect_csv read the passes exactly as measure_pmc does)
import kernel_resources  # noqa: E402

KERNEL = "wf_finish_bvh<false, 4>"
PASS_LIMIT_S = 120
# wanted counters, in passes small enough for one collection each (an SQ pass holds up to 8, an SQC pass fewer)
WANTED = [
    ["SQ_WAVES", "SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_SMEM", "SQ_INSTS_LDS"],
    ["SQ_INSTS_VMEM", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR", "SQ_INSTS_FLAT", "SQ_INSTS_FLAT_LDS_ONLY"],
    ["SQ_IFETCH", "SQ_IFETCH_LEVEL", "SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_WAIT_INST_ANY"],
    ["SQC_ICACHE_REQ", "SQC_ICACHE_HITS", "SQC_ICACHE_MISSES", "SQC_ICACHE_MISSES_DUPLICATE"],
    ["SQ_INSTS_SCRATCH", "SQ_INST_LEVEL_VMEM", "SQ_INSTS_VALU_MFMA_MOPS_F32", "SQ_INSTS_BRANCH", "SQ_INSTS_SENDMSG"],
]


def available():
    """names the installed profiler lists (None: could not be listed — every wanted counter is then tried)"""
    for cmd in (["rocprofv3-avail", "list"], ["rocprofv3", "--list-avail"], ["rocprofv3", "-L"]):
        if not shutil.which(cmd[0]):
            continue
        try:
            r = subprocess.run(["timeout", "-k", "10", "60"] + cmd, capture_output=True, text=True)
        except OSError:
            continue
        names = set(re.findall(r"\b(?:SQC?|TC[CP]|TA|TD|GRBM)_[A-Z0-9_]+\b", r.stdout + r.stderr))
        if r.returncode == 0 and names:
            return names
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lib", default=None, help="library to profile (default: the tree's)")
    ap.add_argument("--build", default=None, help="what the library was built from (recorded; default: 'this tree')")
    ap.add_argument("--passes", type=int, default=256)
    ap.add_argument("--rays-per-sample", type=float, default=3.216)
    ap.add_argument("--scene-dir", default=os.path.join(ROOT, "build", "scenes"))
    a = ap.parse_args()
    lib = os.path.abspath(a.lib) if a.lib else kernel_resources.DEFAULT_LIB
    env = dict(os.environ, TMPDIR="/tmp")
    if a.lib:
        env["ISAKLM_RT_LIB_OVERRIDE"] = lib
    avail = available()
    missing, groups = [], []
    # (the list could not be read: the last group's names are guesses and are left out)
    for g in (WANTED if avail is not None else WANTED[:-1]):
        keep = [c for c in g if avail is None or c in avail]
        missing += [c for c in g if c not in keep]
        if keep:
            groups.append(keep)
    child = [sys.executable, os.path.join(ROOT, "bench.py"), "--pmc-child", "1", "--passes", str(a.passes), "--scene",
             "room2m", "--width", "1920", "--height", "1080", "--scene-dir", a.scene_dir]
    res = {"kernel": KERNEL, "build": a.build or ("this tree" if not a.lib else os.path.basename(lib)), "passes": a.passes, "missing_counters": missing,
           "counters_listed": avail is not None, "counters": {}, "pass_wall_s": [], "error": None}
    samples = None
    for g in groups:
        d = tempfile.mkdtemp(prefix="fin_trip_", dir="/tmp")
        cmd = ["timeout", "-k", "10", str(PASS_LIMIT_S), "rocprofv3", "--pmc", *g, "--kernel-trace", "-d", d, "-o", "run",
               "--output-format", "csv", "--"] + child
        t = time.perf_counter()
        print("[fin_trip_budget] pass:", " ".join(g), file=sys.stderr, flush=True)
        r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            res["error"] = f"pass {g} rc={r.returncode}: stopped"
            shutil.rmtree(d, ignore_errors=True)
            break
        try:
            _, per_kernel, _, ktrace = bench._window_sums(bench._collect_csv(d, "counter_collection"),
                                                          bench._collect_csv(d, "kernel_trace"))
            info = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{\"pmc_child\"")][-1])
        except Exception as e:  # noqa: BLE001
            res["error"] = f"parsing pass {g}: {e}"
            shutil.rmtree(d, ignore_errors=True)
            break
        shutil.rmtree(d, ignore_errors=True)
        samples = info["samples"]
        for k, c in per_kernel.items():
            if k.startswith(KERNEL[:48]):
                res["counters"].update(c)
        res["pass_wall_s"].append(round(time.perf_counter() - t, 1))
    c = res["counters"]
    res["samples"] = samples
    res["rays_per_sample_assumed"] = a.rays_per_sample
    if samples:
        res["per_sample"] = {k: round(v / samples, 2) for k, v in c.items() if k.startswith("SQ_INSTS") or k == "SQ_IFETCH"}
        res["per_ray"] = {k: round(v / samples / a.rays_per_sample, 2) for k, v in c.items() if k.startswith("SQ_INSTS")}
    if c.get("SQC_ICACHE_REQ"):
        res["icache_miss_rate"] = float("%.4g" % (c.get("SQC_ICACHE_MISSES", 0.0) / c["SQC_ICACHE_REQ"]))
    elif c.get("SQC_ICACHE_HITS") is not None and c.get("SQC_ICACHE_MISSES") is not None:
        res["icache_miss_rate"] = float("%.4g" % (c["SQC_ICACHE_MISSES"] / max(c["SQC_ICACHE_HITS"] + c["SQC_ICACHE_MISSES"], 1.0)))
    try:
        res["static"] = {n: v for n, v in kernel_resources.kernels(lib).items()
                         if "wf_finish_bvhILb0ELi4" in n or "wf_longILb0" in n}
    except Exception as e:  # noqa: BLE001
        res["static"] = {"error": str(e)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res.get(k) for k in ("error", "missing_counters", "per_sample", "icache_miss_rate")}))
    return 1 if res["error"] else 0


if __name__ == "__main__":
    sys.exit(main())
