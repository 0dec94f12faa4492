"""Where a deep bounce's time goes in wf_long's wide KD traversal (the verdict's
per-round split): one counted room2m call (RtOptions.counters: the counting
build, KD traversal, deep paths in wf_long<true>) and the wide traversal's own
counters — calls (= bounces traced wide), frontier rounds, and s_memtime
cycles in the frontier + node load wait, the cooperative leaf batch and the
expansion (RT_CNT_WIDE_*, RT_CNT_T_WIDE_*; the counting build waits for each
phase's loads, so the split is of that build).  usage: python tools/wide_rounds.py [passes] [scene]

With a third argument `bounded`: the work of wf_long's bounded deep bounces
instead (csrc/wide_bvh.h) — one RT_TRAVERSAL_BOUNDED_COUNTED call in which only
wf_long counts (RtOptions.debug RT_DEBUG_COUNT_LONG_ONLY): per s_min query its
dependent rounds, wide nodes expanded, leaf slots tested and barycentric
records, and the KD nodes and tests of the bounded KD phase per ray — the
figures tools/deep_ray_work.cpp models on the host (rounds, wide nodes, tests,
KD nodes from the root).  usage: python tools/wide_rounds.py [passes] [scene] bounded"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "isaklm-raytracer_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import helpers  # noqa: E402
import rt  # noqa: E402

passes = int(sys.argv[1]) if len(sys.argv) > 1 else 8
scene = sys.argv[2] if len(sys.argv) > 2 else "room2m"
W, H = 1920, 1080
rt.check(rt.lib().rt_set_device(0))
run = helpers.GpuRun(scene)
g = rt.GBuffer(W, H)
cnt = rt.DeviceCounters()
if len(sys.argv) > 3 and sys.argv[3] == "bounded":
    rt.deviation_stats(reset=True)
    rt.render(run.dev, g, run.camera, 0, rt.options(W, H, passes, adaptive=False, kernel=rt.KERNEL_WAVEFRONT,
                                                     counters=cnt.p, traversal=rt.TRAVERSAL_BOUNDED_COUNTED,
                                                     debug=rt.DEBUG_COUNT_LONG_ONLY))
    rt.join()
    a = cnt.words.read()
    kd_nodes, kd_tests, rays, calls, rounds, wnodes, wtests, bary = (int(a[i]) for i in (0, 1, 7, 22, 23, 37, 38, 39))
    dev = rt.deviation_stats()
    q = max(calls, 1)
    print(json.dumps({"scene": scene, "passes": passes, "wf_long_rays": rays, "smin_queries": calls,
                      "per_query": {"rounds": round(rounds / q, 2), "wide_nodes": round(wnodes / q, 2),
                                    "tests": round(wtests / q, 2), "bary_records": round(bary / q, 2)},
                      "kd_phase_per_ray": {"nodes": round(kd_nodes / max(rays, 1), 2), "tests": round(kd_tests / max(rays, 1), 2)},
                      "wide_overflows": dev["wide_overflows"], "max_deep_depth": dev["max_deep_depth"],
                      "note": "wf_long's rays only (deep paths' bounces and their shadow rays); kd_phase_per_ray is over all "
                              "of them, the misses (no KD phase) and the rays the bound does not apply to included"}), flush=True)
    sys.exit(0)
rt.render(run.dev, g, run.camera, 0, rt.options(W, H, passes, adaptive=False, kernel=rt.KERNEL_WAVEFRONT,
                                                 counters=cnt.p))
rt.join()
a = cnt.words.read()
calls, rounds, t, tl, tf, te = (int(a[i]) for i in (22, 23, 24, 25, 26, 27))
print(json.dumps({"scene": scene, "passes": passes, "wide_calls": calls, "rounds": rounds,
                  "rounds_per_call": round(rounds / max(calls, 1), 2),
                  "cycles_per_call": round(t / max(calls, 1), 1), "cycles_per_round": round(t / max(rounds, 1), 1),
                  "share": {"frontier_and_load_wait": round(tl / max(t, 1), 3), "leaf_batch": round(tf / max(t, 1), 3),
                            "expansion": round(te / max(t, 1), 3)},
                  "note": "s_memtime shader cycles; counting build (each phase waits for its loads)"}), flush=True)
