"""The finisher's parked s_min queries under the wave's work budget (csrc/bvh_trace.h bvh4_query_budget,
WF_BVH_BUDGET) on the GPU:

* a counted call (RT_TRAVERSAL_BOUNDED_COUNTED: wf_finish_bvh<true, 4>) with RT_DEBUG_BUDGET1 — every wave parks
  its unfinished queries after one body of work, in front of node steps and leaf visits alike — renders the
  frame of the plain KD traversal (RT_TRAVERSAL_KD) of the same call bit for bit: frame buffer, squared
  luminance, sample count;
* its BVH node, BVH test and barycentric record counters equal those of the same counted call at the shipped
  budget: parking moves no work;
* a default-options render (the product instantiation at the shipped budget) equals the KD render too.

The host restatement and the progress rule that makes a budget of 1 terminate: tests/test_trip_budget_host.py.
"""
import numpy as np
import pytest

import helpers
import rt

pytestmark = pytest.mark.gpu
WF = rt.KERNEL_WAVEFRONT
PASSES = 4
FRAMES = {"room_small": (64, 48), "cornell_blob": (48, 32)}
WORK = ("b_bvh_node", "b_bvh_tri", "b_bary")


_FRAMES = {}


def _frame(name):
    """(run, W, H, the KD traversal's render): computed once per scene and left unchanged"""
    if name not in _FRAMES:
        W, H = FRAMES[name]
        run = helpers.GpuRun(name)
        ref, _, _ = run.render(W, H, PASSES, kernel=WF, traversal=rt.TRAVERSAL_KD)
        _FRAMES[name] = (run, W, H, ref)
    return _FRAMES[name]


def _same(out, ref, what):
    for name, a, b in list(zip(("frame_buffer", "squared_luminance", "sample_count"), out, ref)):
        av = a.view(np.uint32) if a.dtype == np.float32 else a
        bv = b.view(np.uint32) if b.dtype == np.float32 else b
        bad = np.nonzero((av != bv).reshape(len(av), -1).any(axis=1))[0]
        assert len(bad) == 0, f"{what} {name}: {len(bad)} of {len(av)} pixels differ; first {bad[:8]}"


def _counted(run, W, H, debug):
    """one counted call (wf_finish_bvh<true, 4>): the frame and the finisher's own counters"""
    g = rt.GBuffer(W, H)
    cnt = rt.DeviceCounters()
    rt.render(run.dev, g, run.camera, 0,
              rt.options(W, H, PASSES, adaptive=False, counters=cnt.p, kernel=WF,
                         traversal=rt.TRAVERSAL_BOUNDED_COUNTED, debug=debug))
    rt.join()
    return g.download(), cnt.read(finisher=True)


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_budget_of_one_renders_the_kd_frame_and_moves_no_work(name):
    run, W, H, ref = _frame(name)
    out1, cnt1 = _counted(run, W, H, rt.DEBUG_BUDGET1)
    _same(out1, ref, "counted call, budget 1")
    out, cnt = _counted(run, W, H, 0)
    _same(out, ref, "counted call, shipped budget")
    print({k: (cnt1[k], cnt[k]) for k in WORK})
    assert cnt["b_bvh_node"] > W * H * PASSES, cnt  # (the queries did run in the counting finisher)
    for k in WORK:
        assert cnt1[k] == cnt[k], (k, cnt1, cnt)


def test_shipped_budget_in_the_product_kernel_renders_the_kd_frame():
    run, W, H, ref = _frame("room_small")
    out, _, _ = run.render(W, H, PASSES, kernel=WF)
    _same(out, ref, "default options")
