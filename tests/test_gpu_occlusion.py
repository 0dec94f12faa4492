"""The occlusion query on the GPU (rt_occluded; csrc/query.hip
rt_occluded_kernel, csrc/bvh_trace.h occluded_bvh) against its definition:

    occluded = (the oracle's trace_ray hits) && (s < tmax)

with s the winning intersect_triangle's ray parameter, restated in numpy on
the oracle's hit triangle (occlusion_ref.s_reference; pinned to the host
checker's plain KD traversal by tests/test_occlusion_cpu.py) — never taken
from the code under test.  Every comparison is exact: a uint8 per ray.  The
ray sets and the oracle's results are those of tests/test_gpu_query.py
(imported and shared).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import hazards
import occlusion_ref as oref
import rt
import test_gpu_query as tq

pytestmark = pytest.mark.gpu
f32 = np.float32
MODES = tq.MODES
N = tq.N
INF = f32(np.inf)
E_INVALID = -1
SCENES = ["cornell", "room_small"]


def hit_and_s(c, kind):
    """the oracle's hit flag and the reference s of its hit triangle (computed once per ray set)"""
    cache = c.__dict__.setdefault("_occlusion_s", {})
    if kind not in cache:
        ref = c.ref(kind)
        hit = ref[:, 0] == 1
        s = oref.s_reference(c.tris, c.rays(kind), np.where(hit, ref[:, 1], -1))
        assert np.isfinite(s[hit]).all() and (s[hit] >= f32(1e-5)).all()
        s.setflags(write=False)
        cache[kind] = (hit, s)
    return cache[kind]


def assert_occluded(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, what
    bad = np.nonzero(got != want.astype(np.uint8))[0]
    assert len(bad) == 0, (what, len(bad), bad[:8], got[bad[:8]])


# ------------------------------------------------------------------ 1. the hit flag
@pytest.mark.parametrize("kind", tq.CLASSES)
@pytest.mark.parametrize("name", SCENES)
def test_no_tmax_is_the_hit_flag(name, kind):
    c = tq.case(name)
    rays, ref = c.rays(kind), c.ref(kind)
    hit = ref[:, 0] == 1
    if kind == "inbox":
        assert 0.25 <= hit.mean() <= 0.98
    for mode in MODES:
        assert_occluded(rt.occluded(c.run.dev, rays, traversal=mode), hit, f"{name} {kind} mode {mode} tmax None")
        assert_occluded(rt.occluded(c.run.dev, rays, np.full(len(rays), INF, f32), traversal=mode), hit,
                        f"{name} {kind} mode {mode} tmax +inf")
        assert_occluded(rt.occluded(c.run.dev, rays, INF, traversal=mode), hit, f"{name} {kind} mode {mode} scalar")


# ------------------------------------------------------------------ 2. the threshold, bit-exact
def check_thresholds(c, kind, what):
    rays = c.rays(kind)
    hit, s = hit_and_s(c, kind)
    nh = int(hit.sum())
    assert nh >= 40 and (~hit).sum() >= 40, (what, nh)  # (test_gpu_query asserts >= 1 % hits on the sparsest set)
    zero = np.zeros(len(rays), bool)
    g = np.random.default_rng(31)
    u = np.exp2(g.uniform(-4.0, 4.0, len(rays))).astype(f32)
    random_tmax = (s * u).astype(f32)
    random_want = hit & (s < random_tmax)
    share = random_want[hit].mean()
    print(f"{what}: hits {nh} of {len(rays)}, random tmax: occluded share of the hit rays {share:.3f}")
    assert 0.25 <= share <= 0.75, share  # each outcome on at least a quarter of the hit rays
    sets = [  # (tmax of the hit rays, tmax of the misses, the expected answer)
        (s, INF, zero, "tmax = s"),
        (np.nextafter(s, INF), f32(1.0), hit, "tmax = nextafter(s, +inf)"),
        (np.nextafter(s, -INF), f32(3e38), zero, "tmax = nextafter(s, -inf)"),
        (random_tmax, random_tmax, random_want, "tmax = s * u"),
    ]
    for t_hit, t_miss, want, label in sets:
        tmax = np.where(hit, t_hit, t_miss).astype(f32)
        for mode in MODES:
            assert_occluded(rt.occluded(c.run.dev, rays, tmax, traversal=mode), want, f"{what} mode {mode} {label}")


@pytest.mark.parametrize("kind", oref.THRESHOLD_KINDS)
@pytest.mark.parametrize("name", SCENES)
def test_threshold_is_s_bit_for_bit(name, kind):
    c = tq.case(name)
    if kind == "inbox":
        assert 0.25 <= hit_and_s(c, kind)[0].mean() <= 0.98
    if kind == "gate:4":  # unnormalised, outside the gate: the plain KD traversal in either mode
        assert (np.abs(c.rays(kind)[:, 3:]).max(axis=1) > 2).all()
    check_thresholds(c, kind, f"{name} {kind}")


# ------------------------------------------------------------------ 3. bisection
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_bisection_finds_s(name, mode):
    """independent of the restatement's use as an input: 31 batched calls bisect
    tmax over the positive float bit patterns [+0, +inf] per ray; the largest
    tmax answered 0 is s, bit for bit, and the answers along the way are
    monotone in tmax"""
    c = tq.case(name)
    hit, s = hit_and_s(c, "inbox")
    idx = np.nonzero(hit)[0][:256]
    assert len(idx) == 256
    rays = c.rays("inbox")[idx]
    lo = np.zeros(256, np.uint32)  # answered 0
    hi = np.full(256, 0x7F800000, np.uint32)  # answered 1
    assert not rt.occluded(c.run.dev, rays, lo.view(f32), traversal=mode).any()
    assert rt.occluded(c.run.dev, rays, hi.view(f32), traversal=mode).all()
    asked, answers = [], []
    for _ in range(31):
        mid = ((lo.astype(np.uint64) + hi) // 2).astype(np.uint32)
        occ = rt.occluded(c.run.dev, rays, mid.view(f32), traversal=mode).astype(bool)
        asked.append(mid.copy())
        answers.append(occ.copy())
        hi = np.where(occ, mid, hi)
        lo = np.where(occ, lo, mid)
    assert (hi - lo == 1).all()
    bad = np.nonzero(lo != s[idx].view(np.uint32))[0]
    assert len(bad) == 0, (len(bad), lo[bad[:4]].view(f32), s[idx][bad[:4]])
    asked, answers = np.array(asked), np.array(answers)  # (positive floats order as their bit patterns)
    assert np.array_equal(answers, asked > lo[None, :])


# ------------------------------------------------------------------ 4. special tmax
@pytest.mark.parametrize("name", SCENES)
def test_special_tmax(name):
    c = tq.case(name)
    hit, s = hit_and_s(c, "inbox")
    rays = c.rays("inbox")[hit]
    sh = s[hit]
    never = [f32(np.nan), f32(0.0), f32(-0.0), f32(1e-5), f32(1e-42), f32(-1.0), -INF]
    assert never[4] > 0 and never[4] < np.finfo(f32).tiny  # a denormal
    for mode in MODES:
        for t in never:
            assert not rt.occluded(c.run.dev, rays, t, traversal=mode).any(), (mode, t)
        mixed = np.array(never, f32)[np.arange(len(rays)) % len(never)]
        assert not rt.occluded(c.run.dev, rays, mixed, traversal=mode).any(), mode
        t = np.nextafter(f32(1e-5), INF)
        assert_occluded(rt.occluded(c.run.dev, rays, t, traversal=mode), sh < t, f"nextafter(1e-5f) mode {mode}")
        assert rt.occluded(c.run.dev, rays, INF, traversal=mode).all()  # (rays known to hit)


# ------------------------------------------------------------------ 5. shapes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 257, 300_000])
def test_shapes_and_untouched_surroundings(n):
    """every n around the wave and block sizes and more rays than the resident
    grid has threads; the output starts at an odd byte offset inside a buffer
    of 0xA5 bytes, and every byte outside [offset, offset + n) stays 0xA5"""
    c = tq.case("cornell")
    g = np.random.default_rng(200 + n % 97)
    rays = np.concatenate([tq._inbox(g, c, n), tq._unit(g, n)], axis=1).astype(f32).reshape(n, 6)
    ref = c.osc.trace_rays(rays) if n else np.zeros((0, 12), f32)
    hit = ref[:, 0] == 1
    s = oref.s_reference(c.tris, rays, np.where(hit, ref[:, 1], -1)) if n else np.zeros(0, f32)
    diag = float(np.linalg.norm(c.bounds[3:] - c.bounds[:3]))
    tmax = g.uniform(1e-3 * diag, 0.6 * diag, n).astype(f32)
    want = hit & (s < tmax)
    if n >= 255:
        assert 0.1 * n < want.sum() < hit.sum() < n  # both the hit flag and the threshold decide
    off, pad = 3, 129
    L = rt.lib()
    for mode in MODES:
        d_rays, d_tmax = tq.Dev(rays), tq.Dev(tmax)
        d_out = tq.Dev(np.full(off + n + pad, 0xA5, np.uint8))
        d_stats = tq.Dev(np.zeros(3, np.uint64))
        try:
            out_ptr = d_out.p.value + off
            assert out_ptr % 2 == 1
            rt.occluded_device(c.run.dev, d_rays.p, d_tmax.p, n, out_ptr, traversal=mode, stats_ptr=d_stats.p)
            out, stats = d_out.read(), d_stats.read()
            o = rt.query_options(traversal=mode)
            assert L.rt_occluded(c.run.dev.prepared, d_rays.p, d_tmax.p.value + 2, n, out_ptr,
                                 ctypes.byref(o)) == E_INVALID  # a misaligned tmax pointer
            assert np.array_equal(d_out.read(), out)  # (and nothing was written)
        finally:
            for d in (d_rays, d_tmax, d_out, d_stats):
                d.free()
        assert (out[:off] == 0xA5).all() and (out[off + n:] == 0xA5).all(), "bytes outside the output written"
        assert_occluded(out[off:off + n], want, f"n = {n} mode {mode}")
        # (unit directions from inside the box: all inside the gate; tmax > 1e-5 on every ray here)
        assert (tmax > f32(1e-5)).all()
        assert list(stats) == [n, int(want.sum()), n if mode == rt.TRAVERSAL_KD else 0], (n, stats)


# ------------------------------------------------------------------ 6. stats
@pytest.mark.parametrize("scale", list(tq.GATE_SCALES))
@pytest.mark.parametrize("name", SCENES)
def test_stats_and_gate_accounting(name, scale):
    """stats: [0] rays, [1] occluded rays, [2] rays that ran the plain KD
    traversal — exactly the rays with max|d_i| outside [0.5, 2] in the bounded
    mode; a ray with tmax <= 1e-5 counts in [0] only"""
    c = tq.case(name)
    kind = "gate:" + scale
    rays, ref = c.rays(kind), c.ref(kind)
    d = np.abs(rays[:, 3:])
    assert (d != 0).all() and np.isfinite(rays).all()  # so rt_bounded_ray admits every one of them
    m = d.max(axis=1)
    out_of_gate = (m < f32(0.5)) | (m > f32(2.0))
    outside = int(out_of_gate.sum())
    if scale in ("1", "2"):
        assert outside == 0
    if scale in ("2^-80", "0.25", "4"):
        assert outside == N
    hit = ref[:, 0] == 1
    nhits = int(hit.sum())
    occ, st = rt.occluded(c.run.dev, rays, traversal=rt.TRAVERSAL_BOUNDED, stats=True)
    print(f"{name} scale {scale}: outside the gate {outside}, stats {st}")
    assert_occluded(occ, hit, kind)
    assert st == {"rays": N, "occluded": nhits, "kd_rays": outside}, (st, outside, nhits)
    occ, st = rt.occluded(c.run.dev, rays, traversal=rt.TRAVERSAL_KD, stats=True)
    assert st == {"rays": N, "occluded": nhits, "kd_rays": N}, st
    # every third ray rejected by the tmax rule: not traced, counted in [0] only
    rejected = np.arange(N) % 3 == 0
    low = np.array([1e-5, 0.0, -2.0, np.nan], f32)[np.arange(N) % 4]
    tmax = np.where(rejected, low, INF).astype(f32)
    want = hit & ~rejected
    occ, st = rt.occluded(c.run.dev, rays, tmax, traversal=rt.TRAVERSAL_BOUNDED, stats=True)
    assert_occluded(occ, want, kind + " with rejected rays")
    assert st == {"rays": N, "occluded": int(want.sum()), "kd_rays": int((out_of_gate & ~rejected).sum())}, st
    occ, st = rt.occluded(c.run.dev, rays, tmax, traversal=rt.TRAVERSAL_KD, stats=True)
    assert_occluded(occ, want, kind + " with rejected rays, KD")
    assert st == {"rays": N, "occluded": int(want.sum()), "kd_rays": int((~rejected).sum())}, st


# ------------------------------------------------------------------ 7. hazard geometry
@pytest.mark.parametrize("variant", ["degenerate", "duplicate"])
def test_hazard_geometry(tmp_path, variant):
    """zero-area triangles and a duplicated quad (two passing tests at exactly
    the same s: the tie takes the whole-leaf path): the thresholds of test 2"""
    extra = hazards.DEGENERATE_OBJ if variant == "degenerate" else hazards.DUPLICATE_OBJ
    c = tq._Case(hazards.cornell_variant(str(tmp_path / variant), variant, yaw_room=0.1, extra_obj=extra))
    ref = c.ref("inbox")
    assert 0.25 <= (ref[:, 0] == 1).mean() <= 0.98
    if variant == "duplicate":
        assert ((ref[:, 1] >= len(c.tris) - 4) & (ref[:, 0] == 1)).sum() > 50
    check_thresholds(c, "inbox", variant)


# ------------------------------------------------------------------ 8. between chained renders
def test_occluded_between_chained_renders():
    """two chained rt_render calls (overlap = 1) with rt_occluded calls on
    another stream between them: the frame is the one without the queries, and
    the queries' results are the standalone ones"""
    c = tq.case("room_small")
    W, H, P = 96, 54, 4
    rays = c.rays("inbox")
    hit, s = hit_and_s(c, "inbox")
    g = np.random.default_rng(32)
    tmax = np.where(hit, s * np.exp2(g.uniform(-2.0, 2.0, N)).astype(f32), INF).astype(f32)
    alone = [rt.occluded(c.run.dev, rays), rt.occluded(c.run.dev, rays, tmax)]
    assert_occluded(alone[0], hit, "standalone")
    assert_occluded(alone[1], hit & (s < tmax), "standalone with tmax")
    s_render, s_query = tq._stream(), tq._stream()

    def frame(with_query):
        gb = rt.GBuffer(W, H)
        d_rays, d_tmax = tq.Dev(rays), tq.Dev(tmax)
        d_a, d_b = tq.Dev(np.full(N + 64, 0xA5, np.uint8)), tq.Dev(np.full(N + 64, 0xA5, np.uint8))
        try:
            for k in range(2):
                opt = rt.options(W, H, P, adaptive=False, kernel=rt.KERNEL_WAVEFRONT, overlap=True,
                                 coalesce_passes=-1, stream=s_render.value)
                rt.render(c.run.dev, gb, c.run.camera, 0 if k == 0 else 1, opt)
                if with_query and k == 0:
                    rt.occluded_device(c.run.dev, d_rays.p, None, N, d_a.p, stream=s_query.value)
                    rt.occluded_device(c.run.dev, d_rays.p, d_tmax.p, N, d_b.p, stream=s_query.value)
            rt.join()
            assert tq._HIP.hipStreamSynchronize(s_query) == 0
            return gb.download(), d_a.read(), d_b.read()
        finally:
            for d in (d_rays, d_tmax, d_a, d_b):
                d.free()
            gb.free()

    plain, _, _ = frame(False)
    mixed, a, b = frame(True)
    tq.helpers.assert_bitwise(mixed, plain, what="chained frame with occlusion queries in between")
    assert int(plain[2].sum()) == W * H * P * 2
    assert np.array_equal(a[:N], alone[0]) and np.array_equal(b[:N], alone[1])
    assert (a[N:] == 0xA5).all() and (b[N:] == 0xA5).all()
    for st in (s_render, s_query):
        assert tq._HIP.hipStreamDestroy(st) == 0


# ------------------------------------------------------------------ 9. torch
def test_torch_tensors_on_the_current_stream():
    """rays, tmax and the output in torch device tensors, the query enqueued on
    torch's current stream (rt.occluded_device): the numpy path's answers.  In a
    child process that imports torch first (tests/occlusion_torch_child.py)."""
    pytest.importorskip("torch")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "occlusion_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-4000:]
