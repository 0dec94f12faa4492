"""The adaptive samplers' and the convergence query's CPU tier: rt_convergence_host
pinned to the oracle's own adaptive test (which pixels the oracle samples on
one more pass), the relative-error map against a float32 numpy restatement,
hostile elements, and the argument validation of rt_sample_paths_adaptive,
rt_convergence and rt_convergence_host — none of which needs a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import helpers
import oracle
import rt

f32 = np.float32
E_INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

W, H, PASSES, MIN_SAMPLES, TOLERANCE = 96, 54, 16, 4, 0.3

_frames = {}


def oracle_frame(scene):
    """the oracle's adaptive frame (fb, sq, count, rng) after PASSES passes, and its counts after one more pass;
    computed once per scene and never modified"""
    if scene not in _frames:
        path = helpers.scene_path(scene)
        sc = oracle.OracleScene(path)
        (fb, sq, cnt, rng), _ = helpers.oracle_render(path, W, H, PASSES, adaptive=True, min_samples=MIN_SAMPLES,
                                                      tolerance=TOLERANCE, scene=sc)
        fb2, sq2, cnt2, rng2 = fb.reshape(-1).copy(), sq.copy(), cnt.copy(), rng.copy()
        sc.render(sc.camera, fb2, sq2, cnt2, rng2, W, H, 1, sample_count_arg=1, adaptive=True,
                  min_samples=MIN_SAMPLES, tolerance=TOLERANCE, max_depth=0)
        for a in (fb, sq, cnt, rng, cnt2):
            a.setflags(write=False)
        _frames[scene] = (fb, sq, cnt, rng, cnt2)
    return _frames[scene]


def test_header_and_binding():
    text = open(os.path.join(INC, "isaklm_rt.h")).read()
    assert int(re.search(r"#define RT_ABI_VERSION (\d+)", text).group(1)) == 12
    assert rt.ABI_VERSION == 12 and rt.lib().rt_abi_version() == 12
    assert re.search(r"^#define RT_HAS_ADAPTIVE_SAMPLERS 1$", text, re.M)
    assert re.search(r"^#define RT_HAS_CONVERGENCE 1$", text, re.M)
    for fn in ("rt_sample_paths_adaptive", "rt_convergence", "rt_convergence_host"):
        assert re.search(rf"int {fn}\(", text) and hasattr(rt.lib(), fn)
    assert [n for n, _ in rt.RtAdaptive._fields_] == ["min_samples", "tolerance"]
    assert ctypes.sizeof(rt.RtAdaptive) == 8
    # no existing struct grew
    assert ctypes.sizeof(rt.RtPathOptions) == 32 and ctypes.sizeof(rt.RtSampler) == 64


@pytest.mark.parametrize("scene", ["cornell", "room_small"])
def test_open_set_is_the_oracles(scene):
    """`open` is the set of pixels the oracle samples on its next pass; the cases are not trivial: each of the three
    classes (stopped at min_samples, stopped in between, never stopped) holds at least 5 % of the pixels."""
    fb, sq, cnt, _, cnt_next = oracle_frame(scene)
    n = W * H
    at_min, never = int((cnt == MIN_SAMPLES).sum()), int((cnt == PASSES).sum())
    between = n - at_min - never
    print(f"{scene}: never stopped {never}, stopped at min_samples {at_min}, stopped in between {between} of {n}")
    assert cnt.min() >= MIN_SAMPLES and cnt.max() <= PASSES
    assert min(at_min, never, between) >= 0.05 * n
    sampled = cnt_next != cnt
    assert np.array_equal(cnt_next[sampled], cnt[sampled] + 1)
    stats, err = rt.convergence_host(fb, sq, cnt, MIN_SAMPLES, TOLERANCE, rel_error=True)
    assert stats["elements"] == n and stats["below_min"] == 0
    assert stats["open"] == int(sampled.sum())
    assert stats["samples"] == int(cnt.astype(np.int64).sum())
    # the open mask itself: the test asked of every pixel alone
    mask = np.array([rt.convergence_host(fb[i], sq[i:i + 1], cnt[i:i + 1], MIN_SAMPLES, TOLERANCE)["open"]
                     for i in range(n)], dtype=bool)
    assert np.array_equal(mask, sampled)
    # every pixel that stopped before the last pass is closed, and stays closed
    assert not sampled[cnt < PASSES].any()
    # with a higher min_samples every pixel below it is open, whatever its interval
    more = rt.convergence_host(fb, sq, cnt, PASSES, TOLERANCE)
    assert more["below_min"] == int((cnt < PASSES).sum())
    assert more["open"] == more["below_min"] + int(sampled[cnt == PASSES].sum())


def restated(fb, sq, cnt, min_samples, tolerance):
    """adaptive_run's operations (rt/path_tracing.cuh:352-376) in float32 numpy, one rounding per operation, and
    the map's three cases.  z is the library's host constant, taken from an element built to expose it."""
    fb, sq = np.asarray(fb, f32).reshape(-1, 3), np.asarray(sq, f32)
    cnt = np.asarray(cnt, np.int32)
    with np.errstate(all="ignore"):
        tl = (fb[:, 0] * f32(0.2126) + fb[:, 1] * f32(0.7152)) + fb[:, 2] * f32(0.0722)
        c = cnt.astype(f32)
        mean = tl / c
        var = (sq - (tl * tl) / c) / (cnt.astype(np.int64) - 1).astype(f32)
        iw = f32(z_const(tolerance)) * np.sqrt(var / c)
        open_ = (cnt < min_samples) | (iw > mean * f32(tolerance))
        err = np.where(cnt < 2, f32(np.inf), np.where(iw > 0, iw / mean, f32(0)))
    return open_, err.astype(f32)


def z_const(tolerance):
    """sqrtf(2) * erfinvf(1 - tolerance) (rt/path_tracing.cuh:370): erfinvf(0.95f) correctly rounded for the
    reference's own tolerance, otherwise erf inverted by Newton steps in double and rounded once"""
    import math

    p = f32(1) - f32(tolerance)
    if p == f32(0.95):
        e = f32(1.3859037160873413)
    else:
        x = 0.0
        for _ in range(100):
            nx = x - (math.erf(x) - float(p)) / (1.1283791670955126 * math.exp(-x * x))
            if nx == x:
                break
            x = nx
        e = f32(x)
    return np.sqrt(f32(2)) * e


def test_luminance_restatement_matches_rt_dot():
    """(the restatement's luminance association is the library's: checked on the oracle frame, where a wrong
    association would flip bits of the map)"""
    fb, sq, cnt, _, _ = oracle_frame("cornell")
    want_open, want_err = restated(fb, sq, cnt, MIN_SAMPLES, TOLERANCE)
    _, err = rt.convergence_host(fb, sq, cnt, MIN_SAMPLES, TOLERANCE, rel_error=True)
    assert np.array_equal(err.view(np.uint32), want_err.view(np.uint32))


@pytest.mark.parametrize("tolerance", [0.05, 0.3, 0.9])
@pytest.mark.parametrize("min_samples", [0, 1, 2, 4, 100])
def test_rel_error_and_hostile_elements(min_samples, tolerance):
    """counts 0, 1, 2 and negative, NaN and infinite sums, black elements, a variance that rounds negative"""
    inf, nan = np.inf, np.nan
    rng = np.random.default_rng(7)
    fb = rng.random((64, 3), dtype=f32) * f32(8)
    sq = rng.random(64, dtype=f32) * f32(40)
    cnt = rng.integers(2, 40, 64).astype(np.int32)
    hostile_fb = [[0, 0, 0], [0, 0, 0], [1, 2, 3], [1, 2, 3], [1, 2, 3], [nan, 1, 1], [inf, 1, 1], [1, 1, -inf],
                  [1, 1, 1], [1, 1, 1], [4, 4, 4], [0, 0, 0], [2, 2, 2], [-1, -1, -1], [3e38, 3e38, 3e38]]
    hostile_sq = [0, 0, 5, 5, 5, 1, 1, 1, nan, inf, 1, 0, 0.5, 2, 3e38]
    hostile_cnt = [0, 5, 0, 1, 2, 4, 4, 4, 4, 4, 8, -3, 8, 4, 4]
    fb = np.concatenate([fb, np.array(hostile_fb, f32)])
    sq = np.concatenate([sq, np.array(hostile_sq, f32)])
    cnt = np.concatenate([cnt, np.array(hostile_cnt, np.int32)])
    stats, err = rt.convergence_host(fb, sq, cnt, min_samples, tolerance, rel_error=True)
    want_open, want_err = restated(fb, sq, cnt, min_samples, tolerance)
    assert np.array_equal(err.view(np.uint32), want_err.view(np.uint32)), (err, want_err)
    assert stats == {"elements": len(cnt), "open": int(want_open.sum()), "below_min": int((cnt < min_samples).sum()),
                     "samples": int(cnt.astype(np.int64).sum()) % 2**64}
    # the named cases: +inf below 2 samples, 0 for a black element and for a variance that rounds negative
    assert np.isposinf(err[cnt < 2]).all()
    assert err[64 + 1] == 0 and err[64 + 10] == 0
    # the map is a diagnostic: an element with a NaN interval is closed once it has min_samples, open below
    nan_iw = 64 + 5
    assert np.isnan(err[nan_iw]) or err[nan_iw] == 0
    assert bool(want_open[nan_iw]) == bool(cnt[nan_iw] < min_samples)


def test_min_samples_0_and_1_divide_by_count_minus_1():
    """cnt = 0: 0 / 0 is a NaN and fails the compare — the element stops; cnt = 1 divides by 0"""
    fb = np.array([[0, 0, 0], [1, 1, 1], [1, 1, 1]], f32)
    sq = np.array([0, 1, 0.5], f32)
    cnt = np.array([0, 1, 1], np.int32)
    for m in (0, 1):
        stats = rt.convergence_host(fb, sq, cnt, m, 0.05)
        want, _ = restated(fb, sq, cnt, m, 0.05)
        assert stats["open"] == int(want.sum()) and stats["below_min"] == int((cnt < m).sum())
    assert rt.convergence_host(fb[:1], sq[:1], cnt[:1], 0, 0.05)["open"] == 0
    assert rt.convergence_host(fb[:1], sq[:1], cnt[:1], 1, 0.05)["open"] == 1


def test_argument_errors_without_a_device():
    """Every rejected call returns RT_E_INVALID before it looks at the scene or the device: the scene handle is not
    a scene and the pointers are not device memory."""
    L = rt.lib()
    fake, good = 0x1000, 0x2000
    n = 12
    c = rt.Camera()
    c.FOV = 1.0
    smp = rt.RtSampler(rt.SAMPLER_PINHOLE, 4, 3, c, 1.0, None, None)

    def sample(scene=fake, rng=good, n=n, rad=good, sq=good, cnt=good, opt=None, ad=(4, 0.3), s=smp):
        a = rt.RtAdaptive(*ad) if ad is not None else None
        return L.rt_sample_paths_adaptive(scene, ctypes.byref(s) if s is not None else None, rng, n, rad, sq, cnt, opt,
                                          ctypes.byref(a) if a is not None else None)

    # what rt_sample_paths checks
    for change, what in ((dict(scene=None), "null scene"), (dict(rng=None), "null rng"), (dict(rad=None), "null radiance"),
                         (dict(n=-1), "n < 0"), (dict(n=1 << 31), "n > 2^31 - 1"), (dict(rng=good + 2), "rng misaligned"),
                         (dict(rad=good + 1), "radiance misaligned"), (dict(sq=good + 3), "sq misaligned"),
                         (dict(cnt=good + 2), "sample_count misaligned"), (dict(s=None), "null sampler"),
                         (dict(n=n + 1), "no pixel list and n != width * height")):
        for ad in ((4, 0.3), None):
            assert sample(ad=ad, **change) == E_INVALID, (what, ad)
            assert L.rt_last_error(), what
    for bad, what in ((dict(samples=-1), "samples < 0"), (dict(samples=(1 << 20) + 1), "samples > 2^20"),
                      (dict(max_depth=-1), "max_depth < 0"), (dict(accumulate=2), "accumulate 2"),
                      (dict(traversal=77), "traversal"), (dict(stats=good + 4), "stats not 8-B aligned")):
        assert sample(opt=ctypes.byref(rt.path_options(**bad))) == E_INVALID, what
    # the adaptive test's own
    assert sample(sq=None) == E_INVALID and b"rt_sample_paths_adaptive" in L.rt_last_error()
    assert sample(cnt=None) == E_INVALID
    assert sample(ad=(-1, 0.3)) == E_INVALID
    listed = rt.RtSampler(rt.SAMPLER_PINHOLE, 4, 3, c, 1.0, good, None)
    assert sample(s=listed, n=0, sq=None) == E_INVALID and sample(s=listed, n=0, ad=(-1, 0.3)) == E_INVALID
    # n == 0: RT_OK without a launch; the tolerance is taken unchecked; without `adaptive` the call is rt_sample_paths
    for tol in (0.3, 0.0, -1.0, 1e9, float("nan"), float("inf")):
        assert sample(s=listed, n=0, ad=(0, tol)) == 0
    assert sample(s=listed, n=0, ad=((1 << 31) - 1, 0.3)) == 0
    assert sample(s=listed, n=0, ad=None, sq=None, cnt=None) == 0

    def conv(rad=good, sq=good, cnt=good, n=n, m=4, tol=0.3, err=None, stats=None, host=False):
        if host:
            return L.rt_convergence_host(rad, sq, cnt, n, m, tol, err, stats)
        return L.rt_convergence(rad, sq, cnt, n, m, tol, err, stats, None)

    for host in (False, True):
        for change, what in ((dict(rad=None), "null radiance"), (dict(sq=None), "null sq"), (dict(cnt=None), "null count"),
                             (dict(n=-1), "n < 0"), (dict(n=1 << 31), "n > 2^31 - 1"), (dict(rad=good + 2), "radiance"),
                             (dict(sq=good + 1), "sq"), (dict(cnt=good + 3), "count"), (dict(err=good + 2), "map"),
                             (dict(stats=good + 4), "stats"), (dict(m=-1), "min_samples < 0")):
            assert conv(host=host, **change) == E_INVALID, (what, host)
            assert (b"rt_convergence_host" if host else b"rt_convergence:") in L.rt_last_error(), what
        assert conv(host=host, n=0) == 0  # RT_OK, no launch, nothing is looked at
        assert conv(host=host, n=0, tol=float("nan"), m=(1 << 31) - 1) == 0


def test_binding_argument_errors():
    smp = rt.Sampler("pinhole", 4, 3, rt.Camera())
    rng = np.zeros(12, np.uint32)
    for bad_call in (lambda: rt.sample_paths(None, smp, rng, adaptive=(4, 0.3), radiance=np.zeros((12, 3), f32)),
                     lambda: rt.sample_paths(None, smp, rng, adaptive=(4, 0.3), radiance=np.zeros((12, 3), f32),
                                             sq=np.zeros(12, f32)),
                     lambda: rt.sample_paths(None, smp, rng, adaptive=(4, 0.3), radiance=np.zeros((12, 3), f32),
                                             sq=np.zeros(12, f32), count=True),
                     lambda: rt.convergence_host(np.zeros((12, 3), f32), np.zeros(11, f32), np.zeros(12, np.int32), 4, 0.3),
                     lambda: rt.convergence_host(np.zeros((11, 3), f32), np.zeros(12, f32), np.zeros(12, np.int32), 4, 0.3)):
        with pytest.raises(ValueError):
            bad_call()
