"""The occlusion query (rt_occluded, include/isaklm_rt.h ABI 12) without a
GPU: argument errors are reported before any device call, the binding has the
header's signature, and the traversal of csrc/query.hip / csrc/bvh_trace.h
(the tmax rule, the domain gate, the s_min query capped at min(root exit,
tmax), the early "no", the bounded KD phase) equals its definition —
(trace_ray hits) && (s < tmax) — on the host restatement
(tests/native/occlusion_check.cpp, the device code's float operations), for
rays inside the gate, at its edges and outside it, on plain and on hazard
geometry.  It also pins the s the GPU tests compare with (occlusion_ref.
s_reference, numpy) to the checker's plain-KD restatement, bit for bit.  The
kernel itself is compared with the oracle in tests/test_gpu_occlusion.py.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hazards
import helpers
import occlusion_ref as oref
import oracle
import rt
import test_gpu_query as tq
from test_query_cpu import _rescaled

f32 = np.float32
E_INVALID = -1


def test_abi_version_and_signature():
    text = open(os.path.join(helpers.ROOT, "include", "isaklm_rt.h")).read()
    assert int(re.search(r"#define RT_ABI_VERSION (\d+)", text).group(1)) == 12
    assert rt.ABI_VERSION == 12 and rt.lib().rt_abi_version() == 12
    m = re.search(r"int rt_occluded\(([^;]*)\);", text)
    assert m, "rt_occluded is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["rt_scene_t scene", "const float *rays_device", "const float *tmax_device", "long long n",
                      "uint8_t *occluded_device", "const RtQueryOptions *opt"]
    L = rt.lib()
    vp = ctypes.c_void_p
    assert L.rt_occluded.argtypes == [vp, vp, vp, ctypes.c_longlong, vp, ctypes.POINTER(rt.RtQueryOptions)]
    assert L.rt_occluded.restype is ctypes.c_int
    assert rt.OCCLUSION_STATS == ("rays", "occluded", "kd_rays")


def test_argument_errors_without_a_device():
    """Every rejected call returns RT_E_INVALID before it looks at the scene or
    the device: the scene handle below is not a scene and the pointers are not
    device memory."""
    L = rt.lib()
    fake_scene, good = 0x1000, 0x2000  # never dereferenced by a rejected call
    o = rt.query_options()
    cases = [
        (None, good, good, 4, good, "null scene"),
        (None, good, None, 4, good, "null scene, no tmax"),
        (fake_scene, None, good, 4, good, "null rays"),
        (fake_scene, good, good, 4, None, "null output"),
        (fake_scene, good, None, -1, good, "n < 0"),
        (fake_scene, good, good, 1 << 31, good, "n > 2^31 - 1"),
        (fake_scene, good + 4, good, 4, good, "rays not 8-B aligned"),
        (fake_scene, good, good + 2, 4, good, "tmax not 4-B aligned"),
        (fake_scene, good, good + 1, 4, good + 1, "tmax not 4-B aligned (odd)"),
    ]
    for scene, rays, tmax, n, out, what in cases:
        assert L.rt_occluded(scene, rays, tmax, n, out, ctypes.byref(o)) == E_INVALID, what
        assert L.rt_last_error(), what
        assert L.rt_occluded(scene, rays, tmax, n, out, None) == E_INVALID, what  # (default options)
    with pytest.raises(ValueError):
        rt.occluded(None, np.zeros((4, 5), f32))
    with pytest.raises(ValueError):
        rt.occluded(None, np.zeros((4, 6), f32), tmax=np.zeros(3, f32))


# ---- the traversal on the host restatement ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return oref.build_checker(tmp_path_factory.mktemp("occlusion"))


class _CpuCase:
    """test_gpu_query._Case without the device: the oracle's scene and the seeded ray sets"""

    def __init__(self, path):
        self.path = path
        self.osc = oracle.OracleScene(path)
        arr = self.osc.arrays()
        self.tris = np.frombuffer(arr[0], np.uint8).reshape(-1, 152)
        self.bounds = arr[4].astype(f32)
        self._sets = {}

    def rays(self, kind, n=tq.N):
        if (kind, n) not in self._sets:
            self._sets[kind, n] = tq.make_rays(self, kind) if n == tq.N else tq.make_rays(self, kind, n)
        return self._sets[kind, n]


def _run_check(checker, scene, rays, tmp_path):
    f = str(tmp_path / "rays.f32")
    np.ascontiguousarray(rays, dtype=f32).tofile(f)
    r = subprocess.run([checker, scene, "check", f], capture_output=True, text=True, timeout=300)
    m = re.search(r"rays (\d+) hits (\d+) cases (\d+) occluded (\d+) mismatches (\d+); early (\d+) kd-phase (\d+) "
                  r"plain (\d+) untraced (\d+); T\* leaves (\d+), ties (\d+)", r.stdout)
    assert m, r.stdout[-2000:] + r.stderr[-2000:]
    keys = ("rays", "hits", "cases", "occluded", "mismatches", "early", "kd_phase", "plain", "untraced", "fast", "ties")
    st = dict(zip(keys, (int(x) for x in m.groups())))
    print(scene, st)
    assert r.returncode == (0 if st["mismatches"] == 0 else 1), r.stdout[-2000:]
    return st, r.stdout


@pytest.mark.parametrize("name", ["cornell", "room_small"])
def test_restatement_equals_the_definition(checker, tmp_path, name):
    """1,024 seeded rays per set: in-box unit directions, max|d_i| exactly 0.5 and
    exactly 2 (the gate's edges), scales outside the gate (0.25, 4, 2^-80),
    origins outside the box, rays in the root split plane, axis-parallel and
    non-finite rays — each with ~24 tmax values around its own s, in both
    traversal modes: 0 mismatches, and every path was taken"""
    c = _CpuCase(helpers.scene_path(name))
    n = 1024
    g = np.random.default_rng(2025)
    inbox = c.rays("inbox")[:n]
    sets = [inbox]
    for target in (f32(0.5), f32(2.0)):
        d = _rescaled(g, inbox[:, 3:], target)
        assert np.array_equal(np.abs(d).max(axis=1), np.broadcast_to(target, (n,)))
        sets.append(np.concatenate([inbox[:, :3], d], axis=1))
    for scale in ("0.25", "4", "2^-80"):
        sets.append(c.rays("gate:" + scale)[:n])
    for kind in ("outside", "split", "axis"):
        sets.append(c.rays(kind)[:n])
    sets.append(c.rays("special"))
    rays = np.concatenate(sets).astype(f32)
    st, out = _run_check(checker, c.path, rays, tmp_path)
    assert st["rays"] == len(rays) and st["mismatches"] == 0, out[-2000:]
    # not trivial: hits and misses, occluded and unoccluded answers, and every branch of the kernel
    assert 0.2 * len(rays) < st["hits"] < 0.98 * len(rays), st
    assert 0.1 * st["cases"] < 2 * st["occluded"] < 0.9 * st["cases"], st
    for key in ("early", "kd_phase", "plain", "untraced", "fast"):
        assert st[key] > 1000, (key, st)


@pytest.mark.parametrize("variant", ["degenerate", "duplicate"])
def test_restatement_on_hazard_geometry(checker, tmp_path, variant):
    """zero-area triangles (NaN planes) and a duplicated quad: two passing tests
    at exactly the same s, where the query marks a tie and the KD phase scans
    the whole leaf instead of T*'s entry"""
    extra = hazards.DEGENERATE_OBJ if variant == "degenerate" else hazards.DUPLICATE_OBJ
    c = _CpuCase(hazards.cornell_variant(str(tmp_path / variant), variant, yaw_room=0.1, extra_obj=extra))
    rays = c.rays("inbox")
    st, out = _run_check(checker, c.path, rays, tmp_path)
    assert st["rays"] == len(rays) and st["mismatches"] == 0, out[-2000:]
    assert 0.25 * len(rays) <= st["hits"] <= 0.98 * len(rays)
    if variant == "duplicate":
        assert st["ties"] > 500, st  # (every capped query of a ray on the quad that passes its s: a tie)


def _pin(checker, c, kinds, tmp_path):
    total = 0
    for kind in kinds:
        rays = c.rays(kind)
        ref = c.osc.trace_rays(rays)
        dump = oref.checker_dump(checker, c.path, rays, tmp_path)
        hit = ref[:, 0] == 1
        assert np.array_equal(dump["hit"] == 1, hit), kind
        assert np.array_equal(dump["triangle"][hit], ref[hit, 1].astype(np.int32)), kind
        s = oref.s_reference(c.tris, rays, np.where(hit, ref[:, 1], -1))
        bad = np.nonzero(s.view(np.uint32)[hit] != dump["s"].view(np.uint32)[hit])[0]
        assert len(bad) == 0, (kind, len(bad), s[hit][bad[:4]], dump["s"][hit][bad[:4]])
        assert np.isfinite(s[hit]).all() and (s[hit] >= f32(1e-5)).all()
        total += int(hit.sum())
    return total


@pytest.mark.parametrize("name", ["cornell", "room_small"])
def test_s_reference_is_the_checkers(checker, tmp_path, name):
    """the numpy restatement of rt/trace_ray.cuh:75-90 on the oracle's hit
    triangle == the s of the checker's plain KD traversal, bit for bit, on the
    GPU threshold tests' ray sets (and the oracle's hit and triangle are the
    checker's)"""
    c = _CpuCase(helpers.scene_path(name))
    assert _pin(checker, c, oref.THRESHOLD_KINDS, tmp_path) > 1000


@pytest.mark.parametrize("variant", ["degenerate", "duplicate"])
def test_s_reference_on_hazard_geometry(checker, tmp_path, variant):
    extra = hazards.DEGENERATE_OBJ if variant == "degenerate" else hazards.DUPLICATE_OBJ
    c = _CpuCase(hazards.cornell_variant(str(tmp_path / variant), variant, yaw_room=0.1, extra_obj=extra))
    assert _pin(checker, c, ("inbox",), tmp_path) > 1000
