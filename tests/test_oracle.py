"""Pinning the CPU oracle (oracle/rt_oracle.c) — CPU only.

Known answers used (the reference ships no tests; the comparison
with the reference's own source built as host C++ is tests/test_reference_cpu.py):
  * mt19937: the C++ standard's [rand.predef] check (10000th output of a
    default-constructed std::mt19937 is 4123659995) and the first outputs the
    reference produced when run in this container during the survey
    (3499211612, 581869302, 3890346734).
  * get_random_unilateral: an independent numpy restatement of
    rt/path_tracing.cuh:34-43.
  * load_material: the reference's own rt/materials/*.mat files (copied to
    tests/golden/materials/) parsed against numpy.float32 of the decimal text.
  * intersect_triangle / calculate_barycentric_coordinates: an independent
    float32 numpy restatement on hand-made triangles.
  * regression vectors in tests/golden/oracle_regression.json (make_golden.py).
"""
import json
import os
import sys

import numpy as np
import pytest

import helpers
import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)


def test_mt19937_known_answers():
    out = oracle.mt19937(10000)
    assert out[9999] == 4123659995  # C++ standard [rand.predef]
    assert list(out[:3]) == [3499211612, 581869302, 3890346734]  # SURVEY §8c reference run
    np.testing.assert_array_equal(oracle.mt19937(5, 9995), out[9995:])


def _pcg_numpy(state, n):
    """rt/path_tracing.cuh:34-43 restated with numpy uint32 arithmetic."""
    vals = []
    s = np.uint32(state)
    with np.errstate(over="ignore"):
        for _ in range(n):
            st = np.uint32(s * np.uint32(747796405) + np.uint32(2891336453))
            word = np.uint32(((st >> ((st >> np.uint32(28)) + np.uint32(4))) ^ st) * np.uint32(277803737))
            s = np.uint32((word >> np.uint32(22)) ^ word)
            vals.append(np.float32(s) / np.float32(4294967296.0))
    return np.array(vals, np.float32), int(s)


@pytest.mark.parametrize("seed", [0, 1, 3499211612, 0xFFFFFFFF, 0xDEADBEEF])
def test_pcg_rng_matches_independent_restatement(seed):
    a, sa = oracle.rng_sequence(seed, 64)
    b, sb = _pcg_numpy(seed, 64)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert sa == sb


def test_rng_can_return_one():
    """float(x)/UINT32_MAX rounds to 1.0 for the top 128 states."""
    # find a state whose next output is >= 2^32 - 128
    x = np.uint32(0xFFFFFFC0)
    assert np.float32(x) / np.float32(4294967296.0) == np.float32(1.0)


def _expected_materials(path):
    """decimal text -> float32 (std::stof is correctly rounded)."""
    mats, cur = {}, None
    for raw in open(path, encoding="utf-8-sig"):
        line = raw.rstrip("\n")
        if line.startswith("material "):
            cur = line[len("material "):]
            mats[cur] = [0.0] * 10
            continue
        if cur is None or not line.strip():
            cur = None if not line.strip() else cur
            continue
        t = line.split()
        m = mats[cur]
        if t[0] == "albedo":
            m[0:3] = [np.float32(x) for x in t[1:4]]
        elif t[0] == "emittance":
            m[3:6] = [np.float32(x) for x in t[1:4]]
        elif t[0] == "roughness":
            m[6] = np.float32(t[1])
        elif t[0] == "n":
            m[7] = np.float32(t[1])
        elif t[0] == "k":
            m[8] = np.float32(t[1])
        elif t[0] == "transparent":
            m[9] = 1.0
    return mats


@pytest.mark.parametrize("fname", sorted(os.listdir(os.path.join(GOLDEN, "materials"))))
def test_reference_material_files_parse(fname):
    path = os.path.join(GOLDEN, "materials", fname)
    expected = _expected_materials(path)
    assert expected
    for name, vals in expected.items():
        rc, got = oracle.load_material(path, name)
        if name == "wood" and fname == "chair.mat":
            # chair.mat starts with a UTF-8 BOM on an otherwise empty line; "material wood" still matches
            pass
        assert rc == 1, (fname, name)
        np.testing.assert_array_equal(got, np.array(vals, np.float32), err_msg=f"{fname}:{name}")


def _intersect_numpy(o, d, p1, p2, p3):
    """rt/trace_ray.cuh:48-113 in float32 numpy (independent restatement)."""
    f = np.float32
    o, d, p1, p2, p3 = (np.asarray(v, np.float32) for v in (o, d, p1, p2, p3))

    def dot(a, b):
        return f(f(f(a[0] * b[0]) + f(a[1] * b[1])) + f(a[2] * b[2]))

    def cross(a, b):
        return np.array([f(a[1] * b[2]) - f(a[2] * b[1]), f(a[2] * b[0]) - f(a[0] * b[2]),
                         f(a[0] * b[1]) - f(a[1] * b[0])], np.float32)

    n = cross(p2 - p1, p3 - p1)
    r = f(f(1.0) / np.sqrt(f(f(f(n[0] * n[0]) + f(n[1] * n[1])) + f(n[2] * n[2]))))
    n = (n * r).astype(np.float32)
    dn = dot(d, n)
    if dn == 0:
        return None
    s = f(f(dot(n, p1) - dot(o, n)) / dn)
    if s < f(0.00001):
        return None
    p = (o + (d * s).astype(np.float32)).astype(np.float32)
    v0, v1, v2 = p2 - p1, p3 - p1, p - p1
    d00, d01, d11, d20, d21 = dot(v0, v0), dot(v0, v1), dot(v1, v1), dot(v2, v0), dot(v2, v1)
    rd = f(f(1.0) / f(f(d00 * d11) - f(d01 * d01)))
    by = f(f(f(d11 * d20) - f(d01 * d21)) * rd)
    bz = f(f(f(d00 * d21) - f(d01 * d20)) * rd)
    bx = f(f(f(1.0) - by) - bz)
    if 0 <= bx <= 1 and 0 <= by <= 1 and 0 <= bz <= 1:
        return s, (bx, by, bz)
    return None


def _single_triangle_scene(p1, p2, p3):
    import ctypes

    buf = bytearray(152)
    vals = list(p1) + list(p2) + list(p3) + [0, 0, 1] * 3 + [1.0] * 6
    buf[:len(vals) * 4] = np.array(vals, np.float32).tobytes()
    # material: albedo 0.5, roughness 0.5, n 1.5
    np.frombuffer(buf, np.float32, count=10, offset=96)[:] = [0.5, 0.5, 0.5, 0, 0, 0, 0.5, 1.5, 0, 0]
    return oracle.OracleScene(triangles=bytes(buf), count=1)


def test_ray_triangle_matches_independent_restatement():
    rng = np.random.default_rng(7)
    for _ in range(40):
        p1, p2, p3 = rng.uniform(-1, 1, (3, 3)).astype(np.float32)
        sc = _single_triangle_scene(p1, p2, p3)
        o = rng.uniform(-3, 3, (64, 3)).astype(np.float32)
        tgt = (p1 + p2 + p3) / 3 + rng.normal(0, 0.4, (64, 3)).astype(np.float32)
        d = tgt - o
        d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
        out = sc.trace_rays(np.hstack([o, d]))
        for i in range(64):
            ref = _intersect_numpy(o[i], d[i], p1, p2, p3)
            if ref is None:
                continue  # the KD/bbox path may or may not reach the triangle; checked below when hit
            if out[i, 0] == 1.0:
                s, (bx, by, bz) = ref
                pos = (bx * p1.astype(np.float32) + by * p2 + bz * p3).astype(np.float32)
                np.testing.assert_allclose(out[i, 2:5], pos, rtol=1e-5, atol=1e-5)
        hits = out[:, 0] == 1.0
        for i in np.nonzero(hits)[0]:
            assert _intersect_numpy(o[i], d[i], p1, p2, p3) is not None


def test_regression_vectors():
    gold = json.load(open(os.path.join(GOLDEN, "oracle_regression.json")))
    import make_golden

    for name, g in gold["scenes"].items():
        sc = oracle.OracleScene(helpers.scene_path(name))
        tris, nodes, idx, lights, bounds = sc.arrays()
        assert sc.nnodes == g["nodes"] and sc.nindices == g["indices"] and sc.ntris == g["triangles"]
        assert make_golden.sha(nodes) == g["nodes_sha256"], name
        assert make_golden.sha(idx.tobytes()) == g["indices_sha256"], name
        assert make_golden.sha(tris) == g["triangles_sha256"], name
    for key, g in gold["renders"].items():
        name, W, H, P, calls, adaptive, ms, md, skip = g["case"]
        (fb, sq, cnt, rng), counters = helpers.oracle_render(helpers.scene_path(name), W, H, P, calls=calls,
                                                             adaptive=adaptive, min_samples=ms, max_depth=md,
                                                             seed_skip=skip)
        assert make_golden.accum_digest(fb, sq, cnt, rng) == g["sha256"], key
        assert counters == g["counters"], key


def test_tonemap_math_against_numpy():
    """correct_color (rt/math_library.cuh:445-460) vs a float32/float64 numpy restatement (±1 ulp of powf)."""
    f = np.float32
    rng = np.random.default_rng(3)
    for c in rng.uniform(0, 4, (200, 3)).astype(np.float32):
        got = oracle.correct_color(c)
        x = np.maximum(c, 0).astype(np.float32)
        m_in = np.array([[0.59719, 0.35458, 0.04823], [0.07600, 0.90834, 0.01566], [0.02840, 0.13383, 0.83777]],
                        np.float32)
        m_out = np.array([[1.60475, -0.53108, -0.07367], [-0.10208, 1.10813, -0.00605], [-0.00327, -0.07276, 1.07602]],
                         np.float32)
        y = (m_in.astype(np.float64) @ x).astype(np.float32)
        y = ((y * (y + f(0.0245786)) - f(0.000090537)) / (y * (f(0.983729) * y + f(0.4329510)) + f(0.238081)))
        y = (m_out.astype(np.float64) @ y.astype(np.float32)).astype(np.float32)
        g = np.where(y > 0.0031308, 1.055 * np.power(y.astype(np.float64), float(f(1 / 2.4))) - 0.055,
                     12.92 * y.astype(np.float64)).astype(np.float32)
        ref = np.clip(g, 0, 1)
        np.testing.assert_allclose(got, ref, atol=2e-6)
