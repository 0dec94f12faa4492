"""The oracle, the product's host side and the recorded fixtures against the
reference's own source.  CPU only.

oracle/_ref/libref_rt.so is the reference (INDA23PlusPlus/isaklm-raytracer)
compiled as host C++ from where it lies by oracle/Makefile.ref and driven by
oracle/ref_harness.cpp: IEEE arithmetic without contraction, the project's
transcendentals (csrc/rt_libm.h).  What it computes is what the oracle
(oracle/rt_oracle.c) restates, so the two are compared bit for bit here, and
its recorded results (tests/golden/reference/, cases: tests/reference_cases.py)
are what tests/test_gpu_reference.py holds the kernels to.

 a. the oracle vs the live reference: scene bytes, trace_ray,
    get_scattered_light, sample_direct_light, correct_color and the display
    bytes, the G-buffer seeds, every frame case;
 b. the product's host side (load_mesh, create_kd_tree) vs the live reference;
 c. the fixtures are fresh: regenerating each case live gives the committed
    arrays and hashes;
 d. the fixtures equal the oracle (needs no reference: this part also runs
    where no copy of the reference is present).

Tests a-c need the live library; they skip only where neither the library nor a
copy of the reference to build it from is present.
"""
import json
import os

import numpy as np
import pytest

import oracle
import reference
import reference_cases as rc
import test_independent as ti

f32 = np.float32
_cache = {}


@pytest.fixture(scope="session")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("reference_cases"))


@pytest.fixture(scope="session")
def live(workdir):
    """the live reference library, or a skip where it cannot exist"""
    if not reference.available():
        if oracle.reference_source() is None:
            pytest.skip("no copy of the reference is present, and oracle/_ref/libref_rt.so was not built from one")
        oracle.build()
    assert reference.lib().ref_uses_rt_libm() == 1
    return reference


def _case_dir(workdir, name):
    d = os.path.join(workdir, name)
    os.makedirs(d, exist_ok=True)
    return d


def live_record(workdir, name):
    """(case, arrays) of one case on the live reference, computed once"""
    if ("live", name) not in _cache:
        _cache["live", name] = rc.record(name, _case_dir(workdir, name))
    return _cache["live", name]


def oracle_case(workdir, name):
    """(case, frames, counters) of one case on the oracle, computed once"""
    if ("oracle", name) not in _cache:
        case = rc.Case(name, _case_dir(workdir, name), oracle.OracleScene)
        counters = {}
        _cache["oracle", name] = (case, rc.run_frames(case, counters=counters), counters)
    return _cache["oracle", name]


def assert_same_scene(got, want, what, lights=True):
    gt, gn, gi, gl, gb = got
    wt, wn, wi, wl, wb = want
    assert gt.shape == wt.shape, (what, "triangle count", gt.shape, wt.shape)
    bad = np.nonzero((gt != wt).any(axis=1))[0]
    assert len(bad) == 0, (what, "triangles differ", len(bad), bad[:8], np.nonzero(gt[bad[0]] != wt[bad[0]])[0])
    assert len(gn) == len(wn) and gn == wn, (what, "KD nodes differ", len(gn) // 20, len(wn) // 20)
    assert np.array_equal(gi, wi), (what, "triangle indices differ")
    if lights:
        assert np.array_equal(gl, wl), (what, "light list differs", gl, wl)
    assert gb.tobytes() == wb.tobytes(), (what, "bounds differ", gb, wb)


def assert_same_frames(got, want, what):
    assert len(got) == len(want), what
    for c, (g, w) in enumerate(zip(got, want)):
        for key, a, b in zip(rc.G_NAMES, g, w):
            if not rc.same_bits(a, b):
                av, bv = a.reshape(len(a), -1), b.reshape(len(b), -1)
                bad = np.nonzero((av.view(np.uint32) != bv.view(np.uint32)).any(axis=1))[0]
                raise AssertionError(f"{what} call {c} {key}: {len(bad)} of {len(a)} pixels differ; first "
                                     f"{bad[:8]}: {a[bad[:3]]} vs {b[bad[:3]]}")


# ------------------------------------------------- a. oracle vs live reference
@pytest.mark.parametrize("name", rc.ALL_CASES)
def test_oracle_scene_equals_reference(live, workdir, name):
    """load_mesh, load_material, make_texture's texels, the light list, create_kd_tree and its bounding box"""
    case, _ = live_record(workdir, name)
    osc = oracle_case(workdir, name)[0].scene
    assert osc.camera.tobytes() == case.scene.camera.tobytes()
    assert_same_scene(rc.scene_bytes(osc), rc.scene_bytes(case.scene), name)


def test_oracle_seeds_equal_reference(live):
    """the G_Buffer constructor's std::mt19937 seeds"""
    for w, h in ((48, 36), (3, 3), (100, 7)):
        np.testing.assert_array_equal(live.seeds(w, h), oracle.mt19937(w * h))


def test_oracle_trace_ray_equals_reference(live, workdir):
    """trace_ray on the hazard ray set: hit flag, triangle, position, normal and tangent, the columns
    or_trace_rays reports; rays of every class must both hit and miss"""
    case, out = live_record(workdir, rc.RAY_CASE)
    got = oracle_case(workdir, rc.RAY_CASE)[0].scene.trace_rays(out["rays"])[:, :11]
    want = out["samples"][:, rc.SAMPLE_ORACLE_COLUMNS]
    bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all(axis=1))[0]
    assert len(bad) == 0, (len(bad), bad[:8], got[bad[:3]], want[bad[:3]])
    hit = out["samples"][:, 0] == 1
    assert 0.2 < hit.mean() < 0.98, hit.mean()


def test_oracle_scatter_equals_reference(live):
    """get_scattered_light on the 60,000 inputs of test_independent.py"""
    N, d, nrm, tan, bit, albedo, rough, ior, ext, transparent, inside, pos, state = ti.scatter_inputs()
    smp = ti.scatter_samples(albedo, rough, ior, ext, transparent, pos, nrm, tan, bit)
    r_pos, r_dir, r_w, r_type, r_in, r_rng = live.scatter(d, smp, inside, state)
    o_dir, o_w, o_type, o_in, o_rng = ti.oracle_scatter(d, smp, inside, state)
    assert np.array_equal(o_type, r_type)
    assert np.array_equal(o_in, r_in)
    assert np.array_equal(o_rng, r_rng)
    bad = ~(ti._same(o_dir, r_dir).all(axis=1) & ti._same(o_w, r_w).all(axis=1))
    assert not bad.any(), (np.nonzero(bad)[0][:5], o_dir[bad][:2], r_dir[bad][:2], o_w[bad][:2], r_w[bad][:2])
    assert np.array_equal(r_pos.view(np.uint32), pos.view(np.uint32))  # the new ray starts at the sample
    for t in range(1, 5):  # DIFFUSE, SPECULAR, METALLIC, TRANSMISSION
        assert (r_type == t).sum() > 1000, t


def test_oracle_direct_light_equals_reference(live):
    """sample_direct_light at the shading points of test_independent.py"""
    osc, _, _, pos, nrm, state = ti.direct_light_inputs()
    rsc = live.ReferenceScene(rc._cornell(None))
    want, want_rng = rsc.direct_light(pos, nrm, state)
    got = np.zeros_like(want)
    got_rng = np.zeros_like(want_rng)
    for k in range(len(pos)):
        got[k], got_rng[k] = osc.direct_light(pos[k], nrm[k], int(state[k]))
    assert np.array_equal(got_rng, want_rng)
    assert ti._same(got, want).all(), np.nonzero(~ti._same(got, want).all(axis=1))[0][:8]
    lit = (want > 0).any(axis=1).sum()
    assert 0.2 * len(pos) < lit < len(pos)


def tonemap_domain():
    """colours over correct_color's whole domain: each channel log-spaced from denormal to 1e6 with the
    gamma curve's knee (0.0031308 after the ACES curve) inside, negatives, zeros, infinities, NaN, and the
    mean radiances a renderer produces (uniform and exponential triples)"""
    g = np.random.default_rng(7)
    grid = np.concatenate([f32(10.0) ** np.linspace(-45, 6, 4000, dtype=f32), [0.0, -0.0, -1.0, -1e-30, np.inf, -np.inf,
                                                                             np.nan, 1.0, 0.0031308, 3.4e38]]).astype(f32)
    grey = np.repeat(grid[:, None], 3, axis=1)
    mixed = g.choice(grid, (20000, 3))
    unit = g.uniform(0, 1, (60000, 3)).astype(f32)
    dark = (g.uniform(0, 1, (60000, 3)) * 0.02).astype(f32)  # around the knee
    bright = g.exponential(4.0, (40000, 3)).astype(f32)
    return np.concatenate([grey, mixed, unit, dark, bright]).astype(f32)


def test_oracle_correct_color_equals_reference(live):
    colors = tonemap_domain()
    want = live.correct_color(colors)
    got = np.array([oracle.correct_color(c) for c in colors], f32)
    same = ti._same(got, want).all(axis=1)
    assert same.all(), (np.nonzero(~same)[0][:8], colors[~same][:3], got[~same][:3], want[~same][:3])
    # both branches of the gamma curve, and the clamp at 1
    assert (want == 1.0).any() and ((want > 0) & (want < 12.92 * 0.0031308)).any() and (want > 0.5).any()


@pytest.mark.parametrize("name", list(rc.RENDER_CASES))
def test_oracle_frames_equal_reference(live, workdir, name):
    """path_tracing() over the case's calls: frame_buffer, squared_luminance, sample_count, random_numbers"""
    case, out = live_record(workdir, name)
    ocase, frames, counters = oracle_case(workdir, name)
    assert ocase.camera.tobytes() == case.camera.tobytes() and np.array_equal(ocase.seeds, case.seeds)
    # the reference's trace_ray has a stack of KD_TREE_DEPTH entries; a deeper push is undefined in it
    assert counters["deep_push"] == 0, counters
    want = [tuple(out[f"call{c}_{k}"] for k in rc.G_NAMES) for c in range(len(case.passes))]
    assert_same_frames(frames, want, f"{name}: oracle vs reference,")
    if name == rc.TONEMAP_CASE:
        np.testing.assert_array_equal(oracle.tonemap(frames[-1][0], frames[-1][2]), out["tonemap_rgba"])
    if name in rc.NONFINITE_CASES:
        np.testing.assert_array_equal(oracle.tonemap(frames[-1][0], rc.zeroed_counts(frames[-1][2])),
                                      out["tonemap_rgba"])


# ------------------------------------------ b. the product's host side vs live
@pytest.mark.parametrize("name", list(rc.RENDER_CASES))
def test_product_host_scene_equals_reference(live, workdir, name):
    """rt.HostScene's triangles (materials, texels) and rt.build_kd_tree's nodes, indices and bounds, byte for
    byte.  (The product makes its light list when it uploads a scene: tests/test_gpu_reference.py compares
    that with the recorded list.)"""
    case, _ = live_record(workdir, name)
    prod = rc.ProductScene(case.path)
    assert prod.camera.tobytes() == case.scene.camera.tobytes()
    assert_same_scene(rc.scene_bytes(prod), rc.scene_bytes(case.scene), name, lights=False)


# ------------------------------------------------------ c. fixtures are fresh
@pytest.mark.parametrize("name", rc.ALL_CASES)
def test_fixture_is_fresh(live, workdir, name):
    _, out = live_record(workdir, name)
    fx = rc.load_fixture(name)
    meta = json.loads(str(out["meta"]))
    assert fx["meta"]["files"] == meta["files"], "the scene's input files drifted: regenerate the fixtures"
    assert fx["meta"] == meta
    assert sorted(fx) == sorted(out)
    for key in out:
        if key != "meta":
            assert rc.same_bits(fx[key], out[key]), (name, key)


# ------------------------------------------- d. fixtures equal the oracle
@pytest.mark.parametrize("name", rc.ALL_CASES)
def test_fixture_equals_oracle(workdir, name):
    """needs no reference: the case's inputs rebuilt here hash to the recorded ones, and the oracle gives the
    recorded scene, frames, Samples and display bytes"""
    fx = rc.load_fixture(name)
    case, frames, counters = oracle_case(workdir, name)
    meta = case.meta()
    assert fx["meta"]["files"] == meta["files"], "the scene's input files drifted: regenerate the fixtures"
    assert {k: v for k, v in fx["meta"].items() if k != "scene"} == meta
    record, lights, bounds = rc.scene_record(case.scene)
    assert record == fx["meta"]["scene"]
    assert np.array_equal(lights, fx["lights"]) and bounds.tobytes() == fx["bounds"].tobytes()
    assert case.camera.tobytes() == fx["camera"].tobytes()
    if name == rc.RAY_CASE:
        assert rc.same_bits(case.rays(), fx["rays"])
        got = case.scene.trace_rays(fx["rays"])[:, :11]
        assert rc.same_bits(got, np.ascontiguousarray(fx["samples"][:, rc.SAMPLE_ORACLE_COLUMNS]))
        return
    assert np.array_equal(case.seeds, fx["seeds"])
    assert_same_frames(frames, rc.fixture_frames(fx), f"{name}: oracle vs fixture,")
    if name == rc.TONEMAP_CASE:
        np.testing.assert_array_equal(oracle.tonemap(frames[-1][0], frames[-1][2]), fx["tonemap_rgba"])
    if name in rc.NONFINITE_CASES:
        np.testing.assert_array_equal(oracle.tonemap(frames[-1][0], rc.zeroed_counts(frames[-1][2])),
                                      fx["tonemap_rgba"])
    if name == "materials":  # deep enough for wf_long at the depth tests/test_gpu_materials.py hands paths over
        assert counters["maxdepth"] >= rc.MATERIALS_MIN_DEPTH, counters
    if name == "trap":  # wf_long and the deep bounded traversal are really on the path
        assert counters["maxdepth"] >= rc.TRAP_MIN_DEPTH, counters
    if name == "h4":
        assert fx["meta"]["planted"] >= 30 and counters["xi_one"] >= fx["meta"]["planted"], counters
    hazard = {"aligned": "exit_tie", "aligned_h5": "on_split", "aligned_axis": "axis_parallel",
              "degenerate": "degenerate"}.get(name)
    if hazard:
        assert counters[hazard] > 100, counters


# ------------------------- e. the material cases meet their subject (oracle and fixtures only)
def _pixel_classes(fx):
    """of the recorded final frame: (pixels with a NaN, with an Inf and no NaN, finite and not black), a pixel
    being its three frame_buffer floats and its squared_luminance"""
    fb, sq, _, _ = rc.fixture_frames(fx)[-1]
    v = np.concatenate([fb, sq[:, None]], axis=1)
    nan = np.isnan(v).any(axis=1)
    inf = np.isinf(v).any(axis=1) & ~nan
    return nan, inf, np.isfinite(v).all(axis=1) & (fb != 0).any(axis=1)


def test_materials_case_covers_the_material_space(workdir):
    """every material of the materials case is what at least 8 pixels' centre rays meet first; every transparent
    one transmits there (the oracle's scatter on those hits, on the frame's seeds); the frames are finite, and hold f32 denormals (squared luminances of the albedo
    1e-21 box), which a device that flushed them would not reproduce; no path met the watchdog"""
    import hazards
    import independent as ind

    fx = rc.load_fixture("materials")
    case, _, counters = oracle_case(workdir, "materials")
    assert counters["maxdepth"] >= rc.MATERIALS_MIN_DEPTH and counters["maxdepth"] < 10_000, counters
    assert counters["watchdog"] == 0 and counters["cut"] == 0, counters
    mats = hazards.material_set()
    for want in ("rough_0_", "rough_1e-20_", "rough_1.5_", "n_1.0_", "n_0.5_", "n_100_", "k_1e-20", "k_50",
                 "albedo_0_", "albedo_2", "albedo_1e-30", "emissive_glass", "emissive_metal", "textured"):
        assert any(k.startswith(want) for k in mats), want
    rays, hits, names = rc.first_hits(case)
    names = np.array([n or "" for n in names])
    tris = np.frombuffer(case.scene.arrays()[0], np.uint8).reshape(-1, 152)
    frames = rc.fixture_frames(fx)
    for name, text in mats.items():
        px = np.nonzero(names == name)[0]
        assert len(px) >= 8, (name, len(px))
        if "transparent" not in text.split():
            continue
        t = tris[hits[px, 1].astype(np.int64)]
        mat = t[:, 96:132].copy().view(f32).reshape(-1, 9)
        nrm, tan = hits[px, 5:8], hits[px, 8:11]  # (the bitangent's sign does not matter to the event's type)
        smp = ti.scatter_samples(mat[:, 0:3], mat[:, 6], mat[:, 7], mat[:, 8], t[:, 132] != 0, hits[px, 2:5], nrm, tan,
                                 ind.normalize(ind.cross(nrm, tan)))
        types = ti.oracle_scatter(rays[px, 3:6], smp, np.zeros(len(px), bool), fx["seeds"][px])[2]
        assert (types == ind.TRANSMISSION).any(), (name, np.bincount(types))
    for c, arrays in enumerate(frames):
        for key, a in zip(rc.G_NAMES, arrays):
            assert a.dtype != f32 or np.isfinite(a).all(), (c, key)
    sq = frames[-1][1]
    denormal = (sq != 0) & (np.abs(sq) < np.finfo(f32).tiny)
    assert (denormal & (names == "albedo_1e-21")).sum() >= 8, (denormal.sum(), set(names[denormal]))


def test_nonfinite_case_is_nonfinite(workdir):
    """the recorded final frame of materials_nonfinite has NaN pixels, Inf pixels, and a good share of ordinary
    ones; the adaptive test stopped pixels at different counts; every path ended by itself"""
    import hazards

    for name in rc.NONFINITE_CASES:
        fx = rc.load_fixture(name)
        case, _, counters = oracle_case(workdir, name)
        assert counters["maxdepth"] < 1000 and counters["watchdog"] == 0 and counters["cut"] == 0, counters
        nan, inf, plain = _pixel_classes(fx)
        assert nan.sum() >= 50 and inf.sum() >= 50 and plain.sum() * 4 >= len(plain), (nan.sum(), inf.sum(), plain.sum())
        assert len(np.unique(rc.fixture_frames(fx)[-1][2])) >= 3
        names = [n for n in rc.first_hits(case)[2] if n]
        for mat in hazards.nonfinite_material_set():
            assert names.count(mat) >= 8, (mat, names.count(mat))
        rgba, zeroed = fx["tonemap_rgba"], rc.zeroed_counts(rc.fixture_frames(fx)[-1][2]) == 0
        assert zeroed.sum() > 200 and len(np.unique(rgba[:, :3])) > 50


def test_fixture_sizes():
    sizes = {n: os.path.getsize(rc.fixture_path(n)) for n in rc.ALL_CASES}
    assert max(sizes.values()) <= 256 * 1024 and sum(sizes.values()) <= 2 * 1024 * 1024, sizes
    assert sorted(os.listdir(rc.GOLDEN_DIR)) == sorted(n + ".npz" for n in rc.ALL_CASES)
