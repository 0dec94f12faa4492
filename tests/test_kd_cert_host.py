"""CPU checks of the T* certificate (csrc/bvh_common.h rt_kd_cert; DESIGN.md §5
"The certificate"), by tests/native/kd_cert_check.cpp over the library's own
prepared arrays:

* every safe box has the final-pass property (an independent sweep), every
  split value is in its axis' hash set;
* the bounded traversal as the kernels run it — s_min query, certificate,
  else the bounded KD descent — returns the plain KD traversal's triangle and
  barycentrics bit for bit on every ray, and a certified ray's descent agrees
  with its certificate;
* the shipped slack is >= 4x the derived bound for every ray that relies on it;
* no ray whose origin coordinate is a split value on an axis it goes up is
  certified.

Ray sets per scene: camera rays, bounces (some grazing, some axis-parallel),
chords of transparent objects, origins set to exact split values going up and
down, and rays aimed at a triangle's extreme vertex.  Two more sets have
tests of their own:

* the oracle's own path-traced rays (camera, extension and shadow rays of
  sampled pixels, dumped through or_log_rays as tools/dump_rays.py does):
  real bounce origins are computed hit points off their triangle, and the
  directions are the shading's — the mix the certificate ships on;
* rays built from the safe-box table whose hit point lands within a few ulp
  of the certificate's box threshold lo + delta / hi - delta, on both sides
  of it: some must certify, some must fall back as "box", none may mismatch.
  (The Cornell box has no such ray: its 36 wall triangles' margins exceed
  delta, so no threshold plane cuts a triangle.)

The certified share is printed per scene.  So that the comparison cannot pass
vacuously, Cornell and room_small have a floor at half the share this checker
measured on the CPU (1,000,000 rays, seed 7; a sixteenth of the rays are the
forced split-origin rays that must fall back):

    scene        measured   floor
    cornell      0.7076     0.35    (a quarter of its hits start on a wall that IS a split plane)
    room_small   0.9339     0.46

The adversarial, duplicate and other hazard scenes get no floor: there the
fallback is the point.  The GPU kernels are checked in tests/test_gpu_kd_cert.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hazards
import helpers
import oracle

FLOORS = {"cornell": 0.35, "room_small": 0.46}


@pytest.fixture(scope="module")
def cert_check(tmp_path_factory):
    return helpers.build_native(tmp_path_factory.mktemp("kdc"), "kd_cert_check")


def _field(out, name):
    return out.split(name + " ")[1].split()[0]


def _exec(args):
    """runs the checker; the assertions every ray set shares"""
    r = subprocess.run(args, capture_output=True, text=True, timeout=900, env=dict(os.environ, OMP_NUM_THREADS="8"))
    out = r.stdout
    print(out)
    assert r.returncode == 0, out + r.stderr
    assert " tables 0\n" in out, out  # the final-pass property of every safe box, the hash sets
    assert "mismatches 0 certified-vs-descent mismatches 0 slack violations 0 split-origin certified 0\n" in out, out
    assert float(_field(out, "smallest delta / derived bound")) >= 4.0, out
    return out


def _run(exe, scene, rays=1_000_000, seed=7, cam=None):
    args = [exe, scene, str(rays), str(seed)]
    if cam is not None:
        args.append(" ".join(float(v).hex() for v in cam))
    out = _exec(args)
    assert int(_field(out, "rays")) == rays and int(_field(out, "hits")) > rays // 8, out
    assert int(_field(out, "split-origin rays going up")) > 0, out
    return out


@pytest.mark.parametrize("name", ["cornell", "cornell_blob", "room_small"])
def test_certificate_equals_kd_traversal(cert_check, name):
    out = _run(cert_check, helpers.scene_path(name))
    if name in FLOORS:
        assert float(_field(out, "share")) >= FLOORS[name], out
    assert int(_field(out, "\ncertified")) > 0, out


def test_certificate_room2m(cert_check):
    out = _run(cert_check, helpers.scene_path("room2m"), rays=400_000, seed=11)
    assert int(_field(out, "\ncertified")) > 0, out


def test_certificate_hazard_scenes(cert_check, tmp_path):
    # walls on split planes: hits on leaf exits, origins on splits
    _run(cert_check, hazards.cornell_variant(str(tmp_path / "a"), "aligned", yaw_room=0.0))
    # camera rays from exactly the root split plane
    path = helpers.scene_path("cornell")
    on, _ = hazards.h5_cameras(oracle.OracleScene(path))
    _run(cert_check, path, cam=on[:3])
    # zero-area triangles (dropped from the BVH; listed in KD leaves)
    _run(cert_check, hazards.cornell_variant(str(tmp_path / "d"), "degenerate", yaw_room=0.1,
                                             extra_obj=hazards.DEGENERATE_OBJ))
    # two identical copies of a quad: every hit on them is a tie, which never certifies
    out = _run(cert_check, hazards.cornell_variant(str(tmp_path / "u"), "duplicate", yaw_room=0.1,
                                                   extra_obj=hazards.DUPLICATE_OBJ))
    assert int(_field(out, "fallbacks: tie")) > 1000, out
    # the glass light guide
    _run(cert_check, helpers.make_trap_scene(str(tmp_path / "t")))


@pytest.mark.parametrize("variant", ["far", "tiny", "near"])
def test_certificate_adversarial_scenes(cert_check, tmp_path, variant):
    """slivers with unbounded boxes (no safe box), needles and a cloud of tiny triangles"""
    _run(cert_check, hazards.adversarial_scene(str(tmp_path / variant), variant), seed=3)


def _dump_oracle_rays(scene, path, W, H, npix):
    """the oracle's rays of `npix` path-traced pixels of a W x H frame, in the order it traces them
    (camera, extension and shadow rays; or_log_rays, as tools/dump_rays.py): float32 (n, 6) {o, d}"""
    L = oracle.lib()
    L.or_log_rays.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p, ctypes.c_int,
                                                                            ctypes.c_void_p, ctypes.c_int]
    L.or_log_rays.restype = ctypes.c_int
    sc = oracle.OracleScene(scene)
    pix = np.random.default_rng(0).choice(W * H, npix, replace=False).astype(np.int32)
    cap = npix * 80
    rays = np.zeros((cap, 6), np.float32)
    n = L.or_log_rays(sc.h, sc.camera.ctypes.data, W, H, pix.ctypes.data, len(pix), rays.ctypes.data, cap)
    assert 0 < n <= cap, n
    rays[:n].tofile(path)
    return int(n)


@pytest.mark.parametrize("name,npix", [("cornell", 8192), ("room_small", 8192), ("room2m", 2048)])
def test_certificate_on_the_oracles_path_traced_rays(cert_check, tmp_path, name, npix):
    scene = helpers.scene_path(name)
    f = str(tmp_path / "rays.f32")
    n = _dump_oracle_rays(scene, f, 1920, 1080, npix)
    out = _exec([cert_check, scene, "file", f])
    assert int(_field(out, "rays")) == n and n > 2 * npix, out  # (more than camera rays: bounces and shadow rays)
    assert int(_field(out, "\ncertified")) > 0 and int(_field(out, "hits")) > npix, out


@pytest.mark.parametrize("name,rays", [("cornell_blob", 300_000), ("room_small", 300_000), ("room2m", 100_000)])
def test_certificate_at_the_safe_box_threshold(cert_check, name, rays):
    out = _exec([cert_check, helpers.scene_path(name), "faces", str(rays), "7"])
    near = int(_field(out, "face rays within 8 ulp of a box threshold"))
    cert, box = int(_field(out, "box threshold %d certified" % near)), int(_field(out, "box-fallback"))
    assert near > rays // 20 and cert > near // 100 and box > near // 100, out
