"""CPU checks of wf_long's wave-wide s_min query (csrc/wide_bvh.h) and of the
wide collapse of the conservative BVH it runs on (csrc/host/bvh_build.*
collapse_bvh_wide), by tests/native/wide_smin_check.cpp over the library's
own prepared arrays:

* the wide collapse is structurally the binary tree (every leaf reference
  once, every child box a bit copy of a binary node's box), at the shipped
  arity and at 4, 8, 32 and 64;
* a host restatement of the level-synchronous query (frozen-best rounds,
  leaves tested a round after they are listed, the tie merge across rounds)
  returns the sequential query's (best, tk) bit for bit, whichever way its
  lists are walked, on camera rays, bounce rays, chords of the transparent
  objects and grazing rays;
* the wide query + the bounded KD traversal, and the capacity fallback forced
  with lists of one item, return the plain KD traversal's hit.

The GPU kernel is compared with the oracle in tests/test_gpu_deep_bounded.py.
"""
import os
import subprocess

import pytest

import hazards
import helpers
import oracle


@pytest.fixture(scope="module")
def smin_check(tmp_path_factory):
    return helpers.build_native(tmp_path_factory.mktemp("wsm"), "wide_smin_check")


def _run(exe, scene, rays=200_000, seed=7, cam=None, edges=False):
    args = [exe, scene] + (["edges"] if edges else [str(rays), str(seed)])
    if cam is not None:
        args.append(" ".join(float(v).hex() for v in cam))
    r = subprocess.run(args, capture_output=True, text=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="4"))
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert " structure 0\n" in out, out
    assert "query mismatches 0 order mismatches 0 hit mismatches 0 fallback mismatches 0\n" in out, out
    return out


def _field(out, name):
    return int(out.split(name + " ")[1].split()[0])


@pytest.mark.parametrize("name,rays", [("cornell_blob", 300_000), ("room_small", 300_000)])
def test_wide_query_equals_sequential_query(smin_check, name, rays):
    out = _run(smin_check, helpers.scene_path(name), rays)
    assert _field(out, "rays") == rays and _field(out, "bounded") > rays // 2 and _field(out, "hits") > rays // 4, out
    # the forced fallback (lists of one item) was taken, and the shipped capacities never overflowed
    assert _field(out, "forced fallbacks") > rays // 4 and _field(out, "overflows") == 0, out


def test_wide_query_hazard_scenes_and_light_guide(smin_check, tmp_path):
    aligned = hazards.cornell_variant(str(tmp_path / "a"), "aligned", yaw_room=0.0)
    _run(smin_check, aligned, 100_000)
    degen = hazards.cornell_variant(str(tmp_path / "d"), "degenerate", yaw_room=0.1, extra_obj=hazards.DEGENERATE_OBJ)
    _run(smin_check, degen, 100_000)
    # two identical copies of a quad: two slots pass at exactly the same s
    dup = hazards.cornell_variant(str(tmp_path / "u"), "duplicate", yaw_room=0.1, extra_obj=hazards.DUPLICATE_OBJ)
    assert _field(_run(smin_check, dup, 100_000), "ties") > 1000
    trap = helpers.make_trap_scene(str(tmp_path / "t"))
    _run(smin_check, trap, 100_000)
    # camera rays from exactly the root split plane
    path = helpers.scene_path("cornell")
    on, _ = hazards.h5_cameras(oracle.OracleScene(path))
    _run(smin_check, path, 100_000, cam=on[:3])
    # always-tested slivers (unbounded boxes), needles and a cloud of tiny triangles
    _run(smin_check, hazards.adversarial_scene(str(tmp_path / "n"), "near"), 100_000, seed=3)


def _tie_grid(d):
    """A flat mesh (z = 0) of exactly representable coordinates: 16 x 16 unit
    quads beside a 16 x 64 strip of quarter-unit quads (a T-junction seam at
    x = 16), so the BVH is deeper over the strip than over the coarse part.
    A ray straight down onto the midpoint of an edge meets the triangles on
    both sides at exactly the same s, both passing with a barycentric
    coordinate of exactly 0: a tie — across the diagonals inside one leaf,
    across quads in different leaves, and across the seam in leaves of
    different depth, where the second pass arrives in a later round."""
    os.makedirs(d, exist_ok=True)
    vs, faces = [], []

    def quad(x0, y0, s):
        b = len(vs) + 1
        vs.extend([(x0, y0), (x0 + s, y0), (x0 + s, y0 + s), (x0, y0 + s)])
        faces.append(f"f {b} {b + 1} {b + 2} {b + 3}")

    for i in range(16):
        for j in range(16):
            quad(float(i), float(j), 1.0)
    for i in range(16):
        for j in range(64):
            quad(16.0 + 0.25 * i, 0.25 * j, 0.25)
    with open(os.path.join(d, "grid.obj"), "w") as f:
        f.write("\n".join([f"v {x!r} {y!r} 0.0" for x, y in vs] + ["usemtl lamp", faces[0], "usemtl white"] + faces[1:])
                + "\n")
    with open(os.path.join(d, "grid.mat"), "w") as f:
        f.write("material white\nalbedo 0.7 0.7 0.7\nroughness 0.5\nn 1.5\n\n"
                "material lamp\nalbedo 0.8 0.8 0.8\nemittance 6.0 5.5 5.0\nroughness 0.5\nn 1.5\n")
    p = os.path.join(d, "scene.txt")
    with open(p, "w") as f:
        f.write("mesh grid.obj grid.mat 0 0 0 0 0 1 0\ncamera 0 0 5 0 0 0.8 0\n")
    return p


def test_wide_query_constructed_ties(smin_check, tmp_path):
    """Two triangles sharing an edge, hit exactly on it: the wide query reports
    the tie as the sequential query does — also when the two lie in different
    leaves and the second pass arrives in a later round than the first."""
    out = _run(smin_check, _tie_grid(str(tmp_path / "g")), edges=True)
    assert _field(out, "ties") > 1000, out
    assert _field(out, "cross-round ties") > 0, out
