"""bench.py's measurement code on CPU: the counter-window parser and the
counter-measured roofline arithmetic (FETCH_SIZE x2 + WRITE_SIZE per sample x
samples/s), on synthetic rocprofv3 CSVs."""
import csv
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

FIELDS = ["Dispatch_Id", "Kernel_Name", "Counter_Name", "Counter_Value"]


def _csv(path, rows, fields=FIELDS):
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=fields)
        w.writeheader()
        for r in rows:
            w.writerow(dict(zip(fields, r)))


def _pass(tmp_path, tag, counter, per_kernel):
    """Dispatches: warm-up trace (outside), marker, trace, shade, long, marker, trace (outside)."""
    rows = [(1, "void wf_trace_coop<false>(...)", counter, 999.0), (2, "rt_tonemap_kernel(...)", counter, 0.0)]
    i = 3
    for k, v in per_kernel.items():
        rows.append((i, f"void {k}(RtDevScene, ...)", counter, v))
        i += 1
    rows += [(i, "rt_tonemap_kernel(...)", counter, 0.0), (i + 1, "void wf_trace_coop<false>(...)", counter, 777.0)]
    cc = tmp_path / f"{tag}_counter_collection.csv"
    _csv(cc, rows)
    trace = tmp_path / f"{tag}_kernel_trace.csv"
    _csv(trace, [(r[0], r[1], 1000 * r[0], 1000 * r[0] + 500) for r in rows],
         ["Dispatch_Id", "Kernel_Name", "Start_Timestamp", "End_Timestamp"])
    return str(cc), str(trace)


def test_window_sums_take_only_the_marked_call(tmp_path):
    cc, tr = _pass(tmp_path, "f", "FETCH_SIZE", {"wf_trace_coop<false>": 100.0, "wf_shade<false>": 10.0})
    total, per_kernel, n, kt = bench._window_sums(cc, tr)
    assert total == {"FETCH_SIZE": 110.0}
    assert n == 2
    assert per_kernel["wf_trace_coop<false>"]["FETCH_SIZE"] == 100.0
    assert kt["wf_shade<false>"]["dispatches"] == 1


def test_roofline_from_counters(tmp_path):
    fetch = {"wf_trace_coop<false>": 1000.0, "wf_shade<false>": 50.0, "wf_long<false>": 1.0}
    write = {"wf_trace_coop<false>": 10.0, "wf_shade<false>": 40.0, "wf_long<false>": 0.0}
    sq = {"wf_trace_coop<false>": 0.0}
    passes = {}
    for tag, ctr, vals in (("fetch", "FETCH_SIZE", fetch), ("write", "WRITE_SIZE", write)):
        cc, tr = _pass(tmp_path, tag, ctr, vals)
        total, per_kernel, n, kt = bench._window_sums(cc, tr)
        passes[tag] = {"counters": total, "per_kernel": per_kernel, "dispatches": n, "kernel_trace": kt,
                       "wall_s": 1.0, "samples": 1000}
    sq_rows = []
    for k, (wc, wait, inst, valu, thr) in {"wf_trace_coop<false>": (1000.0, 600.0, 300.0, 100.0, 4800.0),
                                            "wf_long<false>": (9000.0, 8900.0, 10.0, 5.0, 64.0)}.items():
        sq_rows.append((k, {"SQ_WAVE_CYCLES": wc, "SQ_WAIT_ANY": wait, "SQ_ACTIVE_INST_ANY": inst,
                            "SQ_ACTIVE_INST_VALU": valu, "SQ_THREAD_CYCLES_VALU": thr}))
    sq_total = {c: sum(v[c] for _, v in sq_rows) for c in sq_rows[0][1]}
    passes["sq"] = {"counters": sq_total, "per_kernel": dict(sq_rows), "dispatches": 2, "kernel_trace": {},
                    "wall_s": 1.0, "samples": 1000}
    achieved, d = bench.roofline_from_pmc({"passes": passes}, samples_per_s=1e6)
    fetch_b = 2 * 1024 * sum(fetch.values())
    write_b = 1024 * sum(write.values())
    assert d["hbm_bytes_per_sample"] == pytest.approx((fetch_b + write_b) / 1000, rel=1e-3)
    assert d["hbm_bytes_per_sample_raw"] == pytest.approx((fetch_b / 2 + write_b) / 1000, rel=1e-3)
    assert achieved == pytest.approx((fetch_b + write_b) / 1000 * 1e6 / 1e9)
    # the dominant kernel moves the most bytes (wf_long's slices only poll)
    assert d["dominant_kernel"] == "wf_trace_coop<false>"
    assert d["latency"]["scope"] == "wf_trace_coop<false>"
    assert d["latency"]["wait_frac"] == pytest.approx(0.6)
    assert d["latency"]["valu_lane_util"] == pytest.approx(4800.0 / (64 * 100.0), abs=1e-3)


def test_plain_run_times_its_steps_and_dumps_what_they_left(tmp_path, capsys):
    """A plain run (no --full) over the CPU stand-in binding: the warm-up and
    the timed steps are its only renders, the line says what was not
    measured, and --dump-outputs holds the G-buffer those steps left."""
    import json

    import numpy as np

    import bench_stub_rt
    import helpers

    helpers.scene_path("cornell")
    W, H, P = 12, 8, 2
    out = tmp_path / "dump"
    del bench_stub_rt.calls[:]
    rc = bench.main(["--gpus", "1", "--steps", "3", "--warmup", "1", "--passes", str(P), "--steps-per-call", "2",
                     "--scene", "cornell", "--width", str(W), "--height", str(H), "--scene-dir", helpers.SCENE_DIR,
                     "--dump-outputs", str(out)], binding=bench_stub_rt)
    assert rc == 0
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    # (sample_count argument, passes) of every render: 1 warm-up step, then 3 timed steps in calls of 2 + 1
    assert [c[1:] for c in bench_stub_rt.calls] == [(0, P), (1, 2 * P), (1, P)]
    assert line["steps"] == 3 and line["full"] is False
    assert line["roofline"] is None and line["per_sample"] is None and line["cpu_baseline"] is None
    # (both figures are rounded to 3 decimals on the line)
    assert line["value"] == pytest.approx(W * H * P * 3 / (line["ms_per_step"] * 3 / 1e3) / 1e6, rel=2e-2, abs=2e-3)
    ref, _ = helpers.oracle_render(helpers.scene_path("cornell"), W, H, [P, 2 * P, P])
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["frame_buffer", "nonfinite", "rgba", "sample_count", "squared_luminance"]
    assert not got["nonfinite"].any()  # (Cornell at these sizes: every sum finite, nothing replaced)
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["frame_buffer"], ref[0]) and np.array_equal(got["squared_luminance"], ref[1])
    assert np.array_equal(got["sample_count"], np.full(W * H, 4 * P, np.float32))
    assert got["rgba"].shape == (W * H, 4)


def test_scene_goes_to_the_user_cache_when_the_scene_dir_cannot_be_written(tmp_path, monkeypatch):
    """A run from a tree its user cannot write to: the scene is generated once
    into the user's cache and found there by the next run."""
    import rt

    blocked = tmp_path / "file"
    blocked.write_text("")  # a directory below a regular file cannot be made, whoever asks
    monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path / "cache"))
    args = bench.parse_args(["--scene", "cornell", "--scene-dir", str(blocked / "scenes")])
    first = bench.ensure_scene(args, rt)
    assert first == str(tmp_path / "cache" / "isaklm-raytracer_amd" / "scenes" / "cornell" / "scene.txt")
    assert os.path.exists(first) and rt.HostScene(first).triangle_ptr()[1] > 0
    stamp = os.path.getmtime(first)
    assert bench.ensure_scene(args, rt) == first and os.path.getmtime(first) == stamp
    assert os.listdir(tmp_path / "cache" / "isaklm-raytracer_amd" / "scenes") == ["cornell"]


def test_dump_outputs_are_finite_and_say_where_the_render_was_not(tmp_path):
    import numpy as np

    fb = np.arange(12, dtype=np.float32).reshape(4, 3)
    fb[1] = [np.inf, 5.0, np.nan]
    fb[3, 1] = -np.inf
    sq = np.array([1.0, np.nan, 2.0, 3.0], np.float32)
    kept = fb.copy()
    bench.dump_outputs(str(tmp_path), {"frame_buffer": fb, "squared_luminance": sq,
                                       "sample_count": np.full(4, 7, np.int32)})
    assert np.array_equal(fb, kept, equal_nan=True)  # the caller's arrays are left alone
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(np.isfinite(a).all() and a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["frame_buffer"], [[0, 1, 2], [0, 5, 0], [6, 7, 8], [9, 0, 11]])
    assert np.array_equal(got["squared_luminance"], [1, 0, 2, 3])
    # base-4 digits, lowest first: fb.x, fb.y, fb.z, sq; 1 +inf, 2 -inf, 3 NaN
    assert np.array_equal(got["nonfinite"], [0, 1 + 3 * 16 + 3 * 64, 0, 2 * 4])


def test_dump_outputs_samples_the_same_pixels_of_a_large_frame(tmp_path):
    import numpy as np

    n = 5000
    arrays = {"frame_buffer": np.arange(3 * n, dtype=np.float32).reshape(n, 3),
              "sample_count": np.arange(n, dtype=np.int32) + (1 << 24)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, limit=40000)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 40000
    pix = got["pixels"].astype(np.int64)
    assert 1000 < len(pix) < n and np.all(np.diff(pix) > 0)
    assert np.array_equal(got["frame_buffer"], arrays["frame_buffer"][pix])
    assert got["sample_count"].dtype == np.float64  # counts of 2^24 and more are not exact in float32
    assert np.array_equal(got["sample_count"], arrays["sample_count"][pix])
    assert np.array_equal(pix, np.load(tmp_path / "b" / "pixels.npy"))  # the same sample in every run


def test_metric_names_the_rendered_frame():
    assert "1920×1080" in bench.METRIC


def test_call_plan_groups_steps_into_calls():
    # the driver's --steps 20 --warmup 5 with the default 4 steps per call
    assert bench.call_plan(0, 5, 4) == [(0, 4), (4, 1)]
    assert bench.call_plan(5, 20, 4) == [(5, 4), (9, 4), (13, 4), (17, 4), (21, 4)]
    # every step rendered exactly once, only the first call starts at step 0
    for first, count, per in ((0, 1, 4), (1, 4, 4), (0, 7, 3), (3, 0, 4), (2, 9, 1)):
        plan = bench.call_plan(first, count, per)
        covered = [s for start, k in plan for s in range(start, start + k)]
        assert covered == list(range(first, first + count))
        assert all(1 <= k <= per for _, k in plan)
    args = bench.parse_args([])
    assert args.passes * args.steps_per_call == 256
