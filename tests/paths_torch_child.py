"""Child process of test_gpu_paths.test_torch_tensors_on_the_current_stream.

torch is imported first, so the library binds to the HIP runtime torch
loaded (as in tests/query_torch_child.py): rays, RNG states and the outputs
in torch device tensors, rt_trace_paths enqueued on torch's current stream
through rt.trace_paths_device — a 2-sample call, then an accumulating one —
results equal to the numpy path's.  Prints "OK" on success.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "isaklm-raytracer_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import helpers  # noqa: E402
import oracle  # noqa: E402
import rt  # noqa: E402


def main():
    torch.cuda.set_device(0)
    run = helpers.GpuRun("cornell")
    n = 4096
    g = np.random.default_rng(23)
    bounds = oracle.OracleScene(run.path).arrays()[4]
    lo, hi = bounds[:3], bounds[3:]
    d = g.normal(size=(n, 3))
    rays = np.concatenate([g.uniform(lo, hi, (n, 3)), d / np.linalg.norm(d, axis=1)[:, None]], 1).astype(np.float32)
    seeds = oracle.mt19937(n, 11)
    first = rt.trace_paths(run.dev, rays, seeds, samples=2)
    want = rt.trace_paths(run.dev, rays, first[2], samples=1, radiance=first[0], sq=first[1])
    assert (want[0] != 0).any(axis=1).mean() > 0.25 and (want[0] != first[0]).any()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # a stream of torch's own making is the current one
        # (copies only: a torch kernel launch would load torch's whole GPU code object, seconds of start-up;
        # the RNG words travel as int32, the same bytes)
        t_rays = torch.from_numpy(rays).cuda()
        t_rng = torch.from_numpy(seeds.view(np.int32).copy()).cuda()
        t_rad = torch.from_numpy(np.full((n, 3), -7.0, np.float32)).cuda()
        t_sq = torch.from_numpy(np.full(n, -7.0, np.float32)).cuda()
        stream = torch.cuda.current_stream().cuda_stream
        rt.trace_paths_device(run.dev, t_rays.data_ptr(), t_rng.data_ptr(), n, t_rad.data_ptr(), t_sq.data_ptr(),
                              samples=2, stream=stream)
        rt.trace_paths_device(run.dev, t_rays.data_ptr(), t_rng.data_ptr(), n, t_rad.data_ptr(), t_sq.data_ptr(),
                              samples=1, accumulate=True, stream=stream)
        got = (t_rad.cpu().numpy(), t_sq.cpu().numpy(), t_rng.cpu().numpy().view(np.uint32))  # (stream-ordered)
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    print("OK", flush=True)


if __name__ == "__main__":
    main()
