"""Child process of test_gpu_query.test_torch_tensors_on_the_current_stream.

torch is imported first, so the library binds to the HIP runtime torch
loaded (as in tests/queue_sharing_child.py): rays in a torch device tensor,
rt_trace_rays enqueued on torch's current stream through
rt.trace_rays_device, hits and surfaces equal to the numpy path's.  Prints
"OK" on success.
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
    g = np.random.default_rng(21)
    bounds = oracle.OracleScene(run.path).arrays()[4]
    lo, hi = bounds[:3], bounds[3:]
    d = g.normal(size=(n, 3))
    rays = np.concatenate([g.uniform(lo, hi, (n, 3)), d / np.linalg.norm(d, axis=1)[:, None]], 1).astype(np.float32)
    want, want_surf = rt.trace_rays(run.dev, rays, surface=True)
    assert 0.25 * n < (want["triangle"] >= 0).sum()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # a stream of torch's own making is the current one
        t_rays = torch.from_numpy(rays).cuda()
        # (copies only: a torch kernel launch would load torch's whole GPU code object, seconds of start-up)
        t_hits = torch.from_numpy(np.full((n, 4), -7, np.int32)).cuda()
        t_surf = torch.from_numpy(np.full((n, 20), -7.0, np.float32)).cuda()
        rt.trace_rays_device(run.dev, t_rays.data_ptr(), n, t_hits.data_ptr(), t_surf.data_ptr(),
                             stream=torch.cuda.current_stream().cuda_stream)
        hits = t_hits.cpu().numpy()  # (stream-ordered behind the query)
        surf = t_surf.cpu().numpy()
    assert np.array_equal(hits.view(np.uint32), want.view(np.uint32).reshape(n, 4))
    assert np.array_equal(surf.view(np.uint32), want_surf.view(np.uint32).reshape(n, 20))
    print("OK", flush=True)


if __name__ == "__main__":
    main()
