// convergence.hip — rt_convergence's kernel.
//
// The test is defined in convergence_math.h (the text
// host/convergence_host.cpp compiles too); this file only maps it onto the
// GPU: a streaming read of 20 B per element (three colour floats, the
// squared-luminance sum, the count) and an optional 4-B store of the diagnostic
// map, one thread per element up to CV_MAX_BLOCKS blocks and in grid strides
// past that.  No LDS, no workspace, nothing shared between blocks.
//
// stats: each lane counts its elements, its open ones, the ones below
// min_samples and their samples; at the end each wave sums the four over its
// lanes and issues one device atomic per non-zero word (query.hip flush_stats'
// scheme).  The grid's cap bounds those atomics on four addresses — 8,192 waves
// x 4 words — where one thread per element of a 1080p frame issued 130 thousand
// and spent most of its millisecond on them.
#include <hip/hip_runtime.h>

#include "convergence_math.h"
#include "rt_launch.h"

#define CV_BLOCK 256
#define CV_MAX_BLOCKS 2048 // the grid's cap: past it a thread walks the elements in grid strides

namespace {

__global__ void __launch_bounds__(CV_BLOCK) cv_convergence_kernel(const float *radiance, const float *sq,
                                                                    const int *count, uint32_t n, RtCvParams prm,
                                                                    float *rel_error, unsigned long long *stats)
{
    // (e < n <= 2^31 - 1 and the stride is at most 2^19: e + stride does not wrap)
    const uint32_t stride = gridDim.x * CV_BLOCK;
    uint32_t n_in = 0, n_open = 0, n_below = 0; // this lane's elements: at most n / stride + 1 each
    long long cnt = 0;
    for (uint32_t e = blockIdx.x * CV_BLOCK + threadIdx.x; e < n; e += stride) {
        const float *r = radiance + 3 * (size_t)e;
        const int c = count[e];
        const RtCvElement o = rt_cv_element(prm, rt_v3(r[0], r[1], r[2]), sq[e], c);
        if (rel_error) rel_error[e] = o.rel_error;
        ++n_in;
        n_open += o.open;
        n_below += o.below_min;
        cnt += c;
    }
    if (stats) { // (uniform, and the loop's exits have reconverged: every lane of the wave takes part)
        unsigned long long total[4] = {n_in, n_open, n_below, (unsigned long long)cnt}; // (negative counts add
                                                                                       // modulo 2^64, as on the host)
        for (int k = 0; k < 4; ++k)
            for (int off = 32; off > 0; off >>= 1) total[k] += __shfl_xor(total[k], off);
        if (__lane_id() == 0)
            for (int k = 0; k < 4; ++k)
                if (total[k]) atomicAdd(stats + k, total[k]);
    }
}

} // namespace

// ---- launcher (called by abi.hip) ----
int rt_launch_convergence(const float *radiance, const float *sq, const int *count, long long n, const RtCvParams &prm,
                          float *rel_error, unsigned long long *stats, hipStream_t stream)
{
    const long long need = (n + CV_BLOCK - 1) / CV_BLOCK;
    const dim3 grid((uint32_t)(need < CV_MAX_BLOCKS ? need : CV_MAX_BLOCKS)), block(CV_BLOCK);
    hipLaunchKernelGGL(cv_convergence_kernel, grid, block, 0, stream, radiance, sq, count, (uint32_t)n, prm, rel_error,
                       stats);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
