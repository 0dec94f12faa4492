// reproject.hip — rt_reproject's and rt_reproject_sampler's kernel.
//
// The reprojection is defined in reproject_math.h (the text
// host/reproject_host.cpp compiles too); this file only maps it onto the GPU:
// one thread per output pixel, denoise.hip's 1-D grid of 32 x 8 tiles (row by
// row), no LDS, nothing shared between blocks.  A wave is two 32-pixel row
// segments: under coherent camera motion its lanes gather neighbouring source
// pixels, so the four bilinear taps of a wave fall on a handful of cache
// lines per array.  A tap's depth and count are tested before its normal,
// triangle and colour are loaded, and a wave whose pixels all reset (sky, a
// region that was off the old frame) stores its zeros and leaves without a
// colour load.  The kernel is bound by memory latency: ~76 B of unique traffic
// per pixel (DESIGN.md "Temporal reprojection" has the measured time beside a
// copy of the same arrays).  The camera model is a template parameter: the
// pinhole instantiation is rt_reproject's, the others (rt_reproject_sampler)
// differ in the projection alone and add two or three double-precision
// atan evaluations per pixel (rt_libm.h rt_atan2f).
//
// stats: each wave reduces its three sums over its lanes and issues one
// device atomic per non-zero word.
#include <hip/hip_runtime.h>

#include "reproject_math.h"
#include "rt_launch.h"

#define RP_TILE_W 32
#define RP_TILE_H 8

namespace {

__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// MODEL: the two cameras' model (reproject_math.h); RT_SAMPLER_PINHOLE is rt_reproject's kernel and reads no lens
template <int MODEL>
__global__ void __launch_bounds__(256) rp_reproject_kernel(RtRpFrame src, RtDevCamera src_cam, const float *dst_depth,
                                                           const float *dst_normal, const int *dst_triangle,
                                                           RtDevCamera dst_cam, Vec3D delta, int width, int height,
                                                           int tiles_x, RtRpParams prm, Vec3D *fb_out, float *sq_out,
                                                           int *count_out, unsigned long long *stats, RtRpLens lens)
{
    const int x = (int)(blockIdx.x % (unsigned)tiles_x) * RP_TILE_W + threadIdx.x;
    const int y = (int)(blockIdx.x / (unsigned)tiles_x) * RP_TILE_H + threadIdx.y;
    const bool inside = x < width && y < height;
    int kept = 0;
    if (inside) {
        const RtRpPixel o = rt_rp_pixel<MODEL>(src, src_cam, dst_depth, dst_normal, dst_triangle, dst_cam, delta,
                                               width, height, x, y, prm, lens);
        const size_t p = (size_t)y * width + x;
        fb_out[p] = o.fb;
        sq_out[p] = o.sq;
        count_out[p] = o.count;
        kept = o.count;
    }
    if (stats) { // (uniform: every lane of the wave takes part in the shuffles, the ones outside the frame with 0)
        // a wave's sums fit 32 bits: 64 lanes x max_history <= 2^26
        const unsigned n_pix = wave_sum(inside ? 1u : 0u);
        const unsigned n_kept = wave_sum(kept > 0 ? 1u : 0u);
        const unsigned n_samples = wave_sum((unsigned)kept);
        const int lane = (int)((threadIdx.y * RP_TILE_W + threadIdx.x) & 63u);
        if (lane == 0) {
            if (n_pix) atomicAdd(stats + 0, (unsigned long long)n_pix);
            if (n_kept) atomicAdd(stats + 1, (unsigned long long)n_kept);
            if (n_samples) atomicAdd(stats + 2, (unsigned long long)n_samples);
        }
    }
}

} // namespace

// ---- launcher (called by abi.hip) ----
int rt_launch_reproject(const RtRpFrame &src, const RtDevCamera &src_cam, const float *dst_depth,
                        const float *dst_normal, const int *dst_triangle, const RtDevCamera &dst_cam, int width,
                        int height, const RtRpParams &prm, Vec3D *fb_out, float *sq_out, int *count_out,
                        unsigned long long *stats, hipStream_t stream, int model, const RtRpLens &lens)
{
    const dim3 block(RP_TILE_W, RP_TILE_H);
    // (a 1-D grid of tiles, row by row, as rt_launch_denoise: within the x limit for every width * height < 2^31)
    const int tiles_x = (width + RP_TILE_W - 1) / RP_TILE_W;
    const dim3 grid((unsigned)((long long)tiles_x * ((height + RP_TILE_H - 1) / RP_TILE_H)));
    void (*kernel)(RtRpFrame, RtDevCamera, const float *, const float *, const int *, RtDevCamera, Vec3D, int, int, int,
                   RtRpParams, Vec3D *, float *, int *, unsigned long long *, RtRpLens);
    switch (model) {
    case RT_SAMPLER_PINHOLE: kernel = rp_reproject_kernel<RT_SAMPLER_PINHOLE>; break;
    case RT_SAMPLER_EQUIRECT: kernel = rp_reproject_kernel<RT_SAMPLER_EQUIRECT>; break;
    case RT_SAMPLER_FISHEYE: kernel = rp_reproject_kernel<RT_SAMPLER_FISHEYE>; break;
    case RT_SAMPLER_ORTHO: kernel = rp_reproject_kernel<RT_SAMPLER_ORTHO>; break;
    default: return -1; // (abi.hip admits the four image kinds only)
    }
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, src, src_cam, dst_depth, dst_normal, dst_triangle, dst_cam,
                       rt_rp_delta(src_cam, dst_cam), width, height, tiles_x, prm, fb_out, sq_out, count_out, stats,
                       lens);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
