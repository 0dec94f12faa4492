// denoise.hip — rt_denoise's and rt_denoise_sampler's kernels and rt_tonemap_rgb.
//
// The filter is defined in denoise_math.h (the text host/denoise_host.cpp
// compiles too); this file only maps it onto the GPU:
//
//   dn_prepare   G_Buffer + AOVs -> state (irradiance.rgb, variance) and guides
//                (normal.xyz, depth) as one 16-B record each, + the depth slope
//   dn_filter    one a-trous level, state -> state (ping-pong), launched once
//                per level; the last launch multiplies the albedo back and
//                writes the caller's RGB buffer instead
//
// One thread per pixel, a plain grid of 32 x 8 tiles (row by row), no atomics,
// nothing shared between blocks.  A tap costs two 16-B loads; at spacings 1
// and 2 a tile's taps overlap and are served by the CU's vector cache, at
// larger spacings by L2 (a 1920 x 1080 frame's workspace is 108 MB: it stays
// in the Infinity Cache between levels).  The level kernel is bound by
// instruction issue (~100 instructions per tap: the edge stops' IEEE
// divisions), not by memory — the levels with and without overlap take the
// same time within 10 % — so it has no LDS tile.
#include <hip/hip_runtime.h>

#include "denoise_math.h"
#include "rt_launch.h"
#include "rt_workspace.h"

#define DN_TILE_W 32
#define DN_TILE_H 8

namespace {

// WRAP_X: the x axis is periodic (denoise_math.h; rt_denoise_sampler's EQUIRECT frames)
template <bool WRAP_X>
__global__ void __launch_bounds__(256) dn_prepare_kernel(const Vec3D *fb, const float *sq, const int *count,
                                                         const float *depth, const float *normal,
                                                         const float *albedo, int width, int height, int tiles_x,
                                                         int demodulate, RtDn4 *state, RtDn4 *guide, float *slope)
{
    const int x = (int)(blockIdx.x % (unsigned)tiles_x) * DN_TILE_W + threadIdx.x;
    const int y = (int)(blockIdx.x / (unsigned)tiles_x) * DN_TILE_H + threadIdx.y;
    if (x >= width || y >= height) return;
    const int p = y * width + x;
    RtDn4 s, g;
    float gz;
    rt_dn_prepare_pixel<WRAP_X>(fb, sq, count, depth, normal, albedo, width, height, x, y, demodulate, &s, &g, &gz);
    state[p] = s;
    guide[p] = g;
    slope[p] = gz;
}

// FINAL: the last level — remodulate and store 3 floats per pixel into rgb_out (state_out unused)
template <bool FINAL, bool WRAP_X>
__global__ void __launch_bounds__(256) dn_filter_kernel(const RtDn4 *__restrict__ state_in,
                                                        const RtDn4 *__restrict__ guide,
                                                        const float *__restrict__ slope, int width, int height,
                                                        int tiles_x, int step, RtDnParams prm, RtDn4 *__restrict__ state_out,
                                                        const float *__restrict__ albedo, float *__restrict__ rgb_out)
{
    const int x = (int)(blockIdx.x % (unsigned)tiles_x) * DN_TILE_W + threadIdx.x;
    const int y = (int)(blockIdx.x / (unsigned)tiles_x) * DN_TILE_H + threadIdx.y;
    if (x >= width || y >= height) return;
    const int p = y * width + x;
    const RtDn4 s = rt_dn_filter_pixel<WRAP_X>(state_in, guide, slope, width, height, x, y, step, prm);
    if (FINAL) {
        const Vec3D c = rt_dn_remodulate(s, rt_dn_demodulator(albedo, (size_t)p, prm.demodulate));
        float *o = rgb_out + 3 * (size_t)p;
        o[0] = c.x;
        o[1] = c.y;
        o[2] = c.z;
    } else {
        state_out[p] = s;
    }
}

// rt_tonemap_kernel's colour math (path_kernel.hip; rt/render.cuh:44-53) on a float RGB buffer
__global__ void __launch_bounds__(256) rt_tonemap_rgb_kernel(const Vec3D *rgb, RtUChar4 *out, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Vec3D c = rt_correct_color(rgb[i]);
    RtUChar4 o;
    o.x = (uint8_t)(c.x * RT_MAX_COLOR_CHANNEL);
    o.y = (uint8_t)(c.y * RT_MAX_COLOR_CHANNEL);
    o.z = (uint8_t)(c.z * RT_MAX_COLOR_CHANNEL);
    o.w = RT_MAX_COLOR_CHANNEL;
    out[i] = o;
}

// One denoise workspace per device, sized to the last frame: the two
// ping-pong state buffers, the packed guides and the depth slopes (52 B per
// pixel).  One call at a time may use it, in rt_workspace.h's order: a frame
// of another size waits on the host for the last call before the buffers are
// replaced.
struct DenoiseWorkspace {
    RtDn4 *state[2] = {nullptr, nullptr};
    RtDn4 *guide = nullptr;
    float *slope = nullptr;
    size_t pixels = 0;
    SerialEvent serial;
};
DeviceSlots<DenoiseWorkspace> g_denoise;

void free_buffers(DenoiseWorkspace &w)
{
    (void)w.serial.wait_host(); // the buffers' last user, on whatever stream
    if (w.state[0]) (void)hipFree(w.state[0]);
    if (w.state[1]) (void)hipFree(w.state[1]);
    if (w.guide) (void)hipFree(w.guide);
    if (w.slope) (void)hipFree(w.slope);
    w.state[0] = w.state[1] = w.guide = nullptr;
    w.slope = nullptr;
    w.pixels = 0;
}

bool size_workspace(DenoiseWorkspace &w, size_t n)
{
    if (w.pixels == n) return true;
    free_buffers(w);
    void *p[4] = {nullptr, nullptr, nullptr, nullptr};
    const size_t bytes[4] = {n * sizeof(RtDn4), n * sizeof(RtDn4), n * sizeof(RtDn4), n * sizeof(float)};
    for (int i = 0; i < 4; ++i) {
        if (hipMalloc(&p[i], bytes[i]) != hipSuccess) {
            for (int j = 0; j < i; ++j) (void)hipFree(p[j]);
            return false;
        }
    }
    w.state[0] = (RtDn4 *)p[0];
    w.state[1] = (RtDn4 *)p[1];
    w.guide = (RtDn4 *)p[2];
    w.slope = (float *)p[3];
    w.pixels = n;
    return true;
}

// the prepare pass and the levels on `stream` (the workspace is sized and `stream` waits for its last user)
template <bool WRAP_X>
void launch_levels(DenoiseWorkspace &w, const Vec3D *fb, const float *sq, const int *count, const float *depth,
                   const float *normal, const float *albedo, int width, int height, float *rgb_out,
                   const RtDnParams &prm, hipStream_t stream)
{
    const dim3 block(DN_TILE_W, DN_TILE_H);
    // (a 1-D grid of tiles, row by row: up to 2^31 / 256 + width / 32 + height / 8 blocks, within the x limit)
    const int tiles_x = (width + DN_TILE_W - 1) / DN_TILE_W;
    const dim3 grid((unsigned)((long long)tiles_x * ((height + DN_TILE_H - 1) / DN_TILE_H)));
    hipLaunchKernelGGL(dn_prepare_kernel<WRAP_X>, grid, block, 0, stream, fb, sq, count, depth, normal, albedo, width, height,
                       tiles_x, prm.demodulate, w.state[0], w.guide, w.slope);
    for (int s = 0; s < prm.iterations; ++s) {
        const RtDn4 *in = w.state[s & 1];
        if (s + 1 < prm.iterations)
            hipLaunchKernelGGL((dn_filter_kernel<false, WRAP_X>), grid, block, 0, stream, in, w.guide, w.slope, width, height,
                               tiles_x, 1 << s, prm, w.state[(s + 1) & 1], albedo, rgb_out);
        else
            hipLaunchKernelGGL((dn_filter_kernel<true, WRAP_X>), grid, block, 0, stream, in, w.guide, w.slope, width, height,
                               tiles_x, 1 << s, prm, (RtDn4 *)nullptr, albedo, rgb_out);
    }
}

} // namespace

// ---- launchers (called by abi.hip) ----
int rt_launch_denoise(const Vec3D *fb, const float *sq, const int *count, const float *depth, const float *normal,
                      const float *albedo, int width, int height, float *rgb_out, const RtDnParams &prm,
                      hipStream_t stream, int wrap_x)
{
    std::lock_guard<std::mutex> g(g_denoise.mu);
    DenoiseWorkspace *slot = g_denoise.current();
    if (!slot) return -1;
    DenoiseWorkspace &w = *slot;
    if (!size_workspace(w, (size_t)width * height) || !w.serial.wait_on(stream)) return -1;
    if (wrap_x) launch_levels<true>(w, fb, sq, count, depth, normal, albedo, width, height, rgb_out, prm, stream);
    else launch_levels<false>(w, fb, sq, count, depth, normal, albedo, width, height, rgb_out, prm, stream);
    return w.serial.record(stream) ? 0 : -1;
}

int rt_launch_tonemap_rgb(const float *rgb, RtUChar4 *out, int n, hipStream_t stream)
{
    hipLaunchKernelGGL(rt_tonemap_rgb_kernel, dim3((n + 255) / 256), dim3(256), 0, stream,
                       reinterpret_cast<const Vec3D *>(rgb), out, n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

void rt_denoise_shutdown()
{
    g_denoise.shutdown([](DenoiseWorkspace &w) {
        free_buffers(w);
        w.serial.destroy();
    });
}
