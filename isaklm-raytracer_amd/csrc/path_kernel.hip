// path_kernel.hip — the megakernel variant of the render hot path (kernel 0)
// and the tonemap kernel.
//
// Replaces rt/path_tracing.cuh (kernel path_tracing :338-395, trace_path
// :268-325) and the reset_frame / draw_frame kernels of rt/render.cuh:18-59;
// the device arithmetic lives in rt_kernels.h.
//
// Design (MI355X-first, not a translation):
//  * one lane owns one pixel for all `passes` of a launch: RNG state,
//    fb/sq/count live in VGPRs and hit HBM once per launch (the reference
//    does a global read-modify-write per RNG draw and one launch per pass);
//  * a lane whose path ends starts its pixel's next pass immediately (path
//    regeneration), so a wave is not held by its longest path each pass;
//  * every loop iteration issues exactly one ray query from one call site:
//    extension rays and NEE shadow rays (rt/path_tracing.cuh:235-265) are two
//    states of the same loop, so lanes in either state traverse together;
//  * waves are 8x8 pixel tiles and blocks 16x16 tiles, remapped so that each
//    XCD (private L2) renders one contiguous band of the image;
//  * KD stack (node, entry t) in LDS, [depth][lane] => conflict-free.
#include <hip/hip_runtime.h>

#include "bvh_trace.h"
#include "path_event.h"
#include "rt_kernels.h"
#include "rt_launch.h"
#include "rt_workspace.h"

#define RT_BLOCK 256
#ifndef RT_MEGA_BVH_LDS
#define RT_MEGA_BVH_LDS 12 // bounded megakernel: stack entries in LDS; deeper ones spill to HBM
#endif
#ifndef RT_MEGA_BVH_WAVES
#define RT_MEGA_BVH_WAVES 6
#endif

using namespace rtk;

// path_tracing (rt/path_tracing.cuh:338-395) for `passes` passes, with
// reset_frame (rt/render.cuh:18-34) fused in when fr.reset is set.
// BOUNDED: the BVH-bounded traversal (bvh_trace.h), stack entries past STACK
// in `spill` (spill_threads entries apart, indexed by the global thread id)
template <bool COUNT, int STACK, bool BOUNDED>
__global__ void __launch_bounds__(RT_BLOCK, BOUNDED ? RT_MEGA_BVH_WAVES : (STACK <= RT_STACK_SMALL ? 4 : 2))
    rt_path_kernel(RtDevScene sc, RtDevFrame fr, RtDevCamera cam, uint2 *spill, int spill_threads)
{
    __shared__ uint32_t s_node[STACK * RT_BLOCK];
    __shared__ float s_entry[STACK * RT_BLOCK];
    const int tid = threadIdx.x;
    const int tiles_x = (fr.width + 15) / 16;
    const int tile = xcd_tile(blockIdx.x, gridDim.x);
    const int wave = tid >> 6, lane = tid & 63;
    const int x = (tile % tiles_x) * 16 + (wave & 1) * 8 + (lane & 7);
    const int y = (tile / tiles_x) * 16 + (wave >> 1) * 8 + (lane >> 3);
    const bool valid = x < fr.width && y < fr.height && rt_row_owned(fr, y);
    const int pi = valid ? y * fr.width + x : 0;
    Stack<STACK> stk{s_node + tid, s_entry + tid, RT_BLOCK,
                     BOUNDED ? spill + (size_t)blockIdx.x * RT_BLOCK + tid : nullptr, spill_threads};

    Cnt c;
    unsigned long long t_start = 0;
    if (COUNT) {
        c.zero();
        t_start = realtime();
    }

    PathState p; // (p.rng: the pixel's RNG state, carried from path to path)
    Vec3D fb = rt_v3(0.0f, 0.0f, 0.0f);
    float sq = 0.0f;
    int count = 0;
    if (valid) {
        p.rng = fr.rng[pi];
        if (!fr.reset) {
            fb = fr.fb[pi];
            sq = fr.sq[pi];
            count = fr.count[pi];
        }
    }

    int passes_left = valid ? fr.passes : 0;
    bool have_path = false;
    const int limit = fr.max_depth > 0 ? fr.max_depth : RT_WATCHDOG_BOUNCES;

    while (true) {
        if (!have_path) {
            while (passes_left > 0) {
                --passes_left;
                if (!adaptive_run(fr, fb, sq, count)) {
                    if (COUNT) c.v[RT_CNT_SKIP]++;
                    continue;
                }
                camera_ray(fr, cam, x, y, p.rng, p.ro, p.rd);
                path_begin(p, 0);
                have_path = true;
                if (COUNT) c.v[RT_CNT_SAMPLE]++;
                break;
            }
            if (!have_path) break;
        }

        bool finish = false;
        if (!p.shadow && p.depth == limit) { // max_depth / watchdog
            if (COUNT && fr.max_depth <= 0) c.v[RT_CNT_WATCHDOG]++;
            dev_record_cut(fr);
            finish = true;
        } else {
            if (!p.shadow) ++p.depth;
            float bx = 0.0f, by = 0.0f, bz = 0.0f;
            const int hit = BOUNDED ? trace_bvh<false>(sc, p.ro, p.rd, bx, by, bz, stk, c)
                                    : trace<COUNT>(sc, p.ro, p.rd, bx, by, bz, stk, c);
            bool roulette = true;
            if (!p.shadow) {
                if (hit < 0) {
                    finish = true; // miss: break without roulette (:303-306)
                    roulette = false;
                } else {
                    Surface s;
                    if (path_bounce<COUNT>(sc, p, hit, bx, by, bz, s, c)) roulette = false; // ... after the shadow ray
                }
            } else {
                path_shadow_result<COUNT>(sc, p, hit, bx, by, bz, c);
            }
            if (roulette && !path_roulette(p)) finish = true;
        }
        if (finish) { // accumulation (:322-324)
            if (COUNT) c.path_end(p.depth);
            dev_record_end(fr, p.depth);
            fb = fb + p.L;
            sq = sq + rt_square(rt_luminance(p.L));
            ++count;
            have_path = false;
        }
    }

    if (valid) {
        fr.fb[pi] = fb;
        fr.sq[pi] = sq;
        fr.count[pi] = count;
        fr.rng[pi] = p.rng;
    }
    if (COUNT) {
        flush_counters(c, fr.counters);
        if (fr.wave_times && lane == 0) {
            const size_t w = (size_t)blockIdx.x * (RT_BLOCK / 64) + wave;
            fr.wave_times[2 * w] = t_start;
            fr.wave_times[2 * w + 1] = realtime();
        }
    }
}

// draw_frame colour math (rt/render.cuh:44-53) into an RGBA8 HBM buffer
__global__ void __launch_bounds__(256) rt_tonemap_kernel(const Vec3D *fb, const int *count, RtUChar4 *out, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Vec3D c = fb[i] * (1.0f / (float)count[i]);
    c = rt_correct_color(c);
    RtUChar4 o;
    o.x = (uint8_t)(c.x * RT_MAX_COLOR_CHANNEL);
    o.y = (uint8_t)(c.y * RT_MAX_COLOR_CHANNEL);
    o.z = (uint8_t)(c.z * RT_MAX_COLOR_CHANNEL);
    o.w = RT_MAX_COLOR_CHANNEL;
    out[i] = o;
}

// ---- host launchers (called by abi.hip) ----
namespace {
// Per-device spill area of the bounded megakernel (grown on demand), indexed
// by global thread id: one launch at a time may use it, in rt_workspace.h's
// order.
struct MegaSpill {
    uint2 *buf = nullptr;
    size_t entries = 0;
    SerialEvent serial;
};
DeviceSlots<MegaSpill> g_spill;

using PathKernel = void (*)(RtDevScene, RtDevFrame, RtDevCamera, uint2 *, int);
} // namespace

void rt_path_shutdown()
{
    g_spill.shutdown([](MegaSpill &m) {
        m.serial.destroy();
        if (m.buf) (void)hipFree(m.buf);
    });
}

int rt_launch_path(const RtDevScene &sc, const RtDevFrame &fr, const RtDevCamera &cam, int stack_depth,
                   hipStream_t stream, int traversal)
{
    const int tiles = ((fr.width + 15) / 16) * ((fr.height + 15) / 16);
    dim3 grid(tiles), block(RT_BLOCK);
    const bool count = fr.counters != nullptr;
    if (!count && traversal == RT_TRAVERSAL_BOUNDED && sc.bvh_nodes != nullptr) {
        // the bounded traversal: the KD part needs <= RT_STACK_DEPTH entries, the BVH part <= RT_BVH_STACK
        const size_t threads = (size_t)tiles * RT_BLOCK;
        const int deeper = (RT_BVH_STACK > RT_STACK_DEPTH ? RT_BVH_STACK : RT_STACK_DEPTH) - RT_MEGA_BVH_LDS;
        const size_t entries = threads * (size_t)deeper;
        std::lock_guard<std::mutex> g(g_spill.mu);
        MegaSpill *m = g_spill.current();
        if (!m) return -1;
        if (m->entries < entries) {
            if (!m->serial.wait_host()) return -1; // the old buffer's last user
            if (m->buf) (void)hipFree(m->buf);
            m->buf = nullptr;
            m->entries = 0;
            void *p = nullptr;
            if (hipMalloc(&p, entries * sizeof(uint2)) != hipSuccess) return -1;
            m->buf = (uint2 *)p;
            m->entries = entries;
        }
        // the previous launch (maybe on another stream) leaves the spill slots first
        if (!m->serial.wait_on(stream)) return -1;
        hipLaunchKernelGGL((rt_path_kernel<false, RT_MEGA_BVH_LDS, true>), grid, block, 0, stream, sc, fr, cam, m->buf,
                           (int)threads);
        return m->serial.record(stream) ? 0 : -1;
    }
    static const PathKernel plain[2][2] = { // [count][small]
        {rt_path_kernel<false, RT_STACK_DEPTH, false>, rt_path_kernel<false, RT_STACK_SMALL, false>},
        {rt_path_kernel<true, RT_STACK_DEPTH, false>, rt_path_kernel<true, RT_STACK_SMALL, false>}};
    hipLaunchKernelGGL(plain[count][stack_depth <= RT_STACK_SMALL], grid, block, 0, stream, sc, fr, cam,
                       (uint2 *)nullptr, 0);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rt_launch_tonemap(const Vec3D *fb, const int *count, RtUChar4 *out, int n, hipStream_t stream)
{
    hipLaunchKernelGGL(rt_tonemap_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, fb, count, out, n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
