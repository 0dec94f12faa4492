// query.hip — the batched ray query (rt_trace_rays), the occlusion query
// (rt_occluded), the radiance queries (rt_trace_paths, rt_sample_paths), the
// ray generators (rt_camera_rays, rt_sampler_rays) and the first-hit AOV pass
// (rt_render_aov).
//
// The closest-hit query is the renderer's own: trace_ray (rt/trace_ray.cuh:
// 244-318) as rt_kernels.h trace() restates it, sped up by the conservative
// BVH bound of bvh_trace.h where that bound is proven — and surface
// reconstruction is the renderer's shade().  One persistent kernel template
// over (ray source, sink):
//
//   rt_trace_rays   rays from a buffer      -> hit (+ surface) records
//   rt_render_aov   rays from the camera    -> planar AOV buffers
//   rt_sample_aov   a sampler's centre rays -> planar AOV buffers
// and a second kernel of the same shape for the any-hit question:
//   rt_occluded     rays + tmax from buffers -> one byte per ray
// and a third that runs the renderer's whole path loop on the caller's rays:
//   rt_trace_paths  rays + RNG states        -> summed radiance per ray
//   rt_sample_paths a sampler + RNG states   -> summed radiance per element
//   rt_sample_paths_adaptive  the same, the renderer's adaptive test before every sample
//
// One ray per lane; the lanes of a wave take their next rays together from a
// global counter (one wave-aggregated atomic per round).  The traversal stack
// is Stack<RQ_LDS> in LDS with a per-thread HBM spill area.
//
// The domain gate.  trace_bvh's bound is argued (bvh_common.h rt_slab) for
// the rays a renderer makes: unit directions.  rt_slab clamps 1 / d to
// +-2^60 and argues from "t <= the scene box's exit <= 6 scale", which holds
// for |d| ~ 1 only: at |d| ~ 2^-58 and below every axis is clamped, the slab
// distances no longer are the ray's, and boxes holding the hit are culled (a
// wrong s_min, a wrong hit).  A public query takes any 6 floats, so the bound
// is applied only to rays with 0.5 <= max(|d.x|, |d.y|, |d.z|) <= 2 (every
// unit direction: its largest component is >= 1/sqrt(3)) that rt_bounded_ray
// admits; every other ray runs trace<false>(), the reference's traversal
// itself.  Either way the result is trace_ray's, bit for bit.
#include <hip/hip_runtime.h>

#include "bvh_trace.h"
#include "camera_math.h"
#include "convergence_math.h"
#include "path_event.h"
#include "rt_kernels.h"
#include "rt_launch.h"
#include "rt_workspace.h"
#include "sampler_math.h"

#define RQ_BLOCK 256
#ifndef RQ_LDS
#define RQ_LDS 10 // stack entries in LDS (20 KB per block); deeper ones spill to HBM
#endif
#ifndef RQ_WAVES
#define RQ_WAVES 4 // waves per SIMD = resident blocks per CU
#endif
#ifndef PQ_LDS
#define PQ_LDS 10 // rt_path_query_kernel: as RQ_LDS (the shared spill area holds the entries past RQ_LDS)
#endif
#ifndef PQ_WAVES
#define PQ_WAVES 4 // rt_path_query_kernel: resident blocks per CU (<= RQ_WAVES: the spill area's threads)
#endif
#ifndef RQ_COUNT_EARLY
#define RQ_COUNT_EARLY 0 // 1: rt_occluded's stats get a fourth word (a counting build, never the shipped one)
#endif

using namespace rtk;

namespace {

// the pixel centre's direction (camera_math.h rt_camera_centre_dir, the text
// rt_reproject shares), the camera position itself as the origin
__device__ __forceinline__ void camera_ray_centre(const RtDevCamera &cam, int half_w, int half_h, int x, int y,
                                                  Vec3D &ro, Vec3D &rd)
{
    rd = rt_camera_centre_dir(cam, half_w, half_h, x, y);
    ro = rt_v3(cam.pos[0], cam.pos[1], cam.pos[2]);
}

// ---- ray sources ----
struct BufferRays { // n x 6 floats (o.xyz d.xyz), 8-B aligned: three 8-B loads, 1,536 contiguous bytes per wave
    static constexpr bool per_sample = false; // rt_path_query_kernel: loaded once per ray
    const float2 *rays;
    __device__ __forceinline__ void load(uint32_t e, Vec3D &o, Vec3D &d) const
    {
        const float2 *p = rays + 3 * (size_t)e;
        const float2 a = p[0], b = p[1], c = p[2];
        o = rt_v3(a.x, a.y, b.x);
        d = rt_v3(b.y, c.x, c.y);
    }
};
struct SamplerRays { // sampler_math.h: element e's next ray, drawn from the element's own RNG state
    static constexpr bool per_sample = true; // rt_path_query_kernel: drawn once per sample
    RtDevSampler smp;
    int *count; // sample_count_device (optional)
    __device__ __forceinline__ void sample(uint32_t e, uint32_t &st, Vec3D &o, Vec3D &d) const
    {
        rt_sampler_ray<false>(smp, e, st, o, d);
    }
    __device__ __forceinline__ void done(uint32_t e, int samples, int accumulate) const
    {
        if (count) count[e] = (accumulate ? count[e] : 0) + samples;
    }
};
struct CentreRays { // sampler_math.h: element e's centre ray of an image sampler (rt_sample_aov), nothing drawn
    RtDevSampler smp;
    __device__ __forceinline__ void load(uint32_t e, Vec3D &o, Vec3D &d) const
    {
        uint32_t st = 0; // (unused: a centre ray draws nothing)
        rt_sampler_ray<true>(smp, e, st, o, d);
    }
};
struct CameraRays { // ray e = the centre of pixel (e % width, e / width), row 0 = bottom
    RtDevCamera cam;
    int width, half_w, half_h;
    __device__ __forceinline__ void load(uint32_t e, Vec3D &o, Vec3D &d) const
    {
        camera_ray_centre(cam, half_w, half_h, (int)(e % (uint32_t)width), (int)(e / (uint32_t)width), o, d);
    }
};

// ---- sinks ----
struct SurfaceOut { // RtRaySurface's fields
    Vec3D position, normal, tangent, albedo, emittance;
    float t;
};
struct RecordSink { // RtRayHit (one 16-B store) and, if asked for, RtRaySurface (five 16-B stores)
    float4 *hits;
    float4 *surface;
    __device__ __forceinline__ bool wants_surface() const { return surface != nullptr; }
    __device__ __forceinline__ void hit(uint32_t e, int tri, float bx, float by, float bz) const
    {
        hits[e] = make_float4(__int_as_float(tri), bx, by, bz);
    }
    __device__ __forceinline__ void surf(uint32_t e, int, const SurfaceOut &s) const
    {
        float4 *r = surface + 5 * (size_t)e;
        r[0] = make_float4(s.position.x, s.position.y, s.position.z, s.t);
        r[1] = make_float4(s.normal.x, s.normal.y, s.normal.z, 0.0f);
        r[2] = make_float4(s.tangent.x, s.tangent.y, s.tangent.z, 0.0f);
        r[3] = make_float4(s.albedo.x, s.albedo.y, s.albedo.z, 0.0f);
        r[4] = make_float4(s.emittance.x, s.emittance.y, s.emittance.z, 0.0f);
    }
};
struct AovSink { // RtAovBuffers: one array per AOV, any may be null
    float *depth;
    float *normal;
    float *albedo;
    int *triangle;
    __device__ __forceinline__ bool wants_surface() const { return depth || normal || albedo; }
    __device__ __forceinline__ void hit(uint32_t e, int tri, float, float, float) const
    {
        if (triangle) triangle[e] = tri;
    }
    __device__ __forceinline__ void surf(uint32_t e, int, const SurfaceOut &s) const
    {
        if (depth) depth[e] = s.t;
        if (normal) {
            float *p = normal + 3 * (size_t)e;
            p[0] = s.normal.x;
            p[1] = s.normal.y;
            p[2] = s.normal.z;
        }
        if (albedo) {
            float *p = albedo + 3 * (size_t)e;
            p[0] = s.albedo.x;
            p[1] = s.albedo.y;
            p[2] = s.albedo.z;
        }
    }
};

// whether the bound's argument covers this direction (a NaN component fails the first part)
__device__ __forceinline__ bool direction_in_domain(Vec3D d)
{
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    return (ax <= 2.0f && ay <= 2.0f && az <= 2.0f) && (ax >= 0.5f || ay >= 0.5f || az >= 0.5f);
}

// the domain gate (see the head of this file): whether the bounded traversal may take this ray
__device__ __forceinline__ bool in_bounded_domain(const RtDevScene &sc, int kd_only, Vec3D o, Vec3D d)
{
    return !kd_only && direction_in_domain(d) && rt_bounded_ray(o, d, sc.split_vals, sc.split_off);
}

// the closest hit of (o, d) by the bounded traversal inside the gate, by the plain KD traversal outside
// it (ran_kd): trace_ray's result either way
template <typename STACK>
__device__ __forceinline__ int query_trace(const RtDevScene &sc, int kd_only, Vec3D o, Vec3D d, float &bx, float &by,
                                           float &bz, STACK &stk, Cnt &c, bool &ran_kd)
{
    ran_kd = !in_bounded_domain(sc, kd_only, o, d);
    if (ran_kd) return trace<false>(sc, o, d, bx, by, bz, stk, c);
    return trace_bvh<false>(sc, o, d, bx, by, bz, stk, c);
}

// stats[k] += the wave's sum of lane_counts[k], by lane 0 and only where the sum is not zero (every lane
// of the wave calls this: the kernels' loop exits reconverge before it)
template <int N>
__device__ __forceinline__ void flush_stats(unsigned long long *stats, const uint32_t (&lane_counts)[N], int lane)
{
    unsigned long long total[N];
    for (int k = 0; k < N; ++k) {
        total[k] = lane_counts[k];
        for (int off = 32; off > 0; off >>= 1) total[k] += __shfl_xor(total[k], off);
    }
    if (lane != 0) return;
    for (int k = 0; k < N; ++k)
        if (total[k]) atomicAdd(stats + k, total[k]);
}

// one ray's result into the sink: the hit record, and the surface (the renderer's shade()) if asked for
template <typename SINK>
__device__ __forceinline__ void store_result(const RtDevScene &sc, const SINK &sink, uint32_t e, Vec3D o, Vec3D d,
                                             int tri, float bx, float by, float bz)
{
    if (tri < 0) bx = by = bz = 0.0f;
    sink.hit(e, tri, bx, by, bz);
    if (!sink.wants_surface()) return;
    SurfaceOut so;
    if (tri >= 0) {
        Surface s;
        Cnt c; // (not counted)
        shade<false>(sc, tri, bx, by, bz, d, s, c);
        so.position = s.position;
        so.normal = s.normal;
        so.tangent = s.tangent;
        so.albedo = s.albedo;
        so.emittance = s.emittance;
        so.t = rt_magnitude(s.position - o);
    } else {
        const Vec3D z = rt_v3(0.0f, 0.0f, 0.0f);
        so.position = so.normal = so.tangent = so.albedo = so.emittance = z;
        so.t = INFINITY;
    }
    sink.surf(e, tri, so);
}

// n rays of `src` into `sink`.  kd_only: RT_TRAVERSAL_KD (or a scene without a
// BVH).  fetch: the launch's ray counter (zeroed before the launch).  stats
// (optional) adds [0] rays, [1] hits, [2] rays traced by the plain KD traversal.
template <typename SRC, typename SINK>
__global__ void __launch_bounds__(RQ_BLOCK, RQ_WAVES)
    rt_query_kernel(RtDevScene sc, SRC src, SINK sink, uint32_t n, int kd_only, uint32_t *fetch,
                    unsigned long long *stats, uint2 *spill, int spill_threads)
{
    __shared__ uint32_t s_node[RQ_LDS * RQ_BLOCK];
    __shared__ float s_entry[RQ_LDS * RQ_BLOCK];
    const int tid = threadIdx.x;
    const int gtid = blockIdx.x * RQ_BLOCK + tid;
    Stack<RQ_LDS> stk{s_node + tid, s_entry + tid, RQ_BLOCK, spill + gtid, spill_threads};
    Cnt c; // (never counted: every traversal below is the COUNT = false build)
    const int lane = __lane_id();
    uint32_t n_rays = 0, n_hits = 0, n_kd = 0;
    while (true) {
        const uint32_t e = wave_next_index(fetch, lane);
        if (e >= n) break;
        Vec3D o, d;
        src.load(e, o, d);
        float bx = 0.0f, by = 0.0f, bz = 0.0f;
        bool ran_kd;
        const int tri = query_trace(sc, kd_only, o, d, bx, by, bz, stk, c, ran_kd);
        if (ran_kd) ++n_kd;
        ++n_rays;
        if (tri >= 0) ++n_hits;
        store_result(sc, sink, e, o, d, tri, bx, by, bz);
    }
    if (stats) flush_stats(stats, {n_rays, n_hits, n_kd}, lane);
}

// ---- the occlusion query (rt_occluded) ----
struct BufferRaysTmax { // BufferRays and the ray's tmax (NULL: +inf for every ray)
    BufferRays rays;
    const float *tmax;
    __device__ __forceinline__ void load(uint32_t e, Vec3D &o, Vec3D &d, float &t) const
    {
        rays.load(e, o, d);
        t = tmax ? tmax[e] : INFINITY;
    }
};
struct ByteSink { // one byte per ray, any alignment
    uint8_t *out;
    __device__ __forceinline__ void store(uint32_t e, bool occluded) const { out[e] = occluded ? 1 : 0; }
};

// rt_query_kernel's shape for the any-hit question: occluded[e] = trace_ray
// hits ray e with a ray parameter s < tmax[e].  A ray with !(tmax > 1e-5) is
// not traced (no test passes below 1e-5).  Inside the domain gate the capped
// s_min query answers most unoccluded rays alone (bvh_trace.h occluded_bvh);
// outside it the plain KD traversal gives the hit's s.  stats (optional) adds
// [0] rays, [1] occluded rays, [2] rays that ran the plain KD traversal.
// (RQ_COUNT_EARLY: a counting build for tools/occlusion_bench.py — stats then
// has a fourth word, the rays the capped query answered alone.)
template <typename SRC, typename SINK>
__global__ void __launch_bounds__(RQ_BLOCK, RQ_WAVES)
    rt_occluded_kernel(RtDevScene sc, SRC src, SINK sink, uint32_t n, int kd_only, uint32_t *fetch,
                       unsigned long long *stats, uint2 *spill, int spill_threads)
{
    __shared__ uint32_t s_node[RQ_LDS * RQ_BLOCK];
    __shared__ float s_entry[RQ_LDS * RQ_BLOCK];
    const int tid = threadIdx.x;
    const int gtid = blockIdx.x * RQ_BLOCK + tid;
    Stack<RQ_LDS> stk{s_node + tid, s_entry + tid, RQ_BLOCK, spill + gtid, spill_threads};
    Cnt c; // (never counted)
    const int lane = __lane_id();
    uint32_t n_rays = 0, n_occ = 0, n_kd = 0, n_early = 0;
    while (true) {
        const uint32_t e = wave_next_index(fetch, lane);
        if (e >= n) break;
        Vec3D o, d;
        float tmax;
        src.load(e, o, d, tmax);
        bool occ = false;
        if (tmax > 0.00001f) { // (false for a NaN)
            if (in_bounded_domain(sc, kd_only, o, d)) {
                bool early;
                occ = occluded_bvh(sc, o, d, tmax, stk, c, early);
                if (RQ_COUNT_EARLY && early) ++n_early;
            } else {
                float s = INFINITY;
                occ = trace_s(sc, o, d, s, stk, c) >= 0 && s < tmax;
                ++n_kd;
            }
        }
        ++n_rays;
        if (occ) ++n_occ;
        sink.store(e, occ);
    }
    if (stats) {
        flush_stats(stats, {n_rays, n_occ, n_kd}, lane);
        if (RQ_COUNT_EARLY) flush_stats(stats + 3, {n_early}, lane);
    }
}

// ---- the radiance query (rt_trace_paths) ----
// trace_path (rt/path_tracing.cuh:268-325) for the caller's rays: ray e is
// traced `samples` times from rng[e], started as the renderer starts a camera
// ray (PRIMARY, outside every medium, throughput 1), and the sums of L and of
// luminance(L)^2 (:322-324) go to radiance[e] / sq[e], the RNG state back to
// rng[e].  The loop has rt_path_kernel's shape (path_kernel.hip) and runs the
// same events (path_event.h): one ray query per iteration from one place,
// extension and NEE shadow rays as two states of it, the path state in
// registers.
//
// Regeneration is per lane: a lane whose path ends starts its ray's next
// sample in the same iteration, and a lane whose ray is done stores it and
// takes the next ray index from the launch's counter — one atomic for the
// lanes of the wave that need a ray in that iteration.  (Path lengths run
// from 1 to ~10^4 extension rays in glass: a refill in lockstep, as
// rt_query_kernel's, would hold 63 lanes for the longest path of every
// round.)  A lane leaves when the counter is past n.
//
// The gate is applied to every query: the caller's ray may be any 6 floats;
// the rays scatter() and NEE make are unit directions and pass its first part.
// stats (optional) adds [0] rays, [1] paths, [2] trace_ray calls, [3] paths
// cut at `limit`; [4] is the longest path (a maximum).  The per-lane counts
// are 32-bit: a lane makes fewer than 2^32 queries in any launch that ends.
//
// SRC: BufferRays (rt_trace_paths) loads the caller's ray once and restarts
// every sample from it; SamplerRays (rt_sample_paths) draws each sample's ray
// from p.rng where that restart stands — in the iteration the lane's previous
// path ended in, like any other regeneration — and keeps the element's
// sample count.
//
// ADAPT (rt_sample_paths_adaptive; SamplerRays with sq_out and src.count
// given): the lane keeps its element's sample count, and the adaptive test
// (rt_kernels.h adaptive_run, rt_render's own, on min_samples / tolerance /
// z_const) stands at the regeneration point, before each of the element's
// `samples` passes.  A pass the test refuses draws nothing and leaves the sums
// as they were, so every later pass of the call would be refused too: the
// element is done.  It stores its records and the lane takes the next index
// within the same iteration — a wave of converged elements spends no ray
// query on them.  With `accumulate` an element that took no sample is not
// stored: its records would be rewritten with the bits they hold.
template <typename SRC, bool ADAPT>
__global__ void __launch_bounds__(RQ_BLOCK, PQ_WAVES)
    rt_path_query_kernel(RtDevScene sc, SRC src, uint32_t *rng_io, float *radiance, float *sq_out, uint32_t n,
                         int samples, int limit, int accumulate, int kd_only, uint32_t *fetch,
                         unsigned long long *stats, uint2 *spill, int spill_threads, int min_samples, float tolerance,
                         float z_const)
{
    static_assert(!ADAPT || SRC::per_sample, "the adaptive test needs the sampler's per-element count");
    __shared__ uint32_t s_node[PQ_LDS * RQ_BLOCK];
    __shared__ float s_entry[PQ_LDS * RQ_BLOCK];
    const int tid = threadIdx.x;
    const int gtid = blockIdx.x * RQ_BLOCK + tid;
    Stack<PQ_LDS> stk{s_node + tid, s_entry + tid, RQ_BLOCK, spill + gtid, spill_threads};
    Cnt c; // (never counted)
    const int lane = __lane_id();
    uint32_t n_rays = 0, n_paths = 0, n_trace = 0, n_cut = 0, max_len = 0;

    uint32_t e = 0;
    bool have_ray = false, have_path = false;
    int samples_left = 0;
    Vec3D o0 = rt_v3(0, 0, 0), d0 = rt_v3(0, 0, 0); // the caller's ray
    Vec3D sum = rt_v3(0, 0, 0);
    float sum_sq = 0.0f;
    PathState p; // (p.rng: the ray's RNG state, carried from sample to sample)
    int cnt = 0;        // ADAPT: the element's sample count
    bool taken = false; // ADAPT: the element took a sample in this call
    RtDevFrame afr;     // ADAPT: the fields adaptive_run reads
    if constexpr (ADAPT) {
        afr.adaptive = 1;
        afr.min_samples = min_samples;
        afr.tolerance = tolerance;
        afr.z_const = z_const;
    }

    while (true) {
        if (!have_path) {
            if constexpr (ADAPT) {
                bool leave = false;
                while (true) { // one round per element that the test stops before its first sample of the call
                    if (samples_left == 0) {
                        if (have_ray && (taken || !accumulate)) { // the finished element's records
                            float *r = radiance + 3 * (size_t)e;
                            r[0] = sum.x;
                            r[1] = sum.y;
                            r[2] = sum.z;
                            sq_out[e] = sum_sq;
                            rng_io[e] = p.rng;
                            src.count[e] = cnt;
                        }
                        have_ray = false;
                        const uint32_t next = wave_next_index(fetch, lane); // for the lanes that are here
                        if (next >= n) {
                            leave = true;
                            break;
                        }
                        e = next;
                        p.rng = rng_io[e];
                        sum = rt_v3(0.0f, 0.0f, 0.0f);
                        sum_sq = 0.0f;
                        cnt = 0;
                        if (accumulate) {
                            const float *r = radiance + 3 * (size_t)e;
                            sum = rt_v3(r[0], r[1], r[2]);
                            sum_sq = sq_out[e];
                            cnt = src.count[e];
                        }
                        have_ray = true;
                        taken = false;
                        samples_left = samples;
                        ++n_rays;
                    }
                    if (adaptive_run(afr, sum, sum_sq, cnt)) break;
                    samples_left = 0; // this pass is used up, and so is every later one of the call: the state stays
                }
                if (leave) break;
                taken = true;
            } else if (samples_left == 0) { // (its own block on purpose: shared with ADAPT's loop, these
                                            // instantiations' register allocation changed)
                if (have_ray) { // the finished ray's records
                    float *r = radiance + 3 * (size_t)e;
                    r[0] = sum.x;
                    r[1] = sum.y;
                    r[2] = sum.z;
                    if (sq_out) sq_out[e] = sum_sq;
                    rng_io[e] = p.rng;
                    if constexpr (SRC::per_sample) src.done(e, samples, accumulate);
                    have_ray = false;
                }
                const uint32_t next = wave_next_index(fetch, lane); // for the lanes that are here
                if (next >= n) break;
                e = next;
                if constexpr (!SRC::per_sample) src.load(e, o0, d0);
                p.rng = rng_io[e];
                sum = rt_v3(0.0f, 0.0f, 0.0f);
                sum_sq = 0.0f;
                if (accumulate) {
                    const float *r = radiance + 3 * (size_t)e;
                    sum = rt_v3(r[0], r[1], r[2]);
                    if (sq_out) sum_sq = sq_out[e];
                }
                have_ray = true;
                samples_left = samples;
                ++n_rays;
            }
            --samples_left;
            if constexpr (SRC::per_sample) {
                src.sample(e, p.rng, p.ro, p.rd);
            } else {
                p.ro = o0;
                p.rd = d0;
            }
            path_begin(p, 0);
            have_path = true;
            ++n_paths;
        }

        bool finish = false;
        if (!p.shadow && p.depth == limit) { // max_depth / watchdog
            ++n_cut;
            finish = true;
        } else {
            if (!p.shadow) ++p.depth;
            ++n_trace;
            float bx = 0.0f, by = 0.0f, bz = 0.0f;
            bool ran_kd;
            const int hit = query_trace(sc, kd_only, p.ro, p.rd, bx, by, bz, stk, c, ran_kd);
            bool roulette = true;
            if (!p.shadow) {
                if (hit < 0) {
                    finish = true; // miss: break without roulette (:303-306)
                    roulette = false;
                } else {
                    Surface s;
                    if (path_bounce<false>(sc, p, hit, bx, by, bz, s, c)) roulette = false; // ... after the shadow ray
                }
            } else {
                path_shadow_result<false>(sc, p, hit, bx, by, bz, c);
            }
            if (roulette && !path_roulette(p)) finish = true;
        }
        if (finish) { // accumulation (:322-324)
            sum = sum + p.L;
            sum_sq = sum_sq + rt_square(rt_luminance(p.L));
            if constexpr (ADAPT) ++cnt;
            max_len = (uint32_t)p.depth > max_len ? (uint32_t)p.depth : max_len;
            have_path = false;
        }
    }

    if (stats) {
        flush_stats(stats, {n_rays, n_paths, n_trace, n_cut}, lane);
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t other = __shfl_xor(max_len, off);
            max_len = other > max_len ? other : max_len;
        }
        if (lane == 0 && max_len) atomicMax(stats + 4, (unsigned long long)max_len);
    }
}

// rt_sampler_rays: element e's next ray (CENTRE: its centre ray, no RNG), three 8-B stores per lane
template <bool CENTRE>
__global__ void __launch_bounds__(RQ_BLOCK) rt_sampler_rays_kernel(RtDevSampler smp, uint32_t *rng, float2 *rays, uint32_t n)
{
    const uint32_t e = blockIdx.x * RQ_BLOCK + threadIdx.x;
    if (e >= n) return;
    uint32_t st = 0;
    if (!CENTRE) st = rng[e];
    Vec3D o, d;
    rt_sampler_ray<CENTRE>(smp, e, st, o, d);
    if (!CENTRE) rng[e] = st;
    float2 *p = rays + 3 * (size_t)e;
    p[0] = make_float2(o.x, o.y);
    p[1] = make_float2(o.z, d.x);
    p[2] = make_float2(d.y, d.z);
}

// rt_camera_rays: ray y*W + x = the centre of pixel (x, y), three 8-B stores per lane
__global__ void __launch_bounds__(RQ_BLOCK) rt_camera_rays_kernel(CameraRays src, float2 *rays, uint32_t n)
{
    const uint32_t e = blockIdx.x * RQ_BLOCK + threadIdx.x;
    if (e >= n) return;
    Vec3D o, d;
    src.load(e, o, d);
    float2 *p = rays + 3 * (size_t)e;
    p[0] = make_float2(o.x, o.y);
    p[1] = make_float2(o.z, d.x);
    p[2] = make_float2(d.y, d.z);
}

// ---- host side ----
// One query workspace per device: the launch's ray counter and the stack
// spill area (indexed by the resident grid's global thread id), so one query
// kernel at a time may use it, in rt_workspace.h's order.  Its size depends
// on the device alone: nothing is ever replaced.
struct QueryWorkspace {
    uint2 *spill = nullptr;
    size_t spill_threads = 0;
    uint32_t *fetch = nullptr;
    SerialEvent serial;
    int blocks = 0; // the resident grid: RQ_WAVES blocks per CU
};
DeviceSlots<QueryWorkspace> g_query;

// max(RT_STACK_DEPTH, RT_BVH_STACK) entries in all: the KD part needs <= RT_STACK_DEPTH, the BVH part <= RT_BVH_STACK
constexpr int kSpillDepth = (RT_BVH_STACK > RT_STACK_DEPTH ? RT_BVH_STACK : RT_STACK_DEPTH) - RQ_LDS;

// (kernel: rt_query_kernel or rt_occluded_kernel — one signature, one workspace)
template <typename SRC, typename SINK>
using QueryKernel = void (*)(RtDevScene, SRC, SINK, uint32_t, int, uint32_t *, unsigned long long *, uint2 *, int);

// The device's workspace, made on first use, with `stream` waiting for the
// previous launch that used it and the ray counter zeroed on `stream`
// (g_query.mu is held by the caller until the launch is recorded); nullptr on error.
QueryWorkspace *query_workspace(hipStream_t stream)
{
    QueryWorkspace *slot = g_query.current();
    if (!slot) return nullptr;
    QueryWorkspace &w = *slot;
    if (!w.blocks) {
        int dev = 0;
        hipDeviceProp_t prop;
        const int cus = hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
                                prop.multiProcessorCount > 0
                            ? prop.multiProcessorCount
                            : 256;
        w.blocks = cus * RQ_WAVES;
    }
    if (!w.fetch) {
        void *p = nullptr;
        if (hipMalloc(&p, 64) != hipSuccess) return nullptr;
        w.fetch = (uint32_t *)p;
    }
    const size_t threads = (size_t)w.blocks * RQ_BLOCK;
    if (!w.spill) {
        void *p = nullptr;
        if (hipMalloc(&p, threads * (size_t)kSpillDepth * sizeof(uint2)) != hipSuccess) return nullptr;
        w.spill = (uint2 *)p;
        w.spill_threads = threads;
    }
    if (!w.serial.wait_on(stream)) return nullptr;
    if (hipMemsetAsync(w.fetch, 0, sizeof(uint32_t), stream) != hipSuccess) return nullptr;
    return &w;
}

// the resident grid for n rays at `per_cu` blocks per CU (<= RQ_WAVES: the spill area has w.blocks blocks' slots)
int query_grid(const QueryWorkspace &w, long long n, int per_cu)
{
    const long long need = (n + RQ_BLOCK - 1) / RQ_BLOCK;
    const long long resident = (long long)(w.blocks / RQ_WAVES) * per_cu;
    return (int)(need < resident ? need : resident);
}

bool query_kd_only(const RtDevScene &sc, int traversal)
{
    return traversal == RT_TRAVERSAL_KD || sc.bvh_nodes == nullptr || sc.bvh4 == nullptr;
}

template <typename SRC, typename SINK>
int launch_query(QueryKernel<SRC, SINK> kernel, const RtDevScene &sc, const SRC &src, const SINK &sink, long long n, int traversal,
                 unsigned long long *stats, hipStream_t stream)
{
    std::lock_guard<std::mutex> g(g_query.mu);
    QueryWorkspace *w = query_workspace(stream);
    if (!w) return -1;
    hipLaunchKernelGGL(kernel, dim3(query_grid(*w, n, RQ_WAVES)), dim3(RQ_BLOCK), 0, stream, sc, src, sink, (uint32_t)n,
                       (int)query_kd_only(sc, traversal), w->fetch, stats, w->spill, (int)w->spill_threads);
    return w->serial.record(stream) ? 0 : -1;
}

CameraRays camera_source(const RtDevCamera &cam, int width, int height)
{
    CameraRays s;
    s.cam = cam;
    s.width = width;
    s.half_w = width / 2; // SCREEN_W / 2 (integer division), as rt_render's frame
    s.half_h = height / 2;
    return s;
}

} // namespace

// ---- launchers (called by abi.hip) ----
int rt_launch_trace_rays(const RtDevScene &sc, const float *rays, long long n, void *hits, void *surface, int traversal,
                         unsigned long long *stats, hipStream_t stream)
{
    const BufferRays src{reinterpret_cast<const float2 *>(rays)};
    const RecordSink sink{reinterpret_cast<float4 *>(hits), reinterpret_cast<float4 *>(surface)};
    return launch_query(rt_query_kernel<BufferRays, RecordSink>, sc, src, sink, n, traversal, stats, stream);
}

int rt_launch_occluded(const RtDevScene &sc, const float *rays, const float *tmax, long long n, uint8_t *occluded,
                       int traversal, unsigned long long *stats, hipStream_t stream)
{
    const BufferRaysTmax src{BufferRays{reinterpret_cast<const float2 *>(rays)}, tmax};
    const ByteSink sink{occluded};
    return launch_query(rt_occluded_kernel<BufferRaysTmax, ByteSink>, sc, src, sink, n, traversal, stats, stream);
}

namespace {
// (ad: the adaptive test's constants, ADAPT only)
template <typename SRC, bool ADAPT = false>
int launch_path_query(const RtDevScene &sc, const SRC &src, uint32_t *rng, long long n, float *radiance, float *sq,
                      int samples, int max_depth, int accumulate, int traversal, unsigned long long *stats,
                      hipStream_t stream, const RtCvParams &ad = RtCvParams{0, 0.0f, 0.0f})
{
    static_assert(PQ_WAVES <= RQ_WAVES && PQ_LDS >= RQ_LDS, "rt_path_query_kernel within the shared spill area");
    std::lock_guard<std::mutex> g(g_query.mu);
    QueryWorkspace *w = query_workspace(stream);
    if (!w) return -1;
    hipLaunchKernelGGL((rt_path_query_kernel<SRC, ADAPT>), dim3(query_grid(*w, n, PQ_WAVES)), dim3(RQ_BLOCK), 0, stream, sc,
                       src, rng, radiance, sq, (uint32_t)n, samples, max_depth > 0 ? max_depth : RT_WATCHDOG_BOUNCES,
                       accumulate, (int)query_kd_only(sc, traversal), w->fetch, stats, w->spill, (int)w->spill_threads,
                       ad.min_samples, ad.tolerance, ad.z_const);
    return w->serial.record(stream) ? 0 : -1;
}
} // namespace

int rt_launch_trace_paths(const RtDevScene &sc, const float *rays, uint32_t *rng, long long n, float *radiance, float *sq,
                          int samples, int max_depth, int accumulate, int traversal, unsigned long long *stats,
                          hipStream_t stream)
{
    return launch_path_query(sc, BufferRays{reinterpret_cast<const float2 *>(rays)}, rng, n, radiance, sq, samples,
                             max_depth, accumulate, traversal, stats, stream);
}

int rt_launch_sample_paths(const RtDevScene &sc, const RtDevSampler &smp, uint32_t *rng, long long n, float *radiance,
                           float *sq, int *count, int samples, int max_depth, int accumulate, int traversal,
                           unsigned long long *stats, hipStream_t stream, const RtCvParams *adaptive)
{
    if (adaptive) // (sq and count are given: abi.hip checks)
        return launch_path_query<SamplerRays, true>(sc, SamplerRays{smp, count}, rng, n, radiance, sq, samples,
                                                    max_depth, accumulate, traversal, stats, stream, *adaptive);
    return launch_path_query(sc, SamplerRays{smp, count}, rng, n, radiance, sq, samples, max_depth, accumulate,
                             traversal, stats, stream);
}

int rt_launch_sampler_rays(const RtDevSampler &smp, uint32_t *rng, long long n, float *rays, hipStream_t stream)
{
    const dim3 grid((uint32_t)((n + RQ_BLOCK - 1) / RQ_BLOCK)), block(RQ_BLOCK);
    if (rng)
        hipLaunchKernelGGL(rt_sampler_rays_kernel<false>, grid, block, 0, stream, smp, rng,
                           reinterpret_cast<float2 *>(rays), (uint32_t)n);
    else
        hipLaunchKernelGGL(rt_sampler_rays_kernel<true>, grid, block, 0, stream, smp, rng,
                           reinterpret_cast<float2 *>(rays), (uint32_t)n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rt_launch_render_aov(const RtDevScene &sc, const RtDevCamera &cam, int width, int height, float *depth,
                         float *normal, float *albedo, int *triangle, int traversal, unsigned long long *stats,
                         hipStream_t stream)
{
    const AovSink sink{depth, normal, albedo, triangle};
    return launch_query(rt_query_kernel<CameraRays, AovSink>, sc, camera_source(cam, width, height), sink,
                        (long long)width * height, traversal, stats, stream);
}

int rt_launch_sample_aov(const RtDevScene &sc, const RtDevSampler &smp, long long n, float *depth, float *normal,
                         float *albedo, int *triangle, int traversal, unsigned long long *stats, hipStream_t stream)
{
    const AovSink sink{depth, normal, albedo, triangle};
    return launch_query(rt_query_kernel<CentreRays, AovSink>, sc, CentreRays{smp}, sink, n, traversal, stats, stream);
}

int rt_launch_camera_rays(const RtDevCamera &cam, int width, int height, float *rays, hipStream_t stream)
{
    const uint32_t n = (uint32_t)((long long)width * height);
    hipLaunchKernelGGL(rt_camera_rays_kernel, dim3((n + RQ_BLOCK - 1) / RQ_BLOCK), dim3(RQ_BLOCK), 0, stream,
                       camera_source(cam, width, height), reinterpret_cast<float2 *>(rays), n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

void rt_query_shutdown()
{
    g_query.shutdown([](QueryWorkspace &w) {
        w.serial.destroy();
        if (w.spill) (void)hipFree(w.spill);
        if (w.fetch) (void)hipFree(w.fetch);
    });
}
