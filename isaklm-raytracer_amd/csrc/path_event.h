// path_event.h — one event of trace_path (rt/path_tracing.cuh:268-325) for the loops that run it:
// rt_path_kernel (path_kernel.hip), rt_path_query_kernel (query.hip) and shade_step (wf_shade.h, which
// keeps a copy of path_bounce's text: see there).  Each loop issues one ray query per iteration —
// extension and NEE shadow rays (:235-265) are two states of it — and hands the hit to path_bounce or
// path_shadow_result; the depth limit, its order with the roulette and the accumulation stay with the loop.
// P is the path's state between two ray queries: PathState, or wf_shade.h's PathRegs / PathRegsL (the
// same field names; PathRegsL's rp, cont, snorm and light are LDS proxies, hence templates).
#pragma once
#include "rt_kernels.h"

namespace rtk {

struct PathState { // (as made: path_begin(p, 0)'s state, no ray)
    bool shadow = false; // the pending query is an NEE shadow ray
    bool inside = false; // inside_medium
    int prev_type = PRIMARY, depth = 0, light = 0;
    uint32_t rng = 0;
    Vec3D T = rt_v3(1, 1, 1), L = rt_v3(0, 0, 0); // throughput, radiance so far
    // behind a shadow ray: the light point, the scattered direction, the shading normal
    Vec3D rp = rt_v3(0, 0, 0), cont = rt_v3(0, 0, 0), snorm = rt_v3(0, 0, 0);
    Vec3D ro = rt_v3(0, 0, 0), rd = rt_v3(0, 0, 0); // the ray being traced
};

// a path's first state, its first ray in p.ro / p.rd (depth: the extension rays traced so far)
template <typename P>
__device__ __forceinline__ void path_begin(P &p, int depth)
{
    p.T = rt_v3(1.0f, 1.0f, 1.0f);
    p.L = rt_v3(0.0f, 0.0f, 0.0f);
    p.inside = false;
    p.prev_type = PRIMARY;
    p.depth = depth;
    p.shadow = false;
}

// The extension ray p.ro / p.rd hit `hit`: emission, BSDF sample, throughput, and the NEE set-up of a
// diffuse bounce.  Returns true with p.shadow set and the shadow ray in p.ro / p.rd (the scattered
// direction parked in p.cont: the roulette comes after the shadow ray); false with the next extension
// ray there.  `s` receives the hit's surface: the caller's local, because as a local of this function
// it costs the megakernels registers and scratch (profiles/path_event/resources.txt).
template <bool COUNT, typename P>
__device__ __forceinline__ bool path_bounce(const RtDevScene &sc, P &p, int hit, float bx, float by, float bz, Surface &s,
                                            Cnt &c)
{
    shade<COUNT>(sc, hit, bx, by, bz, p.rd, s, c);
    if (p.prev_type != DIFFUSE) p.L = p.L + s.emittance * p.T; // :285-288
    Vec3D nd, w;
    p.prev_type = scatter(p.rd, p.inside, p.rng, s, nd, w);
    p.T = p.T * w;
    p.ro = s.position;
    p.rd = nd;
    if (p.prev_type != DIFFUSE) return false;
    if (COUNT) c.v[RT_CNT_NEE]++; // sample_direct_light (:235-265)
    float xi = rng_next(p.rng);
    if (sc.light_count == 0) {
        rng_next(p.rng);
        rng_next(p.rng);
        p.L = p.L + rt_v3(0.0f, 0.0f, 0.0f) * p.T;
        return false;
    }
    p.light = sc.lights[(int)(xi * (float)sc.light_count)];
    p.rp = light_point(sc, p.light, p.rng);
    p.cont = p.rd;
    p.snorm = s.normal;
    p.rd = rt_normalize(p.rp - p.ro);
    p.shadow = true;
    return true;
}

// The shadow ray p.ro / p.rd came back with `hit`: the light's contribution if it reached the chosen
// light, and the parked extension ray into p.rd.
template <bool COUNT, typename P>
__device__ __forceinline__ void path_shadow_result(const RtDevScene &sc, P &p, int hit, float bx, float by, float bz,
                                                   Cnt &c)
{
    Vec3D direct = rt_v3(0.0f, 0.0f, 0.0f);
    if (hit >= 0 && hit == p.light) direct = light_contribution(sc, p.light, bx, by, bz, p.ro, p.rd, p.rp, p.snorm);
    if (COUNT && hit >= 0 && material_of(sc, hit).tex) c.v[RT_CNT_TEXEL] += 2; // every hit is shaded
    p.L = p.L + direct * p.T;
    p.rd = p.cont;
    p.shadow = false;
}

// Russian roulette (:309-318): false = the path ends here
template <typename P>
__device__ __forceinline__ bool path_roulette(P &p)
{
    float pr = fmaxf(p.T.x, fmaxf(p.T.y, p.T.z));
    float r = rng_next(p.rng);
    const bool survives = !(r > pr);
    if (survives) p.T = p.T * (1.0f / pr);
    return survives;
}

} // namespace rtk
