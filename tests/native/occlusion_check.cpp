// occlusion_check.cpp — host restatement of the occlusion query (rt_occluded:
// csrc/query.hip rt_occluded_kernel, csrc/bvh_trace.h occluded_bvh /
// kd_bounded<false, true> / trace_s) checked against its definition on a real scene:
//
//   occluded(ray, tmax) = trace_ray (rt/trace_ray.cuh:244-318) hits && s < tmax
//
// with s the ray parameter of the winning intersect_triangle.  The definition
// is computed by the plain KD traversal (trace_ray itself, IEEE divisions, no
// bound, no tmax anywhere in it); the restatement runs the device's float
// operations: the tmax rule, the domain gate, the s_min query capped at
// min(root exit, tmax), the early "no" and the bounded KD phase with the T*
// leaf.  Every ray is asked with a set of tmax values chosen around its own s:
// +inf, s, nextafter(s, +-inf), s * u for seeded u in [2^-4, 2^4], values
// below the scene box's entry, the root's exit and the special values (NaN,
// +-0, 1e-5f and its neighbours, a denormal, -1, -inf, 1, 3e38).
//
// Both sides are csrc/host/trace_host.h's kd_descent, instantiated apart.
//
// Links the library's host code (rt_host::*): the scene loader, the KD build
// and prepare_host, i.e. the very arrays the GPU gets.
//
// Usage: occlusion_check scene.txt check rays.f32 [seed]   exit 0 = all identical
//        occlusion_check scene.txt dump rays.f32 out.bin   the definition's (hit, triangle, s) per ray:
//                                                          int32, int32, float32
// rays.f32: float32 (n, 6) origin, direction.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "host/trace_host.h"

using namespace trace_host;

namespace {

// ---- the definition: trace_ray, the winning test's s kept — the shared descent with IEEE divisions,
// no bound and no T*, free of the device's shortcuts; it shares no call with the restatement below ----
Hit plain_trace(const rt_host::PreparedHost &h, Vec3D o, Vec3D d)
{
    float entry, exit_;
    if (!scene_box(h, o, d, entry, exit_)) return Hit{};
    return kd_plain(h, o, d, entry, exit_);
}

// ---- the restatement: the device's path ----
long long g_ties = 0, g_early = 0, g_kd_phase = 0, g_plain = 0, g_untraced = 0;
struct Fast : NoObserver {
    long long n = 0; // T* leaves taken
    void tstar_leaf() { ++n; }
} g_fast;

// bvh_trace.h kd_bounded with WANT_S (s_min = -inf, tstar = -1: trace_s): the device's division, and its fall-back
// to the whole leaf where a T* entry does not pass
Hit device_descent(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float entry, float root_exit, float s_min, int tstar)
{
    return kd_descent<DEVICE_DIV, WHOLE_LEAF>(h, o, d, entry, root_exit, s_min, tstar, g_fast);
}

// query.hip rt_occluded_kernel's per-ray part (kd_only: RT_TRAVERSAL_KD)
bool occluded(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float tmax, bool kd_only)
{
    if (!(tmax > 0.00001f)) {
        ++g_untraced;
        return false;
    }
    float entry, exit_;
    if (!kd_only && direction_in_domain(d) && rt_bounded_ray(o, d, h.split_vals.data(), h.split_off)) {
        // bvh_trace.h occluded_bvh
        if (!scene_box(h, o, d, entry, exit_)) return false;
        const float root_exit = exit_;
        const float best0 = fminf(root_exit, tmax);
        const Smin q = bvh4_smin(h, o, d, best0); // bvh4_bound
        if (!(q.best < best0)) {
            ++g_early;
            return false;
        }
        if (q.tk == TK_TIE) ++g_ties;
        ++g_kd_phase;
        const Hit r = device_descent(h, o, d, entry, root_exit, q.best, tstar_of(h, q.tk));
        return r.tri >= 0 && r.s < tmax;
    }
    ++g_plain;
    if (!scene_box(h, o, d, entry, exit_)) return false; // trace_s
    const Hit r = device_descent(h, o, d, entry, exit_, -INFINITY, -1);
    return r.tri >= 0 && r.s < tmax;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 4 || (strcmp(argv[2], "check") != 0 && strcmp(argv[2], "dump") != 0) ||
        (strcmp(argv[2], "dump") == 0 && argc < 5)) {
        fprintf(stderr, "usage: %s scene.txt check rays.f32 [seed] | scene.txt dump rays.f32 out.bin\n", argv[0]);
        return 2;
    }
    RtHostScene scene;
    Camera cam;
    rt_host::PreparedHost h;
    if (!load_prepared(argv[1], scene, cam, h)) return 2;
    if (h.bvh_depth < 0 || h.bvh4.empty()) {
        fprintf(stderr, "no BVH built\n");
        return 2;
    }
    std::vector<float> v;
    if (!read_rays_f32(argv[3], v)) return 2;
    const long long nr = (long long)(v.size() / 6);
    if (strcmp(argv[2], "dump") == 0) {
        FILE *f = fopen(argv[4], "wb");
        if (!f) return 2;
        long long hits = 0;
        for (long long i = 0; i < nr; ++i) {
            const Vec3D o = ray_o(v, (size_t)i), d = ray_d(v, (size_t)i);
            const Hit a = plain_trace(h, o, d);
            const int32_t rec[2] = {a.tri >= 0 ? 1 : 0, a.tri};
            const float s = a.tri >= 0 ? a.s : 0.0f;
            fwrite(rec, sizeof rec, 1, f);
            fwrite(&s, sizeof s, 1, f);
            hits += a.tri >= 0;
        }
        fclose(f);
        printf("rays %lld hits %lld dumped\n", nr, hits);
        return 0;
    }
    std::mt19937_64 rng(argc > 4 ? strtoull(argv[4], nullptr, 10) : 7);
    std::uniform_real_distribution<float> U(-4.0f, 4.0f);
    long long cases = 0, bad = 0, hits = 0, want_occ = 0;
    for (long long i = 0; i < nr; ++i) {
        const Vec3D o = ray_o(v, (size_t)i), d = ray_d(v, (size_t)i);
        const Hit a = plain_trace(h, o, d);
        hits += a.tri >= 0;
        float entry = 0.0f, exit_ = 0.0f;
        const bool box = scene_box(h, o, d, entry, exit_);
        std::vector<float> tm = {INFINITY, NAN, 0.0f, -0.0f, 0.00001f, nextafterf(0.00001f, INFINITY),
                                 nextafterf(0.00001f, -INFINITY), 0x1p-140f, -1.0f, -INFINITY, 1.0f, 3e38f};
        const float s = a.tri >= 0 ? a.s : (box ? 0.5f * (entry + exit_) : 1.0f);
        tm.push_back(s);
        tm.push_back(nextafterf(s, INFINITY));
        tm.push_back(nextafterf(s, -INFINITY));
        for (int k = 0; k < 4; ++k) tm.push_back(s * exp2f(U(rng)));
        if (box) { // below the scene box's entry, at it, and at the root's exit
            tm.push_back(entry);
            tm.push_back(nextafterf(entry, -INFINITY));
            tm.push_back(0.5f * entry);
            tm.push_back(exit_);
            tm.push_back(nextafterf(exit_, INFINITY));
        }
        for (const float tmax : tm) {
            const bool want = a.tri >= 0 && a.s < tmax;
            want_occ += want;
            for (int kd_only = 0; kd_only < 2; ++kd_only) {
                ++cases;
                const bool got = occluded(h, o, d, tmax, kd_only != 0);
                if (got != want) {
                    if (bad < 5)
                        printf("mismatch ray %lld (%a %a %a %a %a %a) tmax %a kd_only %d: definition %d (tri %d s %a), "
                               "restatement %d\n", i, o.x, o.y, o.z, d.x, d.y, d.z, tmax, kd_only, (int)want, a.tri, a.s,
                               (int)got);
                    ++bad;
                }
            }
        }
    }
    printf("rays %lld hits %lld cases %lld occluded %lld mismatches %lld; early %lld kd-phase %lld plain %lld untraced %lld; "
           "T* leaves %lld, ties %lld\n", nr, hits, cases, want_occ, bad, g_early, g_kd_phase, g_plain, g_untraced, g_fast.n,
           g_ties);
    return bad == 0 ? 0 : 1;
}
