// occlusion_check.cpp — host restatement of the occlusion query (rt_occluded:
// csrc/query.hip rt_occluded_kernel, csrc/bvh_trace.h occluded_bvh /
// kd_bounded_s / trace_s) checked against its definition on a real scene:
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

#include "host/bvh_build.h"
#include "host/rt_host.h"

namespace {

float bitsf(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}

struct E { uint32_t node; float entry; };

struct Hit {
    int tri = -1;
    float s = 0.0f;
};

bool scene_box(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float &t1, float &t2)
{
    const Bounding_Box &b = h.bounds;
    float tminx = (b.min.x - o.x) / d.x, tminy = (b.min.y - o.y) / d.y, tminz = (b.min.z - o.z) / d.z;
    float tmaxx = (b.max.x - o.x) / d.x, tmaxy = (b.max.y - o.y) / d.y, tmaxz = (b.max.z - o.z) / d.z;
    t1 = fmaxf(fmaxf(fminf(tminx, tmaxx), fminf(tminy, tmaxy)), fminf(tminz, tmaxz));
    t2 = fminf(fminf(fmaxf(tminx, tmaxx), fmaxf(tminy, tmaxy)), fmaxf(tminz, tmaxz));
    return t1 <= t2;
}

bool test(const RtF4 *A, const RtIsectBary *R, uint32_t e, Vec3D o, Vec3D d, float closest, float &s)
{
    float b[3];
    if (!rt_tri_plane(A[e], o, d, closest, s)) return false;
    return rt_tri_bary(R[e].b, R[e].c, R[e].d, bitsf(R[e].rd), o, d, s, b[0], b[1], b[2]);
}

// ---- the definition: trace_ray, the winning test's s kept ----
Hit plain_trace(const rt_host::PreparedHost &h, Vec3D o, Vec3D d)
{
    Hit hit;
    float entry, exit_;
    if (!scene_box(h, o, d, entry, exit_)) return hit;
    const float root_exit = exit_;
    E stk[64];
    int sp = 0;
    uint32_t node = 0;
    while (true) {
        uint32_t nx = h.nodes[2 * node], ny = h.nodes[2 * node + 1];
        while ((ny & 3u) != RT_LEAF_TAG) {
            const uint32_t axis = ny & 3u;
            const float split = bitsf(nx);
            const float oax = axis == 0 ? o.x : (axis == 1 ? o.y : o.z);
            const float dax = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
            uint32_t near_c = node + 1, far_c = ny >> 2;
            if (oax >= split) {
                near_c = ny >> 2;
                far_c = node + 1;
            }
            const float t = (split - oax) / dax;
            if (t >= exit_ || t < 0) {
                node = near_c;
            } else if (t <= entry) {
                node = far_c;
            } else {
                stk[sp++] = E{far_c, t};
                node = near_c;
                exit_ = t;
            }
            nx = h.nodes[2 * node];
            ny = h.nodes[2 * node + 1];
        }
        const uint32_t count = ny >> 2;
        float smallest = exit_;
        for (uint32_t e = nx; e < nx + count; ++e) {
            float s;
            if (test(h.isect_a.data(), h.isect_bary.data(), e, o, d, smallest, s)) {
                smallest = s;
                hit.tri = (int)h.isect_bary[e].tri;
                hit.s = s;
            }
        }
        if (hit.tri >= 0) return hit;
        if (sp == 0) return hit;
        --sp;
        node = stk[sp].node;
        entry = stk[sp].entry;
        exit_ = sp > 0 ? stk[sp - 1].entry : root_exit;
    }
}

// ---- the restatement: the device's path ----
long long g_fast = 0, g_ties = 0, g_early = 0, g_kd_phase = 0, g_plain = 0, g_untraced = 0;

// bvh_trace.h kd_bounded_s (s_min = -inf, tstar = -1: trace_s)
Hit kd_bounded_s(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float entry, const float root_exit, float s_min,
                 int tstar)
{
    Hit hit;
    float exit_ = root_exit;
    const float yx = rt_recip_guard(d.x), yy = rt_recip_guard(d.y), yz = rt_recip_guard(d.z);
    E stk[64];
    int sp = 0;
    uint32_t node = 0;
    while (true) {
        uint32_t nx = h.nodes[2 * node], ny = h.nodes[2 * node + 1];
        while ((ny & 3u) != RT_LEAF_TAG) {
            const uint32_t axis = ny & 3u;
            const float split = bitsf(nx);
            const float oax = axis == 0 ? o.x : (axis == 1 ? o.y : o.z);
            const float dax = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
            const float yax = axis == 0 ? yx : (axis == 1 ? yy : yz);
            uint32_t near_c = node + 1, far_c = ny >> 2;
            if (oax >= split) {
                near_c = ny >> 2;
                far_c = node + 1;
            }
            const float t = rt_div_by(split - oax, dax, yax);
            if (t >= exit_ || t < 0) {
                node = near_c;
            } else if (t <= entry) {
                node = far_c;
            } else if (t <= s_min) {
                node = far_c;
                entry = t;
            } else {
                stk[sp++] = E{far_c, t};
                node = near_c;
                exit_ = t;
            }
            nx = h.nodes[2 * node];
            ny = h.nodes[2 * node + 1];
        }
        const uint32_t count = ny >> 2;
        if (count > 0 && exit_ > s_min) {
            float smallest = exit_;
            int be = -1;
            const uint32_t e0 = nx, e1 = nx + count;
            if (tstar >= 0) {
                uint32_t at = e1;
                for (uint32_t e = e0; e < e1 && at == e1; ++e)
                    if (h.isect_tri[e] == (uint32_t)tstar) at = e;
                if (at != e1) {
                    float st;
                    if (test(h.isect_a.data(), h.isect_bary.data(), at, o, d, smallest, st)) {
                        smallest = st;
                        be = (int)at;
                        ++g_fast;
                    }
                }
            }
            if (be < 0) {
                for (uint32_t e = e0; e < e1; ++e) {
                    float s;
                    if (test(h.isect_a.data(), h.isect_bary.data(), e, o, d, smallest, s)) {
                        smallest = s;
                        be = (int)e;
                    }
                }
            }
            if (be >= 0) {
                hit.tri = (int)h.isect_bary[be].tri;
                hit.s = smallest;
                return hit;
            }
        }
        if (sp == 0) return hit;
        --sp;
        node = stk[sp].node;
        entry = stk[sp].entry;
        exit_ = sp > 0 ? stk[sp - 1].entry : root_exit;
    }
}

// bvh_trace.h bvh4_bound (bvh4_query + leaf_scan_min): nearest-first, the other hit children pushed
// farthest-first; tstar = the triangle whose test alone set the smallest s, else -1
float bvh4_bound(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float best, int &tstar, bool &tie)
{
    int tk = -1;
    const RtSlab sl = rt_slab(o, d, rt_ray_margin(o.x, o.y, o.z, h.bvh_scale));
    struct B { uint32_t ref; float tn; };
    std::vector<B> stk;
    uint32_t cur = 0;
    auto pop = [&]() -> uint32_t {
        while (!stk.empty()) {
            const B e = stk.back();
            stk.pop_back();
            if (e.tn <= best) return e.ref;
        }
        return RT_BVH_EMPTY;
    };
    while (true) {
        while (!(cur & RT_BVH_LEAF)) {
            const float *f = reinterpret_cast<const float *>(&h.bvh4[8 * (size_t)cur]);
            const uint32_t *rf = reinterpret_cast<const uint32_t *>(f + 24);
            float t[4];
            uint32_t r[4];
            for (int k = 0; k < 4; ++k) {
                r[k] = rf[k];
                if (!rt_bvh_box(f[k], f[4 + k], f[8 + k], f[12 + k], f[16 + k], f[20 + k], sl, best, t[k])) t[k] = INFINITY;
            }
            auto cswap = [&](int a, int b) { // bvh4_children's comparator
                if (t[b] < t[a]) {
                    std::swap(t[a], t[b]);
                    std::swap(r[a], r[b]);
                }
            };
            cswap(0, 1);
            cswap(2, 3);
            cswap(0, 2);
            cswap(1, 3);
            cswap(1, 2);
            for (int k = 3; k >= 1; --k)
                if (t[k] != INFINITY) stk.push_back(B{r[k], t[k]});
            cur = t[0] != INFINITY ? r[0] : pop();
        }
        if (cur == RT_BVH_EMPTY) break;
        const uint32_t first = (cur & ~RT_BVH_LEAF) >> 3, end = first + (cur & 7u) + 1u;
        for (uint32_t e = first; e < end; ++e) {
            float s, b[3];
            if (!rt_tri_plane(h.bvh_a[e], o, d, INFINITY, s) || !(s <= best)) continue;
            const bool lt = s < best;
            if (!lt && tk < 0) continue;
            const RtIsectBary &R = h.bvh_bary[e];
            if (!rt_tri_bary(R.b, R.c, R.d, bitsf(R.rd), o, d, s, b[0], b[1], b[2])) continue;
            if (lt) {
                best = s;
                tk = (int)e;
            } else {
                tk = -2;
            }
        }
        cur = pop();
        if (cur == RT_BVH_EMPTY) break;
    }
    tie = tk == -2;
    tstar = tk >= 0 ? (int)h.bvh_bary[tk].tri : -1;
    return best;
}

// query.hip direction_in_domain
bool direction_in_domain(Vec3D d)
{
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    return (ax <= 2.0f && ay <= 2.0f && az <= 2.0f) && (ax >= 0.5f || ay >= 0.5f || az >= 0.5f);
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
        int tstar = -1;
        bool tie = false;
        const float s_min = bvh4_bound(h, o, d, best0, tstar, tie);
        if (!(s_min < best0)) {
            ++g_early;
            return false;
        }
        if (tie) ++g_ties;
        ++g_kd_phase;
        const Hit r = kd_bounded_s(h, o, d, entry, root_exit, s_min, tstar);
        return r.tri >= 0 && r.s < tmax;
    }
    ++g_plain;
    if (!scene_box(h, o, d, entry, exit_)) return false; // trace_s
    const Hit r = kd_bounded_s(h, o, d, entry, exit_, -INFINITY, -1);
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
    if (rt_host::load_scene_file(scene, argv[1], &cam) != RT_OK) {
        fprintf(stderr, "scene load failed\n");
        return 2;
    }
    const int n = (int)scene.tris.size();
    std::vector<KD_Tree_Node> nodes;
    std::vector<int> indices;
    Bounding_Box bounds;
    if (rt_host::build_kd_tree(scene.tris.data(), n, nodes, indices, bounds) != RT_OK) return 2;
    std::vector<int> lights = rt_host::light_list(scene.tris.data(), n);
    rt_host::PreparedHost h;
    if (rt_host::prepare_host(scene.tris.data(), n, nodes.data(), (int)nodes.size(), indices.data(),
                              (int)indices.size(), lights.data(), (int)lights.size(), bounds, h) != RT_OK) {
        fprintf(stderr, "prepare failed\n");
        return 2;
    }
    if (h.bvh_depth < 0 || h.bvh4.empty()) {
        fprintf(stderr, "no BVH built\n");
        return 2;
    }
    std::vector<float> v;
    {
        FILE *f = fopen(argv[3], "rb");
        if (!f) return 2;
        float buf[6];
        while (fread(buf, sizeof buf, 1, f) == 1) v.insert(v.end(), buf, buf + 6);
        fclose(f);
    }
    const long long nr = (long long)(v.size() / 6);
    if (strcmp(argv[2], "dump") == 0) {
        FILE *f = fopen(argv[4], "wb");
        if (!f) return 2;
        long long hits = 0;
        for (long long i = 0; i < nr; ++i) {
            const Vec3D o = rt_v3(v[6 * i], v[6 * i + 1], v[6 * i + 2]), d = rt_v3(v[6 * i + 3], v[6 * i + 4], v[6 * i + 5]);
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
        const Vec3D o = rt_v3(v[6 * i], v[6 * i + 1], v[6 * i + 2]), d = rt_v3(v[6 * i + 3], v[6 * i + 4], v[6 * i + 5]);
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
           "T* leaves %lld, ties %lld\n", nr, hits, cases, want_occ, bad, g_early, g_kd_phase, g_plain, g_untraced, g_fast,
           g_ties);
    return bad == 0 ? 0 : 1;
}
