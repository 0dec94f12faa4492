// bvh_trace_check.cpp — host restatement of the BVH-bounded trace_ray
// (csrc/bvh_trace.h) checked against the plain KD traversal (trace_ray,
// rt/trace_ray.cuh:244-318, as csrc/rt_kernels.h trace()) on a real scene:
// camera rays and bounce-like rays (from random points on the triangles, in
// random directions, some grazing), every result compared bit for bit
// (triangle, barycentrics).  Also reports the work per ray of both
// traversals (nodes, triangle tests) — the reason for the bounded one.
//
// Both traversals are csrc/host/trace_host.h's: the bounded one with IEEE
// divisions, a T* entry that does not pass ending the program (exit 3).
//
// Links the library's host code (rt_host::*): the scene loader, the KD
// build and prepare_host, i.e. the very arrays the GPU gets.
//
// Usage: bvh_trace_check scene.txt [rays] [seed] ["x y z" camera position,
// hex floats]; exit 0 = all identical.
#include <math.h>
#include <omp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "host/trace_host.h"

using namespace trace_host;

namespace {

bool g_debug = false;
long long g_fast = 0, g_ties = 0; // T* leaves taken / rays whose s_min two tests share

struct Work : NoObserver {
    long long nodes = 0, tests = 0, bvh_nodes = 0, bvh_tests = 0, leaves = 0, rows = 0;
    void kd_node(uint32_t) { ++nodes; }
    void kd_leaf(uint32_t node, uint32_t count, float entry, float exit_, int sp, bool scanned)
    {
        if (g_debug) printf("  leaf node %u count %u entry %a exit %a sp %d\n", node, count, entry, exit_, sp);
        leaves += scanned;
    }
    void kd_test() { ++tests; }
    void tstar_leaf()
    {
#pragma omp atomic
        ++g_fast;
    }
    void kd_row() { ++rows; }
    void bvh_node() { ++bvh_nodes; }
    void bvh_test() { ++bvh_tests; }
};

long long g_origin_mism = 0;
long long g_bvh4_mism = 0;

// the product's s_min query on the 4-wide collapse (bvh_trace.h bvh4_bound); tstar: the triangle whose
// test alone set the smallest s, else -1
float smin_query(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float best, Work &w, int &tstar)
{
    const Smin q = bvh4_smin(h, o, d, best, w);
    if (q.tk == TK_TIE) {
#pragma omp atomic
        ++g_ties;
    }
    tstar = tstar_of(h, q.tk);
    return q.best;
}

// the bounded descent (bvh_trace.h's step 3): IEEE divisions, and a T* entry that does not pass ends the program
Hit bounded_trace(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, Work &w)
{
    float t1, t2;
    if (!scene_box(h, o, d, t1, t2)) return Hit{};
    if (!rt_bounded_ray(o, d, h.split_vals.data(), h.split_off)) return kd_plain(h, o, d, t1, t2, w);
    Work w2;
    const float s_bin = bvh_bound(h, o, d, t2, w2);
    int tstar = -1;
    const float s_min = smin_query(h, o, d, t2, w, tstar); // the product's query
    if (memcmp(&s_bin, &s_min, 4) != 0) {
#pragma omp atomic
        ++g_bvh4_mism;
    }
    if (!(s_min < t2)) return Hit{};
    return kd_descent<IEEE_DIV, HARD_FAILURE>(h, o, d, t1, t2, s_min, tstar, w);
}

// the plain traversal entered at the KD node of the grid cell holding the
// origin (wavefront.hip wf_long, coop_trace.h kd_origin_frontier): the
// replay with s_min = -inf, then the rest from that state
long long g_origin_resumed = 0;
Hit origin_trace(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, Work &w)
{
    float t1, t2;
    if (!scene_box(h, o, d, t1, t2)) return Hit{};
    size_t k;
    Resume r;
    if (cell_of(h, o, k) && kd_resume(h, h.kd_cell[2 * k], h.kd_cell[2 * k + 1], o, d, t1, t2, -INFINITY, r, w)) {
#pragma omp atomic
        ++g_origin_resumed;
        return kd_plain(h, o, d, t1, t2, w, &r);
    }
    return kd_plain(h, o, d, t1, t2, w);
}

// the plain KD traversal: trace_ray itself, the right answer
Hit plain_trace(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, Work &w)
{
    float t1, t2;
    if (!scene_box(h, o, d, t1, t2)) return Hit{};
    return kd_plain(h, o, d, t1, t2, w);
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: %s scene.txt [rays] [seed]\n", argv[0]);
        return 2;
    }
    const long long rays = argc > 2 ? atoll(argv[2]) : 200000;
    std::mt19937_64 rng(argc > 3 ? strtoull(argv[3], nullptr, 10) : 7);
    RtHostScene scene;
    Camera cam;
    rt_host::PreparedHost h;
    if (!load_prepared(argv[1], scene, cam, h)) return 2;
    const int n = (int)scene.tris.size();
    if (argc > 3 && strcmp(argv[2], "file") == 0) { // a ray file: float32 (n, 6) o, d (tools/dump_rays.py)
        std::vector<float> v;
        if (!read_rays_f32(argv[3], v)) return 2;
        const long long nr = (long long)(v.size() / 6);
        long long bad = 0;
        Work wb, wp;
        for (long long i = 0; i < nr; ++i) {
            const Vec3D o = ray_o(v, (size_t)i), d = ray_d(v, (size_t)i);
            const Hit a = plain_trace(h, o, d, wp), b = bounded_trace(h, o, d, wb);
            if (!same_hit(a, b)) {
                if (bad < 5)
                    printf("mismatch ray %a %a %a %a %a %a: kd %d bounded %d\n", o.x, o.y, o.z, d.x, d.y, d.z, a.tri,
                           b.tri);
                ++bad;
            }
        }
        printf("rays %lld mismatches %lld; T* leaves %lld, ties %lld\n", nr, bad, g_fast, g_ties);
        return bad == 0 ? 0 : 1;
    }
    if (argc > 3 && strcmp(argv[2], "ray") == 0) { // debug one ray: "ox oy oz dx dy dz" (hex floats)
        Vec3D o, d;
        if (sscanf(argv[3], "%a %a %a %a %a %a", &o.x, &o.y, &o.z, &d.x, &d.y, &d.z) != 6) return 2;
        Work w;
        float t1, t2;
        const bool in = scene_box(h, o, d, t1, t2);
        const float s_min = in ? bvh_bound(h, o, d, t2, w) : NAN;
        g_debug = true;
        printf("plain:\n");
        const Hit a = plain_trace(h, o, d, w);
        printf("bounded:\n");
        const Hit b = bounded_trace(h, o, d, w);
        g_debug = false;
        printf("box %d [%a, %a] s_min %a kd %d bounded %d\n", in, t1, t2, s_min, a.tri, b.tri);
        if (in) {
            int ts = -1;
            const float s4 = smin_query(h, o, d, t2, w, ts);
            printf("4-wide query: s_min %a, T* %d\n", s4, ts);
        }
        for (int e = 0; e < (int)h.isect_a.size(); ++e) { // every passing test (KD entry order)
            float s, bb[3];
            if (tri_test(h.isect_a.data(), h.isect_bary.data(), (uint32_t)e, o, d, INFINITY, s, bb))
                printf("  pass: entry %d tri %u s %a\n", e, h.isect_bary[e].tri, s);
        }
        for (size_t k = 0; k < h.bvh_a.size(); ++k) {
            float s, bb[3];
            if (tri_test(h.bvh_a.data(), h.bvh_bary.data(), (uint32_t)k, o, d, INFINITY, s, bb))
                printf("  bvh pass: slot %zu tri %u s %a\n", k, h.bvh_bary[k].tri, s);
        }
        return 0;
    }
    if (argc > 4 && sscanf(argv[4], "%a %a %a", &cam.position.x, &cam.position.y, &cam.position.z) != 3) {
        fprintf(stderr, "bad camera position '%s'\n", argv[4]);
        return 2;
    }
    if (h.bvh_depth < 0) {
        fprintf(stderr, "no BVH built\n");
        return 2;
    }
    printf("tris %d kd_nodes %zu bvh_nodes %zu bvh_depth %d always %d dropped %d\n", n, h.nodes.size() / 2,
           h.bvh_nodes.size() / 4, h.bvh_depth, h.bvh_always, h.bvh_dropped);
    {
        // every triangle's shipped margin (tri_margin + rt_ray_margin, for origins from the scene's
        // centre to far outside it) against the proven bound (bvh_build.h tri_margin_bound)
        const Bounding_Box &b = h.bounds;
        const double box1 = fmax(fabs((double)b.min.x), fabs((double)b.max.x)) +
                            fmax(fabs((double)b.min.y), fabs((double)b.max.y)) +
                            fmax(fabs((double)b.min.z), fabs((double)b.max.z));
        long long shorts = 0, unproven = 0, finite = 0;
        double min_ratio = INFINITY;
#pragma omp parallel for reduction(+ : shorts, unproven, finite) reduction(min : min_ratio)
        for (long long k = 0; k < (long long)h.bvh_bary.size(); ++k) {
            const RtIsectBary &r = h.bvh_bary[(size_t)k];
            const RtF4 &A = h.bvh_a[(size_t)k];
            const Vec3D p1 = rt_v3(r.b.x, r.b.y, r.b.z), v0 = rt_v3(r.c.x, r.c.y, r.c.z), v1 = rt_v3(r.d.x, r.d.y, r.d.z);
            const float rd = bitsf(r.rd);
            const float m = rt_host::tri_margin(p1, v0, v1, rd, A.x, A.y, A.z);
            if (!(m == m) || isinf(m)) continue; // (whole-scene box / left out)
            ++finite;
            for (double on1 : {0.0, box1, 1e3 * box1, 1e6 * box1 + 1.0}) {
                const double pb = rt_host::tri_margin_bound(p1, v0, v1, rd, on1, box1);
                if (isinf(pb)) {
                    ++unproven;
                    continue;
                }
                const float of = (float)(on1 / 3.0);
                const double shipped = (double)m + (double)rt_ray_margin(of, of, of, h.bvh_scale);
                min_ratio = fmin(min_ratio, shipped / pb);
                if (shipped < pb) ++shorts;
            }
        }
        printf("margins: %lld finite, shipped below the proven bound %lld, unproven %lld, min ratio %.4g\n", finite,
               shorts, unproven, min_ratio);
        if (shorts || unproven) return 1;
    }
    Work wp, wb;
    long long mism = 0, hits = 0;
    const unsigned long long seed = rng(); // (drawn once: the engine is shared)
#pragma omp parallel
    {
        Work lp, lb;
        long long lm = 0, lh = 0;
        std::mt19937_64 r2(seed + 0x9e3779b97f4a7c15ull * (unsigned)omp_get_thread_num());
        std::uniform_real_distribution<float> V(0.0f, 1.0f);
        auto u = [&]() { return V(r2); };
#pragma omp for schedule(dynamic, 1024)
        for (long long k = 0; k < rays; ++k) {
            Vec3D o, d;
            const int mode = (int)(k % 4);
            if (mode == 0) { // from the camera
                o = cam.position;
                d = unit_vector(u);
            } else { // from a point on a random triangle (a bounce), some grazing / axis-parallel
                const Triangle &t = scene.tris[(size_t)(u() * n) % n];
                o = point_on(t, u);
                d = unit_vector(u);
                if (mode == 2) d = grazing(d, t, u);
                else if (mode == 3 && (k & 4)) d = axis_parallel(d, (int)(k >> 3) % 3);
                if (d.x != d.x) continue;
            }
            const Hit a = plain_trace(h, o, d, lp), b = bounded_trace(h, o, d, lb);
            Work lo;
            const Hit oc = origin_trace(h, o, d, lo);
            if (!same_hit(oc, a)) {
#pragma omp atomic
                ++g_origin_mism;
            }
            if (a.tri >= 0) ++lh;
            if (!same_hit(a, b)) {
                if (++lm <= 5) {
#pragma omp critical
                    fprintf(stderr, "MISMATCH o (%a %a %a) d (%a %a %a): kd %d, bounded %d\n", o.x, o.y, o.z, d.x,
                            d.y, d.z, a.tri, b.tri);
                }
            }
        }
#pragma omp critical
        {
            mism += lm;
            hits += lh;
            wp.nodes += lp.nodes;
            wp.tests += lp.tests;
            wp.leaves += lp.leaves;
            wb.nodes += lb.nodes;
            wb.tests += lb.tests;
            wb.leaves += lb.leaves;
            wb.bvh_nodes += lb.bvh_nodes;
            wb.bvh_tests += lb.bvh_tests;
        }
    }
    const double R = (double)rays;
    printf("rays %lld hits %lld mismatches %lld\n", rays, hits, mism);
    printf("kd-only per ray: nodes %.1f leaves %.1f tests %.1f\n", wp.nodes / R, wp.leaves / R, wp.tests / R);
    printf("bounded per ray: bvh nodes %.1f bvh tests %.1f kd nodes %.1f leaves %.2f tests %.1f\n", wb.bvh_nodes / R,
           wb.bvh_tests / R, wb.nodes / R, wb.leaves / R, wb.tests / R);
    printf("origin-cell entry: %lld resumed, mismatches vs the plain traversal %lld\n", g_origin_resumed, g_origin_mism);
    printf("4-wide s_min query: %zu nodes, deepest stack %d, s_min differing from the binary query %lld\n",
           h.bvh4.size() / 8, h.bvh4_stack, g_bvh4_mism);
    printf("T* leaves: %lld tested by T*'s entry alone; rays whose s_min two tests share: %lld\n", g_fast, g_ties);
    return mism == 0 && g_origin_mism == 0 && g_bvh4_mism == 0 ? 0 : 1;
}
