// deep_ray_work.cpp — work per ray of a deep (total internal reflection)
// path's bounce on the host: rays from random points of the transparent
// triangles into the glass, at TIR-like angles.  Counts, per ray, the plain
// KD traversal's nodes / leaves / tests, the bounded traversal's BVH nodes /
// leaf visits and KD nodes, and the s_min query over an 8-wide collapse of the
// same BVH (node visits, visits that test leaves) — the dependent-load chains
// a lone ray pays.  Also the model of wf_long's level-synchronous s_min query
// (csrc/wide_bvh.h wide_smin, restated in csrc/host/wide_smin_host.h) over
// the wide collapse at a given arity: per ray its dependent rounds (the leaves
// a round lists are tested in the next one), wide nodes expanded, slots
// tested, the largest frontier, and the KD nodes the bounded traversal still
// visits below the start node of the grid cell holding P = o + d * s_min.
// Both for TIR-like chords (cos to the inward axis 0.2-0.7) and grazing ones
// (0.02-0.2).  Experiment tooling, not product code.
//
// usage: deep_ray_work scene.txt [rays] [seed] [arity,arity,...]
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "host/wide_smin_host.h"

using namespace trace_host;

namespace {

struct W {
    double kd_nodes = 0, kd_leaves = 0, kd_tests = 0, b_nodes = 0, b_leaves = 0, bk_nodes = 0, bk_leaves = 0,
           w_nodes = 0, w_leafvis = 0, w_tests = 0, n = 0;
};

// a KD descent's nodes / scanned leaves / tests; with `mark` a node, below() = the nodes visited from
// the first visit of `mark` on (-1: never visited)
struct KdCount : NoObserver {
    double nodes = 0, leaves = 0, tests = 0, at = -1;
    uint32_t mark = 0xFFFFFFFFu;
    void kd_node(uint32_t n)
    {
        if (at < 0 && n == mark) at = nodes;
        ++nodes;
    }
    void kd_leaf(uint32_t, uint32_t, float, float, int, bool scanned) { leaves += scanned; }
    void kd_test() { ++tests; }
    double below() const { return at < 0 ? -1 : nodes - at; }
};
struct BvhCount : NoObserver {
    double nodes = 0, leaves = 0, tests = 0;
    void bvh_node() { ++nodes; }
    void bvh_leaf() { ++leaves; }
    void bvh_test() { ++tests; }
};

// KD traversal (rt/trace_ray.cuh:244-318) with the skip bound s_min (-inf: plain)
int kd(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float entry, float exit_, float s_min, KdCount &c)
{
    return kd_descent<IEEE_DIV, HARD_FAILURE>(h, o, d, entry, exit_, s_min, -1, c).tri;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const long long rays = argc > 2 ? atoll(argv[2]) : 20000;
    std::mt19937_64 rng(argc > 3 ? strtoull(argv[3], nullptr, 10) : 5);
    RtHostScene scene;
    Camera cam;
    rt_host::PreparedHost h;
    if (!load_prepared(argv[1], scene, cam, h) || h.bvh_depth < 0) return 2;
    const int n = (int)scene.tris.size();
    const Bvh8 w8 = build_bvh8(h);
    // glass triangles and their spheres' centres (split at the middle of their x range)
    std::vector<int> glass;
    double xmin = 1e30, xmax = -1e30;
    for (int i = 0; i < n; ++i)
        if (scene.tris[i].material.transparent) {
            glass.push_back(i);
            xmin = std::min(xmin, (double)scene.tris[i].p1.x);
            xmax = std::max(xmax, (double)scene.tris[i].p1.x);
        }
    if (glass.empty()) return 2;
    const double xmid = 0.5 * (xmin + xmax);
    double c[2][3] = {}, cn[2] = {};
    for (int i : glass) {
        const Triangle &t = scene.tris[i];
        const int k = t.p1.x < xmid ? 0 : 1;
        c[k][0] += t.p1.x; c[k][1] += t.p1.y; c[k][2] += t.p1.z;
        cn[k] += 1;
    }
    for (int k = 0; k < 2; ++k)
        for (int a = 0; a < 3; ++a) c[k][a] /= cn[k] > 0 ? cn[k] : 1;
    std::vector<int> arities{4, 8, 16, 64};
    if (argc > 4) {
        arities.clear();
        for (char *t = strtok(argv[4], ","); t; t = strtok(nullptr, ",")) arities.push_back(atoi(t));
    }
    std::vector<std::vector<RtF4>> wides(arities.size());
    for (size_t k = 0; k < arities.size(); ++k) rt_host::collapse_bvh_wide(h.bvh_nodes, arities[k], wides[k]);
    struct Model { double rounds = 0, nodes = 0, tests = 0, n = 0, differ = 0; int rmax = 0, frontier = 0; };
    std::vector<Model> mdl[2];
    mdl[0].resize(arities.size());
    mdl[1].resize(arities.size());
    double kd_below[2] = {0, 0}, kd_full[2] = {0, 0}, kd_on_path[2] = {0, 0}, kd_rays[2] = {0, 0};
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    auto u = [&]() { return U(rng); };
    W w;
    long long mism = 0;
    const float ranges[2][2] = {{0.2f, 0.7f}, {0.02f, 0.2f}};
    for (int rg = 0; rg < 2; ++rg)
    for (long long r = 0; r < rays; ++r) {
        const Triangle &t = scene.tris[glass[(size_t)(U(rng) * glass.size()) % glass.size()]];
        const Vec3D o = point_on(t, u);
        const int k = o.x < xmid ? 0 : 1;
        const Vec3D a = rt_normalize(rt_v3((float)c[k][0] - o.x, (float)c[k][1] - o.y, (float)c[k][2] - o.z));
        Vec3D d;
        while (true) { // inward at a TIR-like (or grazing) angle: cos to the inward axis in the range
            Vec3D v = rt_v3(2 * U(rng) - 1, 2 * U(rng) - 1, 2 * U(rng) - 1);
            const float l = rt_dot(v, v);
            if (l < 1e-6f || l > 1.0f) continue;
            v = rt_normalize(v);
            if (rg == 1) v = rt_normalize(v - rt_dot(v, a) * a + (ranges[1][0] + (ranges[1][1] - ranges[1][0]) * U(rng)) * a);
            const float ca = rt_dot(v, a);
            if (ca > ranges[rg][0] && ca < ranges[rg][1]) { d = v; break; }
        }
        float t1, t2;
        if (!scene_box(h, o, d, t1, t2)) continue;
        BvhCount b2;
        const float s2 = bvh_bound(h, o, d, t2, b2);
        if (rg == 0) {
            w.b_nodes += b2.nodes;
            w.b_leaves += b2.leaves;
        }
        // the model: the level-synchronous query at every arity, against the depth-first one
        for (size_t q = 0; q < arities.size(); ++q) {
            WsmWork ww;
            float sm;
            int tk;
            if (!wide_smin_host(wides[q], arities[q], h, o, d, t2, 1u << 20, 1u << 20, false, sm, tk, ww)) continue;
            Model &m = mdl[rg][q];
            m.n += 1;
            m.rounds += ww.rounds;
            m.nodes += (double)ww.nodes;
            m.tests += (double)ww.tests;
            m.rmax = ww.rounds > m.rmax ? ww.rounds : m.rmax;
            m.frontier = ww.frontier > m.frontier ? ww.frontier : m.frontier;
            if (memcmp(&sm, &s2, 4) != 0) m.differ += 1;
        }
        // the bounded KD phase, and its part below the start node of P's grid cell
        size_t cell;
        if (s2 < t2 && cell_of(h, rt_v3(o.x + d.x * s2, o.y + d.y * s2, o.z + d.z * s2), cell)) {
            KdCount kc;
            kc.mark = h.kd_cell[2 * cell];
            (void)kd(h, o, d, t1, t2, s2, kc);
            const double nn = kc.nodes, below = kc.below();
            kd_rays[rg] += 1;
            kd_full[rg] += nn;
            if (below >= 0) {
                kd_on_path[rg] += 1;
                kd_below[rg] += below;
            }
        }
        if (rg == 1) continue; // (the tool's earlier figures: the first range only)
        w.n += 1;
        KdCount kp, kb;
        BvhCount b8;
        const int plain = kd(h, o, d, t1, t2, -INFINITY, kp);
        const float s8 = bvh8(h, w8, o, d, t2, b8);
        if (s8 != s2) ++mism;
        const int bounded = s2 < t2 ? kd(h, o, d, t1, t2, s2, kb) : -1;
        if (bounded != plain) ++mism;
        w.kd_nodes += kp.nodes;
        w.kd_leaves += kp.leaves;
        w.kd_tests += kp.tests;
        w.w_nodes += b8.nodes;
        w.w_leafvis += b8.leaves;
        w.w_tests += b8.tests;
        w.bk_nodes += kb.nodes;
        w.bk_leaves += kb.leaves;
    }
    const double R = w.n > 0 ? w.n : 1;
    printf("rays %.0f mismatches %lld (8-wide nodes %zu)\n", w.n, mism, w8.N.size());
    printf("plain KD per ray: nodes %.1f leaves %.1f tests %.1f\n", w.kd_nodes / R, w.kd_leaves / R, w.kd_tests / R);
    printf("bounded per ray: BVH nodes %.1f leaf visits %.1f; KD nodes %.1f leaves %.2f\n", w.b_nodes / R,
           w.b_leaves / R, w.bk_nodes / R, w.bk_leaves / R);
    printf("8-wide BVH per ray: node visits %.1f visits with leaf tests %.1f tests %.1f\n", w.w_nodes / R,
           w.w_leafvis / R, w.w_tests / R);
    for (int rg = 0; rg < 2; ++rg) {
        printf("level-synchronous s_min query, cos to the inward axis %.2f-%.2f:\n", ranges[rg][0], ranges[rg][1]);
        for (size_t q = 0; q < arities.size(); ++q) {
            const Model &m = mdl[rg][q];
            const double n = m.n > 0 ? m.n : 1;
            printf("  arity %2d: rounds %.2f (max %d) wide nodes %.1f tests %.1f largest frontier %d; s_min differing "
                   "from the depth-first query %.0f of %.0f\n", arities[q], m.rounds / n, m.rmax, m.nodes / n,
                   m.tests / n, m.frontier, m.differ, m.n);
        }
        printf("  bounded KD phase: %.1f nodes per ray from the root; P's cell start node on the path for %.0f of %.0f "
               "rays, %.1f nodes left below it\n", kd_full[rg] / (kd_rays[rg] > 0 ? kd_rays[rg] : 1), kd_on_path[rg],
               kd_rays[rg], kd_below[rg] / (kd_on_path[rg] > 0 ? kd_on_path[rg] : 1));
    }
    return 0;
}
