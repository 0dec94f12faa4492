// wide_smin_check.cpp — the wide collapse of the conservative BVH
// (csrc/host/bvh_build.h collapse_bvh_wide) and the level-synchronous s_min
// query wf_long runs on it (csrc/wide_bvh.h wide_smin, restated for the host
// in csrc/host/wide_smin_host.h), checked on the library's own prepared arrays:
//
//  * structure: the wide tree is the binary tree — every leaf reference
//    exactly once, and every child box a bit copy of the box the binary tree
//    stores for the node over the same set of leaves;
//  * the query: (best, tk) equal to the sequential 4-wide query's (bvh_trace.h
//    bvh4_query, restated in csrc/host/trace_host.h bvh4_smin: depth-first, best lowered test by test) bit for bit, with its
//    lists walked forwards and backwards, for camera rays, bounce rays (some
//    grazing, some axis-parallel), chords through the transparent objects at
//    total-internal-reflection angles and grazing chords;
//  * the whole bounce: the wide query + the bounded KD traversal returns the
//    plain KD traversal's hit (triangle, barycentrics), and so does the
//    capacity fallback, forced with lists of one item.
//
// usage: wide_smin_check scene.txt [rays] [seed] ["x y z" camera position, hex floats]
//        wide_smin_check scene.txt edges     rays straight down (-z) onto the midpoint of every triangle edge:
//                                            on a mesh of exactly representable coordinates in a z plane both
//                                            triangles at an edge pass at exactly the same s (the tie cases)
// exit 0 = all identical.
#include <math.h>
#include <omp.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <random>
#include <vector>

#include "host/wide_smin_host.h"

using namespace trace_host;

namespace {

// ---- structure: the wide tree against the binary tree
struct BoxBits {
    uint32_t v[6];
    bool operator==(const BoxBits &o) const { return memcmp(v, o.v, sizeof v) == 0; }
};
struct Sig { // a set of leaf references: count, sum and xor of their hashes
    unsigned long long n = 0, sum = 0, x = 0;
    void add(const Sig &o) { n += o.n; sum += o.sum; x ^= o.x; }
    bool operator<(const Sig &o) const { return n != o.n ? n < o.n : (sum != o.sum ? sum < o.sum : x < o.x); }
};
Sig leaf_sig(uint32_t ref)
{
    unsigned long long z = ref * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
    z ^= z >> 29;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 32;
    return Sig{1, z, z * 0x94D049BB133111EBull};
}

int check_structure(const rt_host::PreparedHost &h, const std::vector<RtF4> &wide, int A)
{
    const size_t nb = h.bvh_nodes.size() / 4, nw = wide.size() / (2 * (size_t)A);
    if (nb == 0 || nw == 0 || wide.size() != nw * 2 * (size_t)A) return 1;
    // the binary tree: per node its leaf set, per (leaf set) the box its parent stores for it
    std::vector<Sig> bs(nb);
    std::map<Sig, BoxBits> by_set;
    std::vector<uint32_t> bin_leaves;
    std::vector<char> done(nb, 0);
    std::vector<uint32_t> st{0};
    auto bchild = [&](uint32_t n, int c, uint32_t &ref, BoxBits &bx) {
        const RtF4 *nd = &h.bvh_nodes[4 * (size_t)n];
        ref = fbits(c == 0 ? nd[3].x : nd[3].y);
        const float f[6] = {c == 0 ? nd[0].x : nd[1].z, c == 0 ? nd[0].y : nd[1].w, c == 0 ? nd[0].z : nd[2].x,
                            c == 0 ? nd[0].w : nd[2].y, c == 0 ? nd[1].x : nd[2].z, c == 0 ? nd[1].y : nd[2].w};
        memcpy(bx.v, f, sizeof f);
    };
    while (!st.empty()) { // post-order
        const uint32_t n = st.back();
        uint32_t r[2];
        BoxBits bx[2];
        bchild(n, 0, r[0], bx[0]);
        bchild(n, 1, r[1], bx[1]);
        bool ready = true;
        for (int c = 0; c < 2; ++c)
            if (r[c] != RT_BVH_EMPTY && !(r[c] & RT_BVH_LEAF) && !done[r[c]]) {
                if (r[c] >= nb) return 2;
                st.push_back(r[c]);
                ready = false;
            }
        if (!ready) continue;
        st.pop_back();
        Sig s;
        for (int c = 0; c < 2; ++c) {
            if (r[c] == RT_BVH_EMPTY) continue;
            const Sig cs = (r[c] & RT_BVH_LEAF) ? leaf_sig(r[c]) : bs[r[c]];
            if (r[c] & RT_BVH_LEAF) bin_leaves.push_back(r[c]);
            auto it = by_set.find(cs);
            if (it != by_set.end() && !(it->second == bx[c])) return 3;
            by_set[cs] = bx[c];
            s.add(cs);
        }
        bs[n] = s;
        done[n] = 1;
    }
    // the wide tree: per node its leaf set (post-order), every child's box against the binary box of its set
    std::vector<Sig> ws(nw);
    std::vector<char> wdone(nw, 0);
    std::vector<uint32_t> wide_leaves;
    st.assign(1, 0u);
    size_t visited = 0;
    while (!st.empty()) {
        const uint32_t n = st.back();
        bool ready = true;
        for (int c = 0; c < A; ++c) {
            const uint32_t ref = fbits(wide[2 * ((size_t)n * A + c) + 1].z);
            if (ref != RT_BVH_EMPTY && !(ref & RT_BVH_LEAF) && !wdone[ref]) {
                if (ref >= nw) return 4;
                st.push_back(ref);
                ready = false;
            }
        }
        if (!ready) continue;
        st.pop_back();
        if (wdone[n]) return 5; // reached twice: not a tree
        ++visited;
        Sig s;
        for (int c = 0; c < A; ++c) {
            const RtF4 *rec = &wide[2 * ((size_t)n * A + c)];
            const uint32_t ref = fbits(rec[1].z);
            if (ref == RT_BVH_EMPTY) continue;
            const Sig cs = (ref & RT_BVH_LEAF) ? leaf_sig(ref) : ws[ref];
            if (ref & RT_BVH_LEAF) wide_leaves.push_back(ref);
            BoxBits bx;
            const float f[6] = {rec[0].x, rec[0].y, rec[0].z, rec[0].w, rec[1].x, rec[1].y};
            memcpy(bx.v, f, sizeof f);
            auto it = by_set.find(cs);
            if (it == by_set.end() || !(it->second == bx)) return 6; // not a bit copy of a binary node's box
            s.add(cs);
        }
        ws[n] = s;
        wdone[n] = 1;
    }
    if (visited != nw) return 7; // unreachable wide nodes
    std::sort(bin_leaves.begin(), bin_leaves.end());
    std::sort(wide_leaves.begin(), wide_leaves.end());
    if (std::adjacent_find(wide_leaves.begin(), wide_leaves.end()) != wide_leaves.end()) return 8;
    if (bin_leaves != wide_leaves) return 9;
    return 0;
}

struct Tally {
    long long rays = 0, bounded = 0, query_mism = 0, order_mism = 0, hit_mism = 0, fallback_mism = 0, overflows = 0,
              forced = 0, ties = 0, cross_ties = 0, hits = 0, rounds = 0, nodes = 0, tests = 0;
    int frontier = 0, leaves = 0;
    void add(const Tally &o)
    {
        rays += o.rays; bounded += o.bounded; query_mism += o.query_mism; order_mism += o.order_mism;
        hit_mism += o.hit_mism; fallback_mism += o.fallback_mism; overflows += o.overflows; forced += o.forced;
        ties += o.ties; cross_ties += o.cross_ties; hits += o.hits; rounds += o.rounds; nodes += o.nodes;
        tests += o.tests;
        frontier = o.frontier > frontier ? o.frontier : frontier;
        leaves = o.leaves > leaves ? o.leaves : leaves;
    }
};

const size_t kFcap = WSM_FCAP, kLcap = WSM_LCAP; // (csrc/wide_bvh_caps.h: the device's)

void check_ray(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, Tally &t)
{
    ++t.rays;
    float t1, t2;
    if (!scene_box(h, o, d, t1, t2)) return;
    // the query itself (also for rays the bound does not apply to: it is a function of the ray alone)
    if (!(o.x - o.x == 0.0f && o.y - o.y == 0.0f && o.z - o.z == 0.0f && d.x - d.x == 0.0f && d.y - d.y == 0.0f &&
          d.z - d.z == 0.0f) || !(fabsf(o.x) + fabsf(o.y) + fabsf(o.z) < 0x1p64f))
        return;
    int tk_a = -1, tk_b = -1;
    const Smin seq = bvh4_smin(h, o, d, t2); // the sequential query (bvh_trace.h bvh4_query)
    const float s_seq = seq.best;
    const int tk_seq = seq.tk;
    float s_a = 0, s_b = 0;
    WsmWork wa, wb;
    const bool ok_a = wide_smin_host(h.bvh_wide, RT_BVHW_ARITY, h, o, d, t2, kFcap, kLcap, false, s_a, tk_a, wa);
    const bool ok_b = wide_smin_host(h.bvh_wide, RT_BVHW_ARITY, h, o, d, t2, kFcap, kLcap, true, s_b, tk_b, wb);
    if (!ok_a || !ok_b) ++t.overflows;
    if (ok_a && (fbits(s_a) != fbits(s_seq) || tk_a != tk_seq)) {
        if (++t.query_mism <= 3)
            fprintf(stderr, "QUERY MISMATCH o (%a %a %a) d (%a %a %a): sequential %a tk %d, wide %a tk %d\n", o.x, o.y,
                    o.z, d.x, d.y, d.z, s_seq, tk_seq, s_a, tk_a);
    }
    if (ok_a != ok_b || (ok_a && (fbits(s_a) != fbits(s_b) || tk_a != tk_b))) ++t.order_mism;
    if (ok_a) {
        t.rounds += wa.rounds;
        t.nodes += wa.nodes;
        t.tests += wa.tests;
        t.frontier = wa.frontier > t.frontier ? wa.frontier : t.frontier;
        t.leaves = wa.leaves > t.leaves ? wa.leaves : t.leaves;
        if (tk_a == TK_TIE) {
            ++t.ties;
            if (wa.cross_round || wb.cross_round) ++t.cross_ties;
        }
    }
    // the whole bounce as wf_long runs it, against the plain KD traversal
    if (!rt_bounded_ray(o, d, h.split_vals.data(), h.split_off)) return;
    ++t.bounded;
    const Hit plain = kd_plain(h, o, d, t1, t2);
    if (plain.tri >= 0) ++t.hits;
    auto bounce = [&](size_t fcap, size_t lcap, bool &fell_back) {
        float s_min;
        int tk;
        WsmWork w;
        fell_back = !wide_smin_host(h.bvh_wide, RT_BVHW_ARITY, h, o, d, t2, fcap, lcap, false, s_min, tk, w);
        if (fell_back) return kd_plain(h, o, d, t1, t2); // (the wide KD traversal: trace_ray's result)
        if (!(s_min < t2)) return Hit{};
        return kd_descent<IEEE_DIV, HARD_FAILURE>(h, o, d, t1, t2, s_min, tstar_of(h, tk));
    };
    bool fb = false;
    const Hit a = bounce(kFcap, kLcap, fb);
    if (!same_hit(a, plain)) {
        if (++t.hit_mism <= 3)
            fprintf(stderr, "HIT MISMATCH o (%a %a %a) d (%a %a %a): kd %d, wide bounded %d\n", o.x, o.y, o.z, d.x, d.y,
                    d.z, plain.tri, a.tri);
    }
    const Hit f = bounce(1, 1, fb); // the forced fallback
    if (fb) ++t.forced;
    if (!same_hit(f, plain)) ++t.fallback_mism;
}

int report(const Tally &t, bool need_forced)
{
    const double R = t.rays > 0 ? (double)t.rays : 1.0;
    printf("rays %lld bounded %lld hits %lld\n", t.rays, t.bounded, t.hits);
    printf("query mismatches %lld order mismatches %lld hit mismatches %lld fallback mismatches %lld\n", t.query_mism,
           t.order_mism, t.hit_mism, t.fallback_mism);
    printf("overflows %lld forced fallbacks %lld ties %lld cross-round ties %lld\n", t.overflows, t.forced, t.ties,
           t.cross_ties);
    printf("per ray: rounds %.2f wide nodes %.2f tests %.1f; largest frontier %d largest leaf list %d\n", t.rounds / R,
           t.nodes / R, t.tests / R, t.frontier, t.leaves);
    const bool ok = t.query_mism == 0 && t.order_mism == 0 && t.hit_mism == 0 && t.fallback_mism == 0 &&
                    (!need_forced || t.forced > 0);
    return ok ? 0 : 1;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: %s scene.txt [rays] [seed] [camera] | scene.txt edges\n", argv[0]);
        return 2;
    }
    RtHostScene scene;
    Camera cam;
    rt_host::PreparedHost h;
    if (!load_prepared(argv[1], scene, cam, h) || h.bvh_depth < 0) {
        fprintf(stderr, "prepare failed / no BVH built\n");
        return 2;
    }
    const int n = (int)scene.tris.size();
    const int sc = check_structure(h, h.bvh_wide, RT_BVHW_ARITY);
    printf("tris %d bvh_nodes %zu wide nodes %zu (arity %d) structure %d\n", n, h.bvh_nodes.size() / 4,
           h.bvh_wide.size() / (2 * RT_BVHW_ARITY), RT_BVHW_ARITY, sc);
    // the other arities the collapse can be built at: the same structural check
    for (int A : {4, 8, 32, 64}) {
        std::vector<RtF4> w;
        rt_host::collapse_bvh_wide(h.bvh_nodes, A, w);
        const int s2 = check_structure(h, w, A);
        if (s2 != 0) {
            printf("arity %d structure %d\n", A, s2);
            return 1;
        }
    }
    if (sc != 0) return 1;

    if (argc > 2 && strcmp(argv[2], "edges") == 0) {
        Tally t;
        for (int i = 0; i < n; ++i) {
            const Triangle &tr = scene.tris[(size_t)i];
            const Vec3D p[3] = {tr.p1, tr.p2, tr.p3};
            for (int e = 0; e < 3; ++e) {
                const Vec3D m = 0.5f * (p[e] + p[(e + 1) % 3]);
                check_ray(h, rt_v3(m.x, m.y, m.z + 1.0f), rt_v3(0.0f, 0.0f, -1.0f), t);
                check_ray(h, rt_v3(m.x, m.y, m.z - 2.0f), rt_v3(0.0f, 0.0f, 1.0f), t);
            }
        }
        return report(t, false);
    }

    const long long rays = argc > 2 ? atoll(argv[2]) : 200000;
    const unsigned long long seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 7;
    if (argc > 4 && sscanf(argv[4], "%a %a %a", &cam.position.x, &cam.position.y, &cam.position.z) != 3) {
        fprintf(stderr, "bad camera position '%s'\n", argv[4]);
        return 2;
    }
    // the transparent objects, for the chords: their triangles in index order (a mesh's are consecutive)
    std::vector<int> glass;
    for (int i = 0; i < n; ++i)
        if (scene.tris[(size_t)i].material.transparent) glass.push_back(i);
    Tally total;
#pragma omp parallel
    {
        Tally t;
        std::mt19937_64 rng(seed + 0x9e3779b97f4a7c15ull * (unsigned)(omp_get_thread_num() + 1));
        std::uniform_real_distribution<float> U(0.0f, 1.0f);
        auto u = [&]() { return U(rng); };
#pragma omp for schedule(dynamic, 1024)
        for (long long k = 0; k < rays; ++k) {
            Vec3D o, d;
            const int mode = (int)(k % 6);
            if (mode == 0) { // from the camera
                o = cam.position;
                d = unit_vector(u);
            } else if (mode >= 4 && !glass.empty()) {
                // a chord of a transparent object: from a point of its surface towards a point of a triangle
                // near it in the mesh's order (mode 4), or nearly along the surface (mode 5: grazing)
                const Triangle &tr = glass_chord(scene, glass, mode == 4 ? (long long)glass.size() : 64, u, o, d);
                if (mode == 5) d = grazing_chord(d, tr, u);
            } else { // a bounce: from a point on a random triangle, some grazing / axis-parallel
                const Triangle &tr = scene.tris[(size_t)(u() * n) % n];
                o = point_on(tr, u);
                d = unit_vector(u);
                if (mode == 2) d = grazing(d, tr, u);
                else if (mode == 3 && (k & 8)) d = axis_parallel(d, (int)(k >> 4) % 3);
            }
            if (d.x != d.x) continue;
            check_ray(h, o, d, t);
        }
#pragma omp critical
        total.add(t);
    }
    return report(total, true);
}
