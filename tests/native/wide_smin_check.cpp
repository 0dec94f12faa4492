// wide_smin_check.cpp — the wide collapse of the conservative BVH
// (csrc/host/bvh_build.h collapse_bvh_wide) and the level-synchronous s_min
// query wf_long runs on it (csrc/wide_bvh.h wide_smin, restated for the host
// in csrc/host/wide_smin_host.h), checked on the library's own prepared arrays:
//
//  * structure: the wide tree is the binary tree — every leaf reference
//    exactly once, and every child box a bit copy of the box the binary tree
//    stores for the node over the same set of leaves;
//  * the query: (best, tk) equal to the sequential 4-wide query's (bvh_trace.h
//    bvh4_query: depth-first, best lowered test by test) bit for bit, with its
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

namespace {

float bitsf(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}
uint32_t fbits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

struct Hit {
    int tri = -1;
    float b[3] = {0, 0, 0};
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

// bvh_trace.h kd_bounded (s_min = -inf: trace_ray itself); tstar >= 0: a leaf listing T* tests its entry alone
Hit kd_trace(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float entry, float exit_, float s_min, int tstar)
{
    Hit hit;
    struct E { uint32_t node; float entry; } stk[64];
    int sp = 0;
    const float root_exit = exit_;
    uint32_t node = 0;
    while (true) {
        uint32_t nx = h.nodes[2 * node], ny = h.nodes[2 * node + 1];
        while ((ny & 3u) != RT_LEAF_TAG) {
            const uint32_t axis = ny & 3u;
            const float split = bitsf(nx);
            const float oax = axis == 0 ? o.x : (axis == 1 ? o.y : o.z);
            const float dax = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
            uint32_t near_c = node + 1, far_c = ny >> 2;
            if (oax >= split) std::swap(near_c, far_c);
            const float t = (split - oax) / dax;
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
            uint32_t lo = nx, hi = nx + count;
            if (tstar >= 0)
                for (uint32_t e = nx; e < nx + count; ++e)
                    if (h.isect_tri[e] == (uint32_t)tstar) {
                        lo = e;
                        hi = e + 1;
                        break;
                    }
            for (uint32_t e = lo; e < hi; ++e) {
                float s, b[3];
                if (rt_tri_plane(h.isect_a[e], o, d, smallest, s) &&
                    rt_tri_bary(h.isect_bary[e].b, h.isect_bary[e].c, h.isect_bary[e].d, bitsf(h.isect_bary[e].rd), o, d,
                                s, b[0], b[1], b[2])) {
                    smallest = s;
                    hit.tri = (int)h.isect_bary[e].tri;
                    memcpy(hit.b, b, sizeof b);
                }
            }
            if (hit.tri >= 0) return hit;
            if (hi - lo != count) {
                fprintf(stderr, "T* entry of a leaf did not pass\n");
                exit(3);
            }
        }
        if (sp == 0) return hit;
        --sp;
        node = stk[sp].node;
        entry = stk[sp].entry;
        exit_ = sp > 0 ? stk[sp - 1].entry : root_exit;
    }
}

// the sequential query (bvh_trace.h bvh4_query on the 4-wide collapse): nearest child first, the
// others pushed farthest-first, best lowered test by test; tk as leaf_scan_min keeps it
float seq_query(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float best, int &tk)
{
    tk = -1;
    const RtSlab sl = rt_slab(o, d, rt_ray_margin(o.x, o.y, o.z, h.bvh_scale));
    struct E { uint32_t ref; float tn; };
    std::vector<E> stk;
    uint32_t cur = 0;
    auto pop = [&]() -> uint32_t {
        while (!stk.empty()) {
            const E e = stk.back();
            stk.pop_back();
            if (e.tn <= best) return e.ref;
        }
        return RT_BVH_EMPTY;
    };
    while (true) {
        while (!(cur & RT_BVH_LEAF)) {
            const float *f = reinterpret_cast<const float *>(&h.bvh4[8 * (size_t)cur]);
            const uint32_t *rf = reinterpret_cast<const uint32_t *>(f + 24);
            E c[4];
            for (int k = 0; k < 4; ++k) {
                float tn;
                const bool hit = rt_bvh_box(f[k], f[4 + k], f[8 + k], f[12 + k], f[16 + k], f[20 + k], sl, best, tn) &&
                                 rf[k] != RT_BVH_EMPTY;
                c[k] = hit ? E{rf[k], tn} : E{RT_BVH_EMPTY, INFINITY};
            }
            std::stable_sort(c, c + 4, [](const E &a, const E &b) {
                const bool ea = a.ref == RT_BVH_EMPTY, eb = b.ref == RT_BVH_EMPTY;
                return ea != eb ? eb : a.tn < b.tn;
            });
            for (int k = 3; k >= 1; --k)
                if (c[k].ref != RT_BVH_EMPTY) stk.push_back(c[k]);
            cur = c[0].ref != RT_BVH_EMPTY ? c[0].ref : pop();
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
                tk = WSM_TK_TIE;
            }
        }
        cur = pop();
        if (cur == RT_BVH_EMPTY) break;
    }
    return best;
}

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
    int tk_seq, tk_a = -1, tk_b = -1;
    const float s_seq = seq_query(h, o, d, t2, tk_seq);
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
        if (tk_a == WSM_TK_TIE) {
            ++t.ties;
            if (wa.cross_round || wb.cross_round) ++t.cross_ties;
        }
    }
    // the whole bounce as wf_long runs it, against the plain KD traversal
    if (!rt_bounded_ray(o, d, h.split_vals.data(), h.split_off)) return;
    ++t.bounded;
    const Hit plain = kd_trace(h, o, d, t1, t2, -INFINITY, -1);
    if (plain.tri >= 0) ++t.hits;
    auto bounce = [&](size_t fcap, size_t lcap, bool &fell_back) {
        float s_min;
        int tk;
        WsmWork w;
        fell_back = !wide_smin_host(h.bvh_wide, RT_BVHW_ARITY, h, o, d, t2, fcap, lcap, false, s_min, tk, w);
        if (fell_back) return kd_trace(h, o, d, t1, t2, -INFINITY, -1); // (the wide KD traversal: trace_ray's result)
        if (!(s_min < t2)) return Hit{};
        return kd_trace(h, o, d, t1, t2, s_min, tk >= 0 ? (int)h.bvh_bary[tk].tri : -1);
    };
    bool fb = false;
    const Hit a = bounce(kFcap, kLcap, fb);
    if (a.tri != plain.tri || memcmp(a.b, plain.b, sizeof a.b) != 0) {
        if (++t.hit_mism <= 3)
            fprintf(stderr, "HIT MISMATCH o (%a %a %a) d (%a %a %a): kd %d, wide bounded %d\n", o.x, o.y, o.z, d.x, d.y,
                    d.z, plain.tri, a.tri);
    }
    const Hit f = bounce(1, 1, fb); // the forced fallback
    if (fb) ++t.forced;
    if (f.tri != plain.tri || memcmp(f.b, plain.b, sizeof f.b) != 0) ++t.fallback_mism;
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
                              (int)indices.size(), lights.data(), (int)lights.size(), bounds, h) != RT_OK ||
        h.bvh_depth < 0) {
        fprintf(stderr, "prepare failed / no BVH built\n");
        return 2;
    }
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
        auto unit = [&]() {
            while (true) {
                Vec3D v = rt_v3(2 * U(rng) - 1, 2 * U(rng) - 1, 2 * U(rng) - 1);
                const float l = rt_dot(v, v);
                if (l > 1e-6f && l <= 1.0f) return rt_normalize(v);
            }
        };
        auto on_tri = [&](const Triangle &tr) {
            float b1 = U(rng), b2 = U(rng);
            if (b1 + b2 > 1) {
                b1 = 1 - b1;
                b2 = 1 - b2;
            }
            return tr.p1 + b1 * (tr.p2 - tr.p1) + b2 * (tr.p3 - tr.p1);
        };
#pragma omp for schedule(dynamic, 1024)
        for (long long k = 0; k < rays; ++k) {
            Vec3D o, d;
            const int mode = (int)(k % 6);
            if (mode == 0) { // from the camera
                o = cam.position;
                d = unit();
            } else if (mode >= 4 && !glass.empty()) {
                // a chord of a transparent object: from a point of its surface towards a point of a triangle
                // near it in the mesh's order (mode 4), or nearly along the surface (mode 5: grazing)
                const size_t gi = (size_t)(U(rng) * glass.size()) % glass.size();
                const Triangle &tr = scene.tris[(size_t)glass[gi]];
                o = on_tri(tr);
                const long long span = mode == 4 ? (long long)glass.size() : 64;
                const long long gj = (long long)gi + (long long)((U(rng) - 0.5f) * span);
                const Triangle &to = scene.tris[(size_t)glass[(size_t)((gj % (long long)glass.size() + glass.size()) % glass.size())]];
                d = rt_normalize(on_tri(to) - o);
                if (mode == 5) {
                    const Vec3D nn = rt_normalize(rt_cross(tr.p2 - tr.p1, tr.p3 - tr.p1));
                    const Vec3D u = unit();
                    if (nn.x == nn.x) d = rt_normalize(u - rt_dot(u, nn) * nn + (0.02f + 0.18f * U(rng)) * (rt_dot(d, nn) < 0 ? -1.0f : 1.0f) * nn);
                }
            } else { // a bounce: from a point on a random triangle, some grazing / axis-parallel
                const Triangle &tr = scene.tris[(size_t)(U(rng) * n) % n];
                o = on_tri(tr);
                d = unit();
                if (mode == 2) {
                    const Vec3D nn = rt_normalize(rt_cross(tr.p2 - tr.p1, tr.p3 - tr.p1));
                    if (nn.x == nn.x) d = rt_normalize(d - rt_dot(d, nn) * nn + 1e-4f * (U(rng) - 0.5f) * nn);
                } else if (mode == 3 && (k & 8)) {
                    const int a = (int)(k >> 4) % 3;
                    if (a == 0) d.x = 0; else if (a == 1) d.y = 0; else d.z = 0;
                    d = rt_normalize(d);
                }
            }
            if (d.x != d.x) continue;
            check_ray(h, o, d, t);
        }
#pragma omp critical
        total.add(t);
    }
    return report(total, true);
}
