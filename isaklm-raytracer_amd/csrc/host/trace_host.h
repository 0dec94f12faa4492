// trace_host.h — the host model of the BVH-bounded traversal, once: the
// device's traversal (csrc/bvh_trace.h, coop_trace.h, query.hip) restated on
// the CPU over the arrays prepare_host produces, for the programs that compare
// it ray by ray with the plain KD traversal (trace_ray):
//
//   kd_descent   bvh_trace.h kd_bounded over rt_kernels.h kd_split_step / kd_pop, statement for statement
//   bvh4_smin    bvh_trace.h bvh4_query + bvh4_children + leaf_scan_min
//   bvh_bound    bvh_trace.h bvh_bound (the binary tree; the 4-wide query's cross-check)
//   Bvh4Walk     bvh4_smin one body at a time; wave_call_budget: bvh_trace.h bvh4_query_budget over a wave's lanes
//                (wave_call_lane_cap: the per-lane cap it replaced)
//   kd_resume    coop_trace.h kd_origin_frontier's replay, cell_of its grid lookup
//   bvh8         an 8-wide work model (experiments only)
//
// and what every such program needs around them: load_prepared, read_rays_f32
// and the ray makers.  A change to kd_bounded or bvh4_query is mirrored HERE,
// in one place.
//
// Not product code: shared by tests/native/{bvh_trace,kd_cert,wide_smin,
// occlusion,trip_budget}_check.cpp and tools/{deep_ray_work,kd_jump_sim,trip_model}.cpp; nothing the
// library is built from includes it.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <utility>
#include <vector>

#include "../bvh_common.h"
#include "bvh_build.h"
#include "rt_host.h"

namespace trace_host {

// ---------------------------------------------------------------- helpers
inline float bitsf(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}
inline uint32_t fbits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// rt_kernels.h scene_box with IEEE divisions (rt_div_by is bit-identical to them)
inline bool scene_box(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float &t1, float &t2)
{
    const Bounding_Box &b = h.bounds;
    float tminx = (b.min.x - o.x) / d.x, tminy = (b.min.y - o.y) / d.y, tminz = (b.min.z - o.z) / d.z;
    float tmaxx = (b.max.x - o.x) / d.x, tmaxy = (b.max.y - o.y) / d.y, tmaxz = (b.max.z - o.z) / d.z;
    t1 = fmaxf(fmaxf(fminf(tminx, tmaxx), fminf(tminy, tmaxy)), fminf(tminz, tmaxz));
    t2 = fminf(fminf(fmaxf(tminx, tmaxx), fmaxf(tminy, tmaxy)), fmaxf(tminz, tmaxz));
    return t1 <= t2;
}

// the leaf test: intersect_triangle on entry e of a (plane, bary) record pair
inline bool tri_test(const RtF4 *A, const RtIsectBary *R, uint32_t e, Vec3D o, Vec3D d, float closest, float &s, float *b)
{
    if (!rt_tri_plane(A[e], o, d, closest, s)) return false;
    return rt_tri_bary(R[e].b, R[e].c, R[e].d, bitsf(R[e].rd), o, d, s, b[0], b[1], b[2]);
}

// query.hip direction_in_domain
inline bool direction_in_domain(Vec3D d)
{
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    return (ax <= 2.0f && ay <= 2.0f && az <= 2.0f) && (ax >= 0.5f || ay >= 0.5f || az >= 0.5f);
}

struct Hit {
    int tri = -1;
    float s = 0.0f; // the winning test's ray parameter
    float b[3] = {0, 0, 0};
};
inline bool same_hit(const Hit &a, const Hit &b) { return a.tri == b.tri && memcmp(a.b, b.b, sizeof a.b) == 0; }

// What a traversal reports while it runs.  A program's counters derive from
// this and redefine the calls they want; the default does nothing and compiles
// away.
struct NoObserver {
    void kd_node(uint32_t /*node*/) {}       // a KD node read
    void kd_leaf(uint32_t /*node*/, uint32_t /*count*/, float /*entry*/, float /*exit*/, int /*sp*/, bool /*scanned*/) {}
    void kd_test() {}                        // a KD leaf entry tested
    void tstar_leaf() {}                     // a leaf answered by T*'s entry alone
    void kd_row() {}                         // a row of the origin-cell replay
    void bvh_node() {}                       // a BVH node expanded
    void bvh_leaf() {}                       // a BVH leaf visit (bvh8: a node visit that tests leaves)
    void bvh_test() {}                       // a BVH leaf slot tested
};

// ---------------------------------------------------------------- the KD descent
struct KdEntry { uint32_t node; float entry; };

// the state the descent resumes from (the origin-cell replay): node, interval, stack
struct Resume {
    uint32_t node = 0;
    float entry = 0, exit_ = 0;
    int sp = 0;
    KdEntry stk[64];
};

enum Division { IEEE_DIV, DEVICE_DIV };       // t = (split - o) / d by `/`, or by rt_recip_guard + rt_div_by
enum TstarMiss { WHOLE_LEAF, HARD_FAILURE };  // a T* entry that does not pass: the device's fall-back, or exit(3)

// bvh_trace.h kd_bounded (its split step and pop: rt_kernels.h kd_split_step,
// kd_pop — Division is their KdDivision): the reference's KD traversal with the
// skip bound s_min (-inf: the plain traversal, trace_ray itself) from the scene
// box's [entry, root_exit]; tstar >= 0: a leaf that lists T* tests T*'s first
// entry alone.  `from`: the start state of the origin-cell replay (kd_resume).
template <Division DIV, TstarMiss MISS, class Obs>
Hit kd_descent(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float entry, const float root_exit, float s_min,
               int tstar, Obs &obs, const Resume *from = nullptr)
{
    Hit hit;
    float exit_ = root_exit;
    const bool dev = DIV == DEVICE_DIV;
    const float yx = dev ? rt_recip_guard(d.x) : 0.0f, yy = dev ? rt_recip_guard(d.y) : 0.0f,
                yz = dev ? rt_recip_guard(d.z) : 0.0f;
    KdEntry stk[64];
    int sp = 0;
    uint32_t node = 0;
    if (from) {
        node = from->node;
        entry = from->entry;
        exit_ = from->exit_;
        sp = from->sp;
        memcpy(stk, from->stk, sizeof(KdEntry) * (size_t)sp);
    }
    while (true) {
        uint32_t nx = h.nodes[2 * node], ny = h.nodes[2 * node + 1];
        obs.kd_node(node);
        while ((ny & 3u) != RT_LEAF_TAG) {
            const uint32_t axis = ny & 3u;
            const float split = bitsf(nx);
            const float oax = axis == 0 ? o.x : (axis == 1 ? o.y : o.z);
            const float dax = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
            const float yax = axis == 0 ? yx : (axis == 1 ? yy : yz);
            uint32_t near_c = node + 1, far_c = ny >> 2;
            if (oax >= split) { // ray_behind_plane
                near_c = ny >> 2;
                far_c = node + 1;
            }
            const float t = dev ? rt_div_by(split - oax, dax, yax) : (split - oax) / dax; // intersect_plane
            if (t >= exit_ || t < 0) {
                node = near_c;
            } else if (t <= entry) {
                node = far_c;
            } else if (t <= s_min) { // the near side holds no hit: its leaves' exits are <= t
                node = far_c;
                entry = t;
            } else {
                stk[sp++] = KdEntry{far_c, t};
                node = near_c;
                exit_ = t;
            }
            nx = h.nodes[2 * node];
            ny = h.nodes[2 * node + 1];
            obs.kd_node(node);
        }
        const uint32_t count = ny >> 2;
        const bool scan = count > 0 && exit_ > s_min;
        obs.kd_leaf(node, count, entry, exit_, sp, scan);
        if (scan) {
            float smallest = exit_; // trace_leaf_node: closest starts at the leaf's exit
            int be = -1;
            const uint32_t e0 = nx, e1 = nx + count;
            if (tstar >= 0) { // the T* leaf: T*'s first listing, its test the leaf's result
                uint32_t at = e1;
                for (uint32_t e = e0; e < e1 && at == e1; ++e)
                    if (h.isect_tri[e] == (uint32_t)tstar) at = e;
                if (at != e1) {
                    float st, b[3];
                    obs.kd_test();
                    if (tri_test(h.isect_a.data(), h.isect_bary.data(), at, o, d, smallest, st, b)) {
                        smallest = st;
                        be = (int)at;
                        memcpy(hit.b, b, sizeof b);
                        obs.tstar_leaf();
                    } else if (MISS == HARD_FAILURE) {
                        fprintf(stderr, "T* entry of a leaf did not pass\n");
                        exit(3);
                    }
                }
            }
            if (be < 0) { // the whole leaf (no T*, or a T* entry that did not pass)
                for (uint32_t e = e0; e < e1; ++e) {
                    float s, b[3];
                    obs.kd_test();
                    if (tri_test(h.isect_a.data(), h.isect_bary.data(), e, o, d, smallest, s, b)) {
                        smallest = s;
                        be = (int)e;
                        memcpy(hit.b, b, sizeof b);
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
template <Division DIV, TstarMiss MISS>
Hit kd_descent(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float entry, float root_exit, float s_min, int tstar)
{
    NoObserver none;
    return kd_descent<DIV, MISS>(h, o, d, entry, root_exit, s_min, tstar, none);
}

// The plain KD traversal (trace_ray) from the scene box's interval: the right-
// hand side of every comparison — IEEE divisions, no bound, no T*.
template <class Obs>
Hit kd_plain(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float entry, float root_exit, Obs &obs,
             const Resume *from = nullptr)
{
    return kd_descent<IEEE_DIV, HARD_FAILURE>(h, o, d, entry, root_exit, -INFINITY, -1, obs, from);
}
inline Hit kd_plain(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float entry, float root_exit)
{
    NoObserver none;
    return kd_plain(h, o, d, entry, root_exit, none);
}

// ---------------------------------------------------------------- the s_min queries
// tk as bvh_trace.h leaf_scan_min leaves it: -1 (no pass), the slot whose test
// alone set best, or TK_TIE (a second slot passes at exactly that s)
constexpr int TK_TIE = -2;
struct Smin {
    float best;
    int tk;
};
// T*: the triangle of slot tk (kd_descent's tstar), -1 where no single slot has s_min
inline int tstar_of(const rt_host::PreparedHost &h, int tk) { return tk >= 0 ? (int)h.bvh_bary[tk].tri : -1; }

// bvh_trace.h bvh4_query over the 4-wide collapse: a node's hit children nearest
// first by bvh4_children's compare-and-swap network (a missed child's entry is
// INFINITY), the nearest descended into, the others pushed farthest-first and
// popped while their entry is <= best; leaves scanned by leaf_scan_min.
// (margin_scale: tools/kd_jump_sim.cpp's experiment; 1 is the device's margin.)
template <class Obs>
Smin bvh4_smin(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float best, Obs &obs, float margin_scale = 1.0f)
{
    int tk = -1;
    const RtSlab sl = rt_slab(o, d, margin_scale * rt_ray_margin(o.x, o.y, o.z, h.bvh_scale));
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
            obs.bvh_node();
            const float *f = reinterpret_cast<const float *>(&h.bvh4[8 * (size_t)cur]);
            const uint32_t *rf = reinterpret_cast<const uint32_t *>(f + 24);
            float t[4];
            uint32_t r[4];
            for (int k = 0; k < 4; ++k) { // (an unused slot's box is culled by its own slab test)
                r[k] = rf[k];
                if (!rt_bvh_box(f[k], f[4 + k], f[8 + k], f[12 + k], f[16 + k], f[20 + k], sl, best, t[k])) t[k] = INFINITY;
            }
            auto cswap = [&](int a, int b) {
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
        obs.bvh_leaf();
        for (uint32_t e = first; e < end; ++e) { // leaf_scan_min
            float s, b[3];
            obs.bvh_test();
            if (!rt_tri_plane(h.bvh_a[e], o, d, INFINITY, s) || !(s <= best)) continue;
            const bool lt = s < best;
            if (!lt && tk < 0) continue; // (at best0, or a tie already)
            const RtIsectBary &R = h.bvh_bary[e];
            if (!rt_tri_bary(R.b, R.c, R.d, bitsf(R.rd), o, d, s, b[0], b[1], b[2])) continue;
            if (lt) {
                best = s;
                tk = (int)e;
            } else {
                tk = TK_TIE;
            }
        }
        cur = pop();
        if (cur == RT_BVH_EMPTY) break;
    }
    return Smin{best, tk};
}
inline Smin bvh4_smin(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float best)
{
    NoObserver none;
    return bvh4_smin(h, o, d, best, none);
}

// ---------------------------------------------------------------- the parked queries of a wave (wf_finish_bvh)
// bvh4_smin one body at a time: the state the device keeps between two bodies (BvhPark's cur, sp, best, tk and
// the stack), a node step (bvh4_children + pop) and a leaf visit (leaf_scan_min + pop) as bvh4_smin runs them.
struct Bvh4Walk {
    const rt_host::PreparedHost *h = nullptr;
    Vec3D o, d;
    RtSlab sl;
    struct B { uint32_t ref; float tn; };
    std::vector<B> stk;
    uint32_t cur = RT_BVH_EMPTY;
    float best = 0.0f;
    int tk = -1;
    long long bodies = 0, trips = 0; // bodies of its own so far; wave calls it took part in

    void start(const rt_host::PreparedHost &hh, Vec3D oo, Vec3D dd, float best0)
    {
        h = &hh;
        o = oo;
        d = dd;
        sl = rt_slab(o, d, rt_ray_margin(o.x, o.y, o.z, hh.bvh_scale));
        stk.clear();
        cur = 0;
        best = best0;
        tk = -1;
        bodies = trips = 0;
    }
    bool done() const { return cur == RT_BVH_EMPTY; }
    bool at_node() const { return !(cur & RT_BVH_LEAF); }
    bool at_leaf() const { return (cur & RT_BVH_LEAF) && cur != RT_BVH_EMPTY; }
    int leaf_chunks() const { return (int)((cur & 7u) + 1u + 3u) / 4; } // leaf_scan_min's 4-entry chunks
    uint32_t pop()
    {
        while (!stk.empty()) {
            const B e = stk.back();
            stk.pop_back();
            if (e.tn <= best) return e.ref;
        }
        return RT_BVH_EMPTY;
    }
    void node_step()
    {
        ++bodies;
        const float *f = reinterpret_cast<const float *>(&h->bvh4[8 * (size_t)cur]);
        const uint32_t *rf = reinterpret_cast<const uint32_t *>(f + 24);
        float t[4];
        uint32_t r[4];
        for (int k = 0; k < 4; ++k) {
            r[k] = rf[k];
            if (!rt_bvh_box(f[k], f[4 + k], f[8 + k], f[12 + k], f[16 + k], f[20 + k], sl, best, t[k])) t[k] = INFINITY;
        }
        auto cswap = [&](int a, int b) {
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
    void leaf_visit()
    {
        ++bodies;
        const uint32_t first = (cur & ~RT_BVH_LEAF) >> 3, end = first + (cur & 7u) + 1u;
        for (uint32_t e = first; e < end; ++e) { // leaf_scan_min
            float s, b[3];
            if (!rt_tri_plane(h->bvh_a[e], o, d, INFINITY, s) || !(s <= best)) continue;
            const bool lt = s < best;
            if (!lt && tk < 0) continue;
            const RtIsectBary &R = h->bvh_bary[e];
            if (!rt_tri_bary(R.b, R.c, R.d, bitsf(R.rd), o, d, s, b[0], b[1], b[2])) continue;
            if (lt) {
                best = s;
                tk = (int)e;
            } else {
                tk = TK_TIE;
            }
        }
        cur = pop();
    }
};

// what one call of a wave's parked queries executed: the bodies the WAVE ran (a node-phase iteration or a leaf
// visit, whichever lanes take part; chunks: the longest leaf of each visit in 4-entry chunks), the bodies of
// the lanes' own, the lanes in the call and those whose query ended in it
struct WaveTrip {
    long long node_bodies = 0, leaf_bodies = 0, leaf_chunks = 0, lane_bodies = 0, lanes = 0, finished = 0;
};

// bvh_trace.h bvh4_query_budget over the lanes of a wave (the unfinished queries in `q`): one body at a time — a
// node step for the lanes at a node or a leaf visit for the lanes at a leaf, whichever are more (a tie: the node
// step) —, one count per body; the first bodies are owed (a leaf visit if a lane entered at a leaf, then a node
// step if a lane entered at a node), and from `budget` bodies on every unfinished lane parks
inline WaveTrip wave_call_budget(std::vector<Bvh4Walk *> &q, int budget)
{
    WaveTrip w;
    auto count = [&](auto pred) {
        int n = 0;
        for (Bvh4Walk *l : q) n += pred(*l) ? 1 : 0;
        return n;
    };
    for (Bvh4Walk *l : q) {
        ++l->trips;
        ++w.lanes;
    }
    long long bodies = 0;
    bool lead = count([](const Bvh4Walk &l) { return l.at_leaf(); }) > 0;
    bool owed = count([](const Bvh4Walk &l) { return l.at_node(); }) > 0;
    while (true) {
        const int nn = count([](const Bvh4Walk &l) { return l.at_node(); });
        const int nl = count([](const Bvh4Walk &l) { return l.at_leaf(); });
        if (nn + nl == 0) break;
        bool leaf_phase;
        if (lead) {
            leaf_phase = true;
            lead = false;
        } else if (owed) {
            leaf_phase = false;
            owed = false;
        } else {
            if (bodies >= budget) break;
            leaf_phase = nl > nn;
        }
        if (leaf_phase) {
            int chunks = 0;
            for (Bvh4Walk *l : q)
                if (l->at_leaf()) {
                    chunks = std::max(chunks, l->leaf_chunks());
                    l->leaf_visit();
                    ++w.lane_bodies;
                }
            ++w.leaf_bodies;
            w.leaf_chunks += chunks;
        } else {
            for (Bvh4Walk *l : q)
                if (l->at_node()) {
                    l->node_step();
                    ++w.lane_bodies;
                }
            ++w.node_bodies;
        }
        ++bodies;
    }
    for (Bvh4Walk *l : q) w.finished += l->done();
    return w;
}

// bvh_trace.h bvh4_query<PARK> over the lanes of a wave: the while-while loop with a cap on each lane's own node
// steps (the rule before the budget); a lane parks in front of its (cap + 1)-th node step, leaf visits are free
inline WaveTrip wave_call_lane_cap(std::vector<Bvh4Walk *> &q, int cap)
{
    WaveTrip w;
    std::vector<int> steps(q.size(), 0);
    std::vector<char> parked(q.size(), 0);
    for (Bvh4Walk *l : q) {
        ++l->trips;
        ++w.lanes;
    }
    while (true) {
        while (true) { // the node phase: until every lane holds a leaf, is done or is parked
            bool ran = false;
            for (size_t i = 0; i < q.size(); ++i) {
                if (parked[i] || !q[i]->at_node()) continue;
                if (steps[i] >= cap) {
                    parked[i] = 1;
                    continue;
                }
                ++steps[i];
                q[i]->node_step();
                ++w.lane_bodies;
                ran = true;
            }
            if (!ran) break;
            ++w.node_bodies;
        }
        int chunks = 0;
        bool leaf = false;
        for (size_t i = 0; i < q.size(); ++i) {
            if (parked[i] || !q[i]->at_leaf()) continue;
            chunks = std::max(chunks, q[i]->leaf_chunks());
            q[i]->leaf_visit();
            ++w.lane_bodies;
            leaf = true;
        }
        if (!leaf) break;
        ++w.leaf_bodies;
        w.leaf_chunks += chunks;
    }
    for (Bvh4Walk *l : q) w.finished += l->done();
    return w;
}

// bvh_trace.h bvh_bound: the same query on the binary tree (best alone)
template <class Obs>
float bvh_bound(const rt_host::PreparedHost &h, Vec3D o, Vec3D d, float best, Obs &obs)
{
    const RtSlab sl = rt_slab(o, d, rt_ray_margin(o.x, o.y, o.z, h.bvh_scale));
    struct B { uint32_t ref; float tn; };
    B stk[RT_BVH_STACK];
    int sp = 0;
    uint32_t cur = 0;
    while (true) {
        if (!(cur & RT_BVH_LEAF)) {
            obs.bvh_node();
            const RtF4 *nd = &h.bvh_nodes[4 * (size_t)cur];
            const uint32_t c0 = fbits(nd[3].x), c1 = fbits(nd[3].y);
            float tn0, tn1;
            const bool h0 = rt_bvh_box(nd[0].x, nd[0].y, nd[0].z, nd[0].w, nd[1].x, nd[1].y, sl, best, tn0) &&
                            c0 != RT_BVH_EMPTY;
            const bool h1 = rt_bvh_box(nd[1].z, nd[1].w, nd[2].x, nd[2].y, nd[2].z, nd[2].w, sl, best, tn1) &&
                            c1 != RT_BVH_EMPTY;
            if (h0 && h1) {
                const bool sf = tn1 < tn0;
                stk[sp++] = B{sf ? c0 : c1, sf ? tn0 : tn1};
                cur = sf ? c1 : c0;
                continue;
            }
            if (h0 || h1) {
                cur = h0 ? c0 : c1;
                continue;
            }
        } else {
            obs.bvh_leaf();
            const uint32_t first = (cur & ~RT_BVH_LEAF) >> 3, end = first + (cur & 7u) + 1u;
            for (uint32_t e = first; e < end; ++e) {
                float s, b[3];
                obs.bvh_test();
                if (tri_test(h.bvh_a.data(), h.bvh_bary.data(), e, o, d, best, s, b)) best = s;
            }
        }
        bool more = false;
        while (sp > 0) {
            --sp;
            if (stk[sp].tn <= best) {
                cur = stk[sp].ref;
                more = true;
                break;
            }
        }
        if (!more) return best;
    }
}

// ---------------------------------------------------------------- the origin-cell entry
// the grid cell holding p (coop_trace.h kd_origin_frontier: a NaN coordinate goes to cell 0); false: no grid
inline bool cell_of(const rt_host::PreparedHost &h, Vec3D p, size_t &k)
{
    if (h.kd_grid <= 0) return false;
    const int G = h.kd_grid;
    const float q[3] = {p.x, p.y, p.z};
    const float bmin[3] = {h.bounds.min.x, h.bounds.min.y, h.bounds.min.z};
    int c[3];
    for (int a = 0; a < 3; ++a) {
        const float f = (q[a] - bmin[a]) * h.kd_grid_scale[a];
        c[a] = f >= 0.0f ? (f < (float)(G - 1) ? (int)f : G - 1) : 0;
    }
    k = ((size_t)c[2] * G + c[1]) * G + c[0];
    return true;
}

// coop_trace.h kd_origin_frontier's replay: the bounded descent's decisions
// along the stored root path of a grid cell's start node, each checked against
// the path (false: some decision differs -> the root)
template <class Obs>
bool kd_resume(const rt_host::PreparedHost &h, uint32_t start, uint32_t packed, Vec3D o, Vec3D d, float entry,
               float exit_, float s_min, Resume &r, Obs &obs)
{
    if (start == 0xFFFFFFFFu) return false;
    const uint32_t depth = packed & 31u;
    const uint32_t *row = h.kd_rows.data() + 4 * (size_t)(packed >> 5);
    r.sp = 0;
    for (uint32_t k = 0; k < depth; ++k) {
        const uint32_t *rec = row + 4 * k;
        obs.kd_row();
        const uint32_t axis = rec[1] & 3u, anc = rec[2];
        const float split = bitsf(rec[0]);
        const float oax = axis == 0 ? o.x : (axis == 1 ? o.y : o.z);
        const float dax = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
        uint32_t near_c = anc + 1, far_c = rec[1] >> 2;
        if (oax >= split) {
            near_c = rec[1] >> 2;
            far_c = anc + 1;
        }
        const uint32_t taken = rec[3] ? rec[1] >> 2 : anc + 1;
        const float t = (split - oax) / dax;
        if (t >= exit_ || t < 0) {
            if (near_c != taken) return false;
        } else if (t <= entry) {
            if (far_c != taken) return false;
        } else if (t <= s_min) {
            if (far_c != taken) return false;
            entry = t;
        } else {
            if (near_c != taken) return false;
            r.stk[r.sp++] = KdEntry{far_c, t};
            exit_ = t;
        }
    }
    r.node = start;
    r.entry = entry;
    r.exit_ = exit_;
    return true;
}

// ---------------------------------------------------------------- the 8-wide work model (tools)
// 8-wide collapse: child refs (binary inner index / leaf ref) with their boxes
struct Node8 {
    int n = 0;
    uint32_t ref[8];
    float lo[8][3], hi[8][3];
};

inline void child_of(const rt_host::PreparedHost &h, uint32_t node, int c, uint32_t &ref, float *lo, float *hi)
{
    const RtF4 *nd = &h.bvh_nodes[4 * (size_t)node];
    ref = fbits(c == 0 ? nd[3].x : nd[3].y);
    if (c == 0) { lo[0] = nd[0].x; lo[1] = nd[0].y; lo[2] = nd[0].z; hi[0] = nd[0].w; hi[1] = nd[1].x; hi[2] = nd[1].y; }
    else { lo[0] = nd[1].z; lo[1] = nd[1].w; lo[2] = nd[2].x; hi[0] = nd[2].y; hi[1] = nd[2].z; hi[2] = nd[2].w; }
}

inline Node8 collapse(const rt_host::PreparedHost &h, uint32_t node)
{
    Node8 m;
    for (int c = 0; c < 2; ++c) {
        child_of(h, node, c, m.ref[m.n], m.lo[m.n], m.hi[m.n]);
        if (m.ref[m.n] != RT_BVH_EMPTY) ++m.n;
    }
    while (m.n < 8) {
        int pick = -1;
        float area = -1;
        for (int k = 0; k < m.n; ++k) {
            if (m.ref[k] & RT_BVH_LEAF) continue;
            const float ex = m.hi[k][0] - m.lo[k][0], ey = m.hi[k][1] - m.lo[k][1], ez = m.hi[k][2] - m.lo[k][2];
            const float a = ex * ey + ey * ez + ez * ex;
            if (a > area) { area = a; pick = k; }
        }
        if (pick < 0) break;
        const uint32_t inner = m.ref[pick];
        uint32_t r2[2];
        float l2[2][3], h2[2][3];
        child_of(h, inner, 0, r2[0], l2[0], h2[0]);
        child_of(h, inner, 1, r2[1], l2[1], h2[1]);
        int put = 0;
        for (int c = 0; c < 2; ++c) {
            if (r2[c] == RT_BVH_EMPTY) continue;
            const int k = put == 0 ? pick : m.n++;
            ++put;
            m.ref[k] = r2[c];
            memcpy(m.lo[k], l2[c], 12);
            memcpy(m.hi[k], h2[c], 12);
        }
        if (put == 0) { // (both empty: drop the child)
            m.ref[pick] = m.ref[--m.n];
            memcpy(m.lo[pick], m.lo[m.n], 12);
            memcpy(m.hi[pick], m.hi[m.n], 12);
        }
    }
    return m;
}

// the 8-wide collapse of every binary node reachable as a node of it (idx: binary node -> N)
struct Bvh8 {
    std::vector<Node8> N;
    std::vector<int> idx;
};
inline Bvh8 build_bvh8(const rt_host::PreparedHost &h)
{
    Bvh8 w;
    w.idx.assign(h.bvh_nodes.size() / 4, -1);
    std::vector<uint32_t> todo{0};
    while (!todo.empty()) {
        const uint32_t b = todo.back();
        todo.pop_back();
        w.idx[b] = (int)w.N.size();
        w.N.push_back(collapse(h, b));
        const Node8 &nd = w.N.back();
        for (int k = 0; k < nd.n; ++k)
            if (!(nd.ref[k] & RT_BVH_LEAF)) todo.push_back(nd.ref[k]);
    }
    return w;
}

// the 8-wide query: per node, all child boxes at once, every hit leaf child's
// triangles at once (one batch), then the hit inner children nearest first
template <class Obs>
float bvh8(const rt_host::PreparedHost &h, const Bvh8 &w, Vec3D o, Vec3D d, float best, Obs &obs,
           float margin_scale = 1.0f)
{
    const RtSlab sl = rt_slab(o, d, margin_scale * rt_ray_margin(o.x, o.y, o.z, h.bvh_scale));
    struct B { uint32_t r; float tn; } stk[512];
    int sp = 0;
    uint32_t cur = 0;
    while (true) {
        obs.bvh_node();
        const Node8 &nd = w.N[(size_t)w.idx[cur]];
        float tn[8];
        bool hit[8];
        for (int k = 0; k < nd.n; ++k)
            hit[k] = rt_bvh_box(nd.lo[k][0], nd.lo[k][1], nd.lo[k][2], nd.hi[k][0], nd.hi[k][1], nd.hi[k][2], sl,
                                best, tn[k]);
        bool any_leaf = false;
        for (int k = 0; k < nd.n; ++k) {
            if (!hit[k] || !(nd.ref[k] & RT_BVH_LEAF)) continue;
            any_leaf = true;
            const uint32_t f = (nd.ref[k] & ~RT_BVH_LEAF) >> 3, e1 = f + (nd.ref[k] & 7u) + 1u;
            for (uint32_t e = f; e < e1; ++e) {
                float s, b[3];
                obs.bvh_test();
                if (tri_test(h.bvh_a.data(), h.bvh_bary.data(), e, o, d, best, s, b)) best = s;
            }
        }
        if (any_leaf) obs.bvh_leaf();
        int order[8], no = 0;
        for (int k = 0; k < nd.n; ++k)
            if (hit[k] && !(nd.ref[k] & RT_BVH_LEAF) && tn[k] <= best) order[no++] = k;
        std::sort(order, order + no, [&](int a, int b) { return tn[a] > tn[b]; }); // farthest first
        for (int i = 0; i + 1 < no; ++i) stk[sp++] = B{nd.ref[order[i]], tn[order[i]]};
        if (no > 0) { cur = nd.ref[order[no - 1]]; continue; }
        bool more = false;
        while (sp > 0) {
            --sp;
            if (stk[sp].tn <= best) { cur = stk[sp].r; more = true; break; }
        }
        if (!more) return best;
    }
}

// ---------------------------------------------------------------- scene and rays
// load the scene file, build the KD tree and the light list, prepare_host: the
// very arrays the GPU gets.  False (with a line on stderr): one of them failed.
// (prepare_s: prepare_host's wall time.)  "No BVH built" is the caller's check.
inline bool load_prepared(const char *path, RtHostScene &scene, Camera &cam, rt_host::PreparedHost &h,
                          double *prepare_s = nullptr)
{
    if (rt_host::load_scene_file(scene, path, &cam) != RT_OK) {
        fprintf(stderr, "scene load failed\n");
        return false;
    }
    const int n = (int)scene.tris.size();
    std::vector<KD_Tree_Node> nodes;
    std::vector<int> indices;
    Bounding_Box bounds;
    if (rt_host::build_kd_tree(scene.tris.data(), n, nodes, indices, bounds) != RT_OK) {
        fprintf(stderr, "KD build failed\n");
        return false;
    }
    std::vector<int> lights = rt_host::light_list(scene.tris.data(), n);
    const auto t0 = std::chrono::steady_clock::now();
    if (rt_host::prepare_host(scene.tris.data(), n, nodes.data(), (int)nodes.size(), indices.data(),
                              (int)indices.size(), lights.data(), (int)lights.size(), bounds, h) != RT_OK) {
        fprintf(stderr, "prepare failed\n");
        return false;
    }
    if (prepare_s) *prepare_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return true;
}

// a raw float32 (n, 6) ray file {o, d} (tools/dump_rays.py, or_log_rays); false: cannot open
inline bool read_rays_f32(const char *path, std::vector<float> &v)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return false;
    }
    float buf[6 * 4096];
    size_t got;
    while ((got = fread(buf, sizeof(float), 6 * 4096, f)) > 0) v.insert(v.end(), buf, buf + got);
    fclose(f);
    v.resize(v.size() / 6 * 6);
    return true;
}
inline Vec3D ray_o(const std::vector<float> &v, size_t i) { return rt_v3(v[6 * i], v[6 * i + 1], v[6 * i + 2]); }
inline Vec3D ray_d(const std::vector<float> &v, size_t i) { return rt_v3(v[6 * i + 3], v[6 * i + 4], v[6 * i + 5]); }

// The ray makers, over the caller's u(): uniform in [0, 1).  Which ray of a
// program's schedule uses which is the program's own business.
template <class U>
Vec3D unit_vector(U &u)
{
    while (true) {
        Vec3D v = rt_v3(2 * u() - 1, 2 * u() - 1, 2 * u() - 1);
        const float l = rt_dot(v, v);
        if (l > 1e-6f && l <= 1.0f) return rt_normalize(v);
    }
}
template <class U>
Vec3D point_on(const Triangle &tr, U &u) // uniform on the triangle
{
    float b1 = u(), b2 = u();
    if (b1 + b2 > 1) {
        b1 = 1 - b1;
        b2 = 1 - b2;
    }
    return tr.p1 + b1 * (tr.p2 - tr.p1) + b2 * (tr.p3 - tr.p1);
}
inline Vec3D tri_normal(const Triangle &tr) { return rt_normalize(rt_cross(tr.p2 - tr.p1, tr.p3 - tr.p1)); }
// d turned into the plane of tr but for 1e-4 * [-0.5, 0.5) of its normal (a degenerate triangle: d as it is)
template <class U>
Vec3D grazing(Vec3D d, const Triangle &tr, U &u)
{
    const Vec3D nn = tri_normal(tr);
    return nn.x == nn.x ? rt_normalize(d - rt_dot(d, nn) * nn + 1e-4f * (u() - 0.5f) * nn) : d;
}
// d with component a zeroed (NaN where nothing is left)
inline Vec3D axis_parallel(Vec3D d, int a)
{
    if (a == 0) d.x = 0; else if (a == 1) d.y = 0; else d.z = 0;
    return rt_normalize(d);
}
// a chord of a transparent object: from a point on one of the `glass` triangles
// (returned) towards a point on one within span / 2 of it in the mesh's order
template <class U>
const Triangle &glass_chord(const RtHostScene &scene, const std::vector<int> &glass, long long span, U &u, Vec3D &o,
                            Vec3D &d)
{
    const long long ng = (long long)glass.size();
    const size_t gi = (size_t)(u() * glass.size()) % glass.size();
    const Triangle &tr = scene.tris[(size_t)glass[gi]];
    o = point_on(tr, u);
    const long long gj = (long long)gi + (long long)((u() - 0.5f) * span);
    const Triangle &to = scene.tris[(size_t)glass[(size_t)((gj % ng + ng) % ng)]];
    d = rt_normalize(point_on(to, u) - o);
    return tr;
}
// the chord d turned nearly along tr's surface: 0.02-0.2 of the normal, on d's side of it
template <class U>
Vec3D grazing_chord(Vec3D d, const Triangle &tr, U &u)
{
    const Vec3D nn = tri_normal(tr);
    const Vec3D v = unit_vector(u);
    return nn.x == nn.x ? rt_normalize(v - rt_dot(v, nn) * nn + (0.02f + 0.18f * u()) * (rt_dot(d, nn) < 0 ? -1.0f : 1.0f) * nn) : d;
}

} // namespace trace_host
