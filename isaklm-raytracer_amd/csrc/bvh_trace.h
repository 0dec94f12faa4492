// bvh_trace.h — trace_ray (rt/trace_ray.cuh:244-318) bounded by the
// conservative BVH (host/bvh_build.h): same result, bit for bit, with a
// fraction of the KD traversal's work.
//
//  1. the reference's scene-box test gives [entry, exit] (no box: miss);
//  2. the BVH query computes s_min = the smallest s of any triangle test
//     that passes with s < exit, with the reference's own per-triangle
//     arithmetic (intersect_triangle + barycentrics, rt/trace_ray.cuh:48-113);
//     the BVH's boxes are grown so that no passing test is culled.  None:
//     every leaf test of the reference fails too (a hit needs s < the leaf's
//     exit <= the root's exit) — a miss;
//  3. the reference's KD traversal, unchanged (split distance, near / far
//     order, the implied-exit stack), except that a split crossing at
//     t <= s_min goes straight to the far side with entry = t: every leaf
//     under the near side has exit <= t <= s_min, and a test there can only
//     pass with s >= s_min >= exit — the reference finds nothing in it and
//     continues at the far side with exactly that entry.  Leaves with exit
//     <= s_min are skipped for the same reason; the others get the
//     reference's leaf test (closest starts at the leaf's exit, strict <,
//     first wins).
// Any lower bound of the smallest passing s would do (a smaller one only
// skips less), so the query may cull with any best-so-far it has proven.
#pragma once
#include "bvh_common.h"
#include "rt_kernels.h"

namespace rtk {

// Scene data is read-only for a kernel's lifetime: loaded through the
// constant address space (a wave-uniform address becomes a scalar load
// through the scalar cache; a divergent one stays a vector load).
// (the host pass of the single-source compile sees plain loads: these are
// __device__ functions and never run there)
#if defined(__HIP_DEVICE_COMPILE__)
#define RT_CONST __attribute__((address_space(4)))
#else
#define RT_CONST
#endif
__device__ __forceinline__ RtF4 ldc4(const RtF4 *p)
{
    const RT_CONST RtF4 *q = (const RT_CONST RtF4 *)p;
    return RtF4{q->x, q->y, q->z, q->w};
}
__device__ __forceinline__ uint2 ldc_u2(const void *p)
{
    const RT_CONST uint32_t *q = (const RT_CONST uint32_t *)p;
    return make_uint2(q[0], q[1]);
}
__device__ __forceinline__ float ldc_f(const uint32_t *p) { return __uint_as_float(*(const RT_CONST uint32_t *)p); }
__device__ __forceinline__ uint4 ldc_u4(const uint32_t *p)
{
    const RT_CONST uint4 *q = (const RT_CONST uint4 *)p;
    return *q;
}

// The tests of leaf entries [e0, e1) in order (trace_leaf_node,
// rt/trace_ray.cuh:115-172: intersect_triangle + calculate_barycentric_
// coordinates, :48-113, on precomputed records): an entry passes with
// dn != 0, s >= 1e-5, s < smallest and barycentrics in [0, 1], and then
// becomes the smallest.  The plane records are loaded 4 at a time (a leaf
// costs a few load round trips instead of one per entry), the plane test is
// pre-screened against the smallest at the start of the chunk (a superset)
// and re-checked in entry order against the running smallest — the
// reference's result.  Returns the passing entry that is the smallest (-1: none) and its
// barycentric coordinates.
template <bool COUNT>
__device__ __forceinline__ int leaf_scan(const RtF4 *plane, const RtIsectBary *bary, uint32_t e0, uint32_t e1, Vec3D o,
                                         Vec3D d, float &smallest, float &bx, float &by, float &bz, Cnt &c)
{
    int best = -1;
    for (uint32_t e = e0; e < e1; e += 4) {
        float s[4];
        bool p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = e + k < e1;
            const RtF4 A = ldc4(plane + (in ? e + k : e));
            p[k] = rt_tri_plane(A, o, d, smallest, s[k]) && in;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!p[k] || !(s[k] < smallest)) continue;
            if (COUNT) c.v[RT_CNT_B_BARY]++;
            float cx, cy, cz;
            if (rt_tri_bary(ldc4(&bary[e + k].b), ldc4(&bary[e + k].c), ldc4(&bary[e + k].d),
                            ldc_f(&bary[e + k].rd), o, d, s[k], cx, cy, cz)) {
                smallest = s[k];
                best = (int)(e + k);
                bx = cx;
                by = cy;
                bz = cz;
            }
        }
    }
    return best;
}

// The s_min query's leaf scan (step 2): as leaf_scan, and it also keeps which
// slot's test set the smallest s (tk; -1: none yet).  A second passing test at
// exactly that s — another triangle: a triangle has one BVH slot — makes it
// RT_TK_TIE.  (A test at s == best0, the root's exit, before any pass is no
// pass: the reference's tests need s < the leaf's exit <= the root's.)
#define RT_TK_TIE (-2)
template <bool COUNT>
__device__ __forceinline__ void leaf_scan_min(const RtF4 *plane, const RtIsectBary *bary, uint32_t e0, uint32_t e1,
                                              Vec3D o, Vec3D d, float &smallest, int &tk, Cnt &c)
{
    for (uint32_t e = e0; e < e1; e += 4) {
        float s[4];
        bool p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = e + k < e1;
            const RtF4 A = ldc4(plane + (in ? e + k : e));
            p[k] = rt_tri_plane(A, o, d, INFINITY, s[k]) && s[k] <= smallest && in;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!p[k] || !(s[k] <= smallest)) continue;
            const bool lt = s[k] < smallest;
            if (!lt && tk < 0) continue; // (at best0, or a tie already)
            if (COUNT) c.v[RT_CNT_B_BARY]++;
            float cx, cy, cz;
            if (rt_tri_bary(ldc4(&bary[e + k].b), ldc4(&bary[e + k].c), ldc4(&bary[e + k].d),
                            ldc_f(&bary[e + k].rd), o, d, s[k], cx, cy, cz)) {
                if (lt) {
                    smallest = s[k];
                    tk = (int)(e + k);
                } else {
                    tk = RT_TK_TIE;
                }
            }
        }
    }
}

// the s_min queries' pop: the next stacked subtree that may still hold a smaller s — entered at
// tn <= best — (RT_BVH_EMPTY: none)
template <typename STACK>
__device__ __forceinline__ uint32_t bvh_pop(STACK &stk, int &sp, const float best)
{
    while (sp > 0) {
        --sp;
        uint32_t n;
        float tn;
        stk.get(sp, n, tn);
        if (tn <= best) return n;
    }
    return RT_BVH_EMPTY;
}

// s_min of step 2: the smallest s < best of any passing test (best if none)
template <bool COUNT, typename STACK>
__device__ __forceinline__ float bvh_bound(const RtDevScene &sc, Vec3D o, Vec3D d, float best, STACK &stk, Cnt &cn)
{
    const RtSlab sl = rt_slab(o, d, rt_ray_margin(o.x, o.y, o.z, sc.bvh_scale));
    int sp = 0;
    uint32_t cur = 0; // the root (always an inner node)
    // "while-while" (SIMT): the lanes descend inner nodes together until each
    // holds a leaf (or is done), then test their leaves together — a lane at a
    // leaf does not drag its wave through every other lane's node steps one
    // iteration at a time
    while (true) {
        while (!(cur & RT_BVH_LEAF)) {
            const RtF4 *nd = sc.bvh_nodes + 4 * (size_t)cur;
            if (COUNT) cn.v[RT_CNT_B_BVH_NODE]++;
            const RtF4 a = ldc4(nd), b = ldc4(nd + 1), c = ldc4(nd + 2);
            const uint2 ch = ldc_u2(nd + 3);
            float tn0, tn1;
            const bool h0 = rt_bvh_box(a.x, a.y, a.z, a.w, b.x, b.y, sl, best, tn0) && ch.x != RT_BVH_EMPTY;
            const bool h1 = rt_bvh_box(b.z, b.w, c.x, c.y, c.z, c.w, sl, best, tn1) && ch.y != RT_BVH_EMPTY;
            if (h0 && h1) {
                const bool second_first = tn1 < tn0;
                stk.put(sp, second_first ? ch.x : ch.y, second_first ? tn0 : tn1);
                ++sp;
                cur = second_first ? ch.y : ch.x;
            } else if (h0 || h1) {
                cur = h0 ? ch.x : ch.y;
            } else {
                cur = bvh_pop(stk, sp, best);
            }
        }
        if (cur == RT_BVH_EMPTY) return best;
        const uint32_t first = (cur & ~RT_BVH_LEAF) >> 3, end = first + (cur & 7u) + 1u;
        if (COUNT) cn.v[RT_CNT_B_BVH_TRI] += end - first;
        float bx, by, bz;
        (void)leaf_scan<COUNT>(sc.bvh_a, sc.bvh_bary, first, end, o, d, best, bx, by, bz, cn);
        cur = bvh_pop(stk, sp, best);
        if (cur == RT_BVH_EMPTY) return best;
    }
}

// s_min of step 2 over the 4-wide collapse of the BVH (host/bvh_build.h
// collapse_bvh4): the same conservative boxes and leaves as bvh_bound's
// binary tree, so the same smallest passing s whatever the visiting order,
// with half the dependent node loads (a node is one 128-B line: the 4 child
// boxes SoA and their references).  The hit children go nearest-first: the
// nearest is descended into, the others pushed farthest-first with their
// entry distance, and popped only while that distance is <= the best s so far.
#ifndef RT_BVH4
#define RT_BVH4 1 // trace_bvh's s_min query on the 4-wide collapse (0: the binary tree)
#endif
//
// The query's state between two bodies — node steps or leaf visits — is (cur,
// sp, best, tk) plus the stack (LDS / spill area): bvh4_query_budget stops a
// query there, hands that state back (returns false), and a later call with
// resume picks it up where it stopped — the same visiting order, the same
// s_min.  The whole-call finisher parks its lanes' unfinished queries so that
// the rest of the wave goes on with shading instead of waiting (wf_finish_bvh).
// (bvh4_query runs a query to its end and returns the result in pk.best / pk.tk.)
struct BvhPark {
    uint32_t cur;
    int sp;
    float best;
    int tk; // the slot whose test set best (leaf_scan_min)
};

// One node step of the 4-wide query: node `cur`'s children whose grown box
// the ray may meet within [0, best], nearest first — the nearest returned,
// the others pushed farthest-first with their entry distance (RT_BVH_EMPTY:
// none hit).  A missed child sorts last by its entry alone (INFINITY; a hit's
// entry is <= best, finite): a 5-comparator network on (entry, reference).
template <typename STACK>
__device__ __forceinline__ uint32_t bvh4_children(const RtDevScene &sc, uint32_t cur, const RtSlab &sl, float best,
                                                  STACK &stk, int &sp)
{
    const RtF4 *nd = sc.bvh4 + 8 * (size_t)cur;
    const RtF4 lx = ldc4(nd), ly = ldc4(nd + 1), lz = ldc4(nd + 2), hx = ldc4(nd + 3), hy = ldc4(nd + 4),
               hz = ldc4(nd + 5);
    const uint4 rf = ldc_u4(reinterpret_cast<const uint32_t *>(nd + 6));
    float t0, t1, t2, t3;
    uint32_t r0 = rf.x, r1 = rf.y, r2 = rf.z, r3 = rf.w;
    // (an unused slot's box is culled by its own slab test: host/bvh_build.cpp collapse_bvh4)
    if (!rt_bvh_box(lx.x, ly.x, lz.x, hx.x, hy.x, hz.x, sl, best, t0)) t0 = INFINITY;
    if (!rt_bvh_box(lx.y, ly.y, lz.y, hx.y, hy.y, hz.y, sl, best, t1)) t1 = INFINITY;
    if (!rt_bvh_box(lx.z, ly.z, lz.z, hx.z, hy.z, hz.z, sl, best, t2)) t2 = INFINITY;
    if (!rt_bvh_box(lx.w, ly.w, lz.w, hx.w, hy.w, hz.w, sl, best, t3)) t3 = INFINITY;
    auto cswap = [](float &ta, uint32_t &ra, float &tb, uint32_t &rb) {
        const bool sw = tb < ta;
        const float t = sw ? tb : ta, u = sw ? ta : tb;
        const uint32_t r = sw ? rb : ra, q = sw ? ra : rb;
        ta = t;
        tb = u;
        ra = r;
        rb = q;
    };
    cswap(t0, r0, t1, r1);
    cswap(t2, r2, t3, r3);
    cswap(t0, r0, t2, r2);
    cswap(t1, r1, t3, r3);
    cswap(t1, r1, t2, r2);
    if (t3 != INFINITY) {
        stk.put(sp, r3, t3);
        ++sp;
    }
    if (t2 != INFINITY) {
        stk.put(sp, r2, t2);
        ++sp;
    }
    if (t1 != INFINITY) {
        stk.put(sp, r1, t1);
        ++sp;
    }
    return t0 != INFINITY ? r0 : RT_BVH_EMPTY;
}

template <bool COUNT, typename STACK>
__device__ __forceinline__ void bvh4_query(const RtDevScene &sc, Vec3D o, Vec3D d, float best0, STACK &stk, Cnt &cn,
                                           BvhPark &pk)
{
    const RtSlab sl = rt_slab(o, d, rt_ray_margin(o.x, o.y, o.z, sc.bvh_scale));
    int sp = 0;
    uint32_t cur = 0; // the root (always an inner node)
    float best = best0;
    int tk = -1;
    while (true) {
        while (!(cur & RT_BVH_LEAF)) {
            if (COUNT) cn.v[RT_CNT_B_BVH_NODE]++;
            const uint32_t next = bvh4_children(sc, cur, sl, best, stk, sp);
            cur = next != RT_BVH_EMPTY ? next : bvh_pop(stk, sp, best);
        }
        if (cur == RT_BVH_EMPTY) break;
        const uint32_t first = (cur & ~RT_BVH_LEAF) >> 3, end = first + (cur & 7u) + 1u;
        if (COUNT) cn.v[RT_CNT_B_BVH_TRI] += end - first;
        leaf_scan_min<COUNT>(sc.bvh_a, sc.bvh_bary, first, end, o, d, best, tk, cn);
        cur = bvh_pop(stk, sp, best);
        if (cur == RT_BVH_EMPTY) break;
    }
    pk.best = best;
    pk.tk = tk;
}

// The parked query scheduled and budgeted by the WAVE's work (wf_finish_bvh, WF_BVH_BUDGET).  A cap on a lane's
// own node steps does not bound what its wave executes: leaf visits were never counted, and in a while-while
// loop the node runs of lanes whose leaves fall at different places do not line up — the wave ran 16 node-phase
// iterations and 5 leaf visits per call for lanes that took at most 6 node steps each (profiles/query_budget/).
// Here the wave executes one BODY at a time: a node step for the lanes that hold a node, or a leaf visit for the
// lanes that hold a leaf, whichever has more lanes waiting (a tie: the node step) — the others wait with their
// state untouched.  Every body counts once, in a scalar (the loop's conditions are ballots: wave-uniform over
// the lanes in this call), and at `budget` bodies every lane whose query is unfinished parks: in front of a node
// step or in front of a leaf visit (cur is then the leaf's reference, and the resumed lane goes on with its scan).
//
// Progress rule: whatever the budget, a lane with an unfinished query executes at least one body of its own in
// every call.  New rays join the wave in every trip and always start at a node, so a majority (or a node phase
// that always ran first) could starve a lane parked at a leaf for ever.  Hence the first bodies of a call are
// owed: a leaf visit if any lane entered at a leaf, then a node step if any lane entered at a node — neither
// subject to the budget.  A query therefore takes no more calls than it has bodies.
//
// A lane's own sequence of node steps, leaf visits and pops is bvh4_query's: only where it waits and where it
// pauses moves.  Returns true with the result in pk.best / pk.tk, false with the state in pk.
template <bool COUNT, typename STACK>
__device__ __forceinline__ bool bvh4_query_budget(const RtDevScene &sc, Vec3D o, Vec3D d, float best0, STACK &stk,
                                                  Cnt &cn, const int budget, bool resume, BvhPark &pk)
{
    const RtSlab sl = rt_slab(o, d, rt_ray_margin(o.x, o.y, o.z, sc.bvh_scale));
    int sp = 0;
    uint32_t cur = 0; // the root (always an inner node)
    float best = best0;
    int tk = -1;
    if (resume) {
        sp = pk.sp;
        cur = pk.cur;
        best = pk.best;
        tk = pk.tk;
    }
    auto leaf_visit = [&]() {
        const uint32_t first = (cur & ~RT_BVH_LEAF) >> 3, end = first + (cur & 7u) + 1u;
        if (COUNT) cn.v[RT_CNT_B_BVH_TRI] += end - first;
        leaf_scan_min<COUNT>(sc.bvh_a, sc.bvh_bary, first, end, o, d, best, tk, cn);
        cur = bvh_pop(stk, sp, best);
    };
    int bodies = 0;                                       // (wave-uniform, as everything that steers the loop)
    bool lead = __any((cur & RT_BVH_LEAF) != 0u) != 0;    // lanes resumed at a leaf (never RT_BVH_EMPTY: that is done)
    bool owed = __any(!(cur & RT_BVH_LEAF)) != 0;         // lanes entered at a node
    while (true) {
        const bool node = !(cur & RT_BVH_LEAF), leaf = !node && cur != RT_BVH_EMPTY;
        const unsigned long long nm = __ballot(node), lm = __ballot(leaf);
        if (!(nm | lm)) break;
        bool leaf_phase;
        if (lead) {
            leaf_phase = true;
            lead = false;
        } else if (owed) {
            leaf_phase = false;
            owed = false;
        } else {
            if (bodies >= budget) break;
            leaf_phase = __popcll(lm) > __popcll(nm);
        }
        if (leaf_phase) {
            if (leaf) leaf_visit();
        } else if (node) {
            if (COUNT) cn.v[RT_CNT_B_BVH_NODE]++;
            const uint32_t next = bvh4_children(sc, cur, sl, best, stk, sp);
            cur = next != RT_BVH_EMPTY ? next : bvh_pop(stk, sp, best);
        }
        ++bodies;
    }
    pk.cur = cur;
    pk.sp = sp;
    pk.best = best;
    pk.tk = tk;
    return cur == RT_BVH_EMPTY;
}

// (tstar: the triangle whose test alone set s_min — kd_bounded's fast leaf —, else -1; tk: its BVH slot,
// -1 / RT_TK_TIE as leaf_scan_min leaves it)
template <bool COUNT, typename STACK>
__device__ __forceinline__ float bvh4_bound(const RtDevScene &sc, Vec3D o, Vec3D d, float best, STACK &stk, Cnt &cn,
                                            int &tstar, int &tk)
{
    BvhPark pk;
    bvh4_query<COUNT>(sc, o, d, best, stk, cn, pk);
    tk = pk.tk;
    tstar = pk.tk >= 0 ? (int)sc.bvh_bary[pk.tk].tri : -1;
    return pk.best;
}
template <bool COUNT, typename STACK>
__device__ __forceinline__ float bvh4_bound(const RtDevScene &sc, Vec3D o, Vec3D d, float best, STACK &stk, Cnt &cn,
                                            int &tstar)
{
    int tk;
    return bvh4_bound<COUNT>(sc, o, d, best, stk, cn, tstar, tk);
}

// The T* certificate (bvh_common.h rt_kd_cert): where it holds, step 3's descent would end in
// a leaf that lists T* and return T*'s own test — the triangle of BVH slot tk with the barycentrics of
// rt_tri_bary on that slot's record at s = s_min (the s its rt_tri_plane gave the query: leaf_scan_min),
// the same arithmetic on the same floats as kd_bounded's T* leaf runs on the KD entry's copy.  True: the
// hit is set (RT_CNT_HIT counted where `count`); false: the caller runs the descent.  COUNT: c.cert[0] counts
// the certified rays; the callers count in c.cert[1] the hits found by a KD descent instead — rays the certificate
// did not cover and rays the bound does not apply to —, so cert[0] + cert[1] = RT_CNT_HIT.  (A few descents of
// bounded rays miss although a test passes: the reference's split-at-the-origin quirk)
template <bool COUNT>
__device__ __forceinline__ bool kd_certified(const RtDevScene &sc, const Vec3D o, const Vec3D d, const float entry,
                                             const float root_exit, const float s_min, const int tk, int &hit,
                                             float &hbx, float &hby, float &hbz, Cnt &c, const bool count = true)
{
#if RT_KD_CERT
    if (!sc.kd_cert.safe) return false;
    if (rt_kd_cert(sc.kd_cert, o, d, entry, root_exit, s_min, tk) != RT_CERT_OK) return false;
    const RtIsectBary *r = sc.bvh_bary + tk;
    float cx, cy, cz;
    if (!rt_tri_bary(ldc4(&r->b), ldc4(&r->c), ldc4(&r->d), ldc_f(&r->rd), o, d, s_min, cx, cy, cz))
        return false; // (never: this test passed in the query)
    if (COUNT && count) {
        c.v[RT_CNT_HIT]++;
        c.cert[0]++;
    }
    hit = (int)ldc_u2(&r->rd).y;
    hbx = cx;
    hby = cy;
    hbz = cz;
    return true;
#else
    return false;
#endif
}

// step 3: the reference's KD traversal with the skip bound s_min (-inf: the
// plain traversal, trace()) and T* (-1: none), from the scene box's [entry,
// root_exit].  Returns the triangle or -1, the hit's barycentrics and hs = the
// *t of the winning intersect_triangle (rt/trace_ray.cuh:90-97), the value
// trace_leaf_node's smallest_t ends on — only with WANT_S: the occlusion
// query's (trace_s, occluded_bvh); the render kernels leave hs alone.
// The leaf visit — T*'s entry alone, else leaf_scan — stays written out here and
// in wide_bvh.h kd_bounded_wave (they differ in the search for T*'s listing):
// as one function taking the search, the search loop's exit compiles otherwise
// and the render and query kernels change length (profiles/kd_step/README.md).
template <bool COUNT, bool WANT_S = false, typename STACK>
__device__ __forceinline__ int kd_bounded(const RtDevScene &sc, const Vec3D o, const Vec3D d, float entry,
                                          const float root_exit, const float s_min, const int tstar, float &hbx,
                                          float &hby, float &hbz, float &hs, STACK &stk, Cnt &c)
{
    float exit_ = root_exit;
    const Vec3D y = rt_v3(rt_recip_guard(d.x), rt_recip_guard(d.y), rt_recip_guard(d.z));
    int sp = 0;
    uint32_t node = 0;
    while (true) {
        uint2 nd = ldc_u2(sc.nodes + 2 * (size_t)node);
        if (COUNT) c.v[RT_CNT_NODE]++;
        while ((nd.y & 3u) != RT_LEAF_TAG) {
            const uint32_t axis = nd.y & 3u;
            kd_split_step<KD_DEVICE_DIV, KD_BOUNDED>(nd, kd_axis(axis, o), kd_axis(axis, d), kd_axis(axis, y), s_min, node,
                                                     entry, exit_, sp, stk);
            nd = ldc_u2(sc.nodes + 2 * (size_t)node);
            if (COUNT) c.v[RT_CNT_NODE]++;
        }
        const uint32_t count = nd.y >> 2;
        if (count > 0 && exit_ > s_min) {
            // trace_leaf_node (:115-172): closest starts at the leaf's exit
            float smallest = exit_;
            float bx = 0.0f, by = 0.0f, bz = 0.0f;
            int be = -1;
            const uint32_t e0 = nd.x, e1 = nd.x + count;
            if (tstar >= 0) {
                // s_min is the smallest s of every passing test and T*'s test alone has it (tstar,
                // leaf_scan_min): where this leaf lists T*, T*'s test is the leaf's result — it passes
                // (s_min < exit), nothing passes below s_min, nothing else at it — and the reference's
                // scan returns exactly that entry (its first listing; its arithmetic on the same record)
                uint32_t at = e1;
                for (uint32_t e = e0; e < e1 && at == e1; e += 4) {
                    uint32_t id[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) id[k] = *(const RT_CONST uint32_t *)(sc.isect_tri + (e + k < e1 ? e + k : e));
#pragma unroll
                    for (int k = 3; k >= 0; --k)
                        if (e + k < e1 && id[k] == (uint32_t)tstar) at = e + k;
                }
                if (at != e1) { // T*'s entry alone: leaf_scan's test of it, not a 4-wide chunk
                    float st, cx, cy, cz;
                    if (COUNT) c.v[RT_CNT_TRI] += 1;
                    if (rt_tri_plane(ldc4(sc.isect_a + at), o, d, smallest, st) &&
                        rt_tri_bary(ldc4(&sc.isect_bary[at].b), ldc4(&sc.isect_bary[at].c), ldc4(&sc.isect_bary[at].d),
                                    ldc_f(&sc.isect_bary[at].rd), o, d, st, cx, cy, cz)) {
                        smallest = st;
                        be = (int)at;
                        bx = cx;
                        by = cy;
                        bz = cz;
                    }
                }
            }
            if (be < 0) { // the whole leaf (no T*, or a T* entry that did not pass — excluded above)
                if (COUNT) c.v[RT_CNT_TRI] += count;
                be = leaf_scan<COUNT>(sc.isect_a, sc.isect_bary, e0, e1, o, d, smallest, bx, by, bz, c);
            }
            const int best = be >= 0 ? (int)ldc_u2(&sc.isect_bary[be].rd).y : -1;
            // (a listed entry's triangle index is >= 0: WANT_S asks the entry, as the occlusion kernel always did)
            if (WANT_S ? be >= 0 : best >= 0) {
                if (COUNT) c.v[RT_CNT_HIT]++;
                hbx = bx;
                hby = by;
                hbz = bz;
                if (WANT_S) hs = smallest;
                return best;
            }
        }
        if (sp == 0) return -1;
        kd_pop(stk, sp, root_exit, node, entry, exit_);
    }
}

// trace_ray with the bound: returns the triangle index or -1 and the hit's
// barycentric coordinates, bit-identical to trace().  COUNT (RT_TRAVERSAL_
// BOUNDED_COUNTED): this traversal's own work — RT_CNT_RAY, RT_CNT_NODE / _TRI
// (KD nodes / plane tests), RT_CNT_B_* (BVH nodes / plane tests, barycentric
// records of both phases)
template <bool COUNT, typename STACK>
__device__ __forceinline__ int trace_bvh(const RtDevScene &sc, const Vec3D o, const Vec3D d, float &hbx, float &hby,
                                         float &hbz, STACK &stk, Cnt &c)
{
    if (COUNT) c.v[RT_CNT_RAY]++;
    float entry, exit_;
    if (!bbox_hit(sc, o, d, entry, exit_)) return -1;
    const float root_exit = exit_;
    float s_min = -INFINITY; // (the plain KD traversal)
    int tstar = -1;
    if (rt_bounded_ray(o, d, sc.split_vals, sc.split_off)) {
        int tk = -1;
        s_min = RT_BVH4 ? bvh4_bound<COUNT>(sc, o, d, exit_, stk, c, tstar, tk)
                        : bvh_bound<COUNT>(sc, o, d, exit_, stk, c);
        if (!(s_min < root_exit)) return -1;
        int hit;
        if (kd_certified<COUNT>(sc, o, d, entry, root_exit, s_min, tk, hit, hbx, hby, hbz, c)) return hit;
    }
    float hs; // (the occlusion query's)
    const int h = kd_bounded<COUNT>(sc, o, d, entry, root_exit, s_min, tstar, hbx, hby, hbz, hs, stk, c);
    if (COUNT && h >= 0) c.cert[1]++;
    return h;
}

// trace_bvh with the s_min query parked after `budget` bodies of its wave (bvh4_query_budget), and with the KD descent of
// a ray the certificate does not cover put off where the caller asks (defer_kd).  Returns RT_PARK_DONE
// with the hit in `hit` (-1: miss) — trace_bvh's result, bit for bit —, RT_PARK_BVH (pk holds the query's
// state) or RT_PARK_KD (pk.best / pk.tk hold s_min and its slot: only the descent is left); call again
// with that value as `resume`.  Lanes are independent paths: any schedule gives the same bits.
#define RT_PARK_DONE 0
#define RT_PARK_BVH 1
#define RT_PARK_KD 2
template <bool COUNT, typename STACK>
__device__ __forceinline__ int trace_bvh_park(const RtDevScene &sc, const Vec3D o, const Vec3D d, int &hit, float &hbx,
                                              float &hby, float &hbz, STACK &stk, Cnt &c, int budget, int resume,
                                              bool defer_kd, BvhPark &pk)
{
    if (COUNT && resume == RT_PARK_DONE) c.v[RT_CNT_RAY]++;
    hit = -1;
    float entry, exit_;
    if (!bbox_hit(sc, o, d, entry, exit_)) return RT_PARK_DONE;
    const float root_exit = exit_;
    float s_min = -INFINITY; // (the plain KD traversal)
    int tstar = -1;
    if (rt_bounded_ray(o, d, sc.split_vals, sc.split_off)) {
        if (resume != RT_PARK_KD) {
            if (!bvh4_query_budget<COUNT>(sc, o, d, exit_, stk, c, budget, resume == RT_PARK_BVH, pk)) return RT_PARK_BVH;
            if (!(pk.best < root_exit)) return RT_PARK_DONE;
            if (kd_certified<COUNT>(sc, o, d, entry, root_exit, pk.best, pk.tk, hit, hbx, hby, hbz, c))
                return RT_PARK_DONE;
            if (RT_KD_CERT && defer_kd) return RT_PARK_KD;
        }
        s_min = pk.best;
        if (pk.tk >= 0) tstar = (int)sc.bvh_bary[pk.tk].tri;
    }
    float hs; // (the occlusion query's)
    hit = kd_bounded<COUNT>(sc, o, d, entry, root_exit, s_min, tstar, hbx, hby, hbz, hs, stk, c);
    if (COUNT && hit >= 0) c.cert[1]++;
    return RT_PARK_DONE;
}

// ---- the occlusion query (rt_occluded, query.hip) ----
// trace_ray's hit and its ray parameter by the plain KD traversal (the rays
// outside the bound's domain, RT_TRAVERSAL_KD): -1 = miss
template <typename STACK>
__device__ __forceinline__ int trace_s(const RtDevScene &sc, const Vec3D o, const Vec3D d, float &hs, STACK &stk,
                                       Cnt &c)
{
    float entry, exit_;
    if (!bbox_hit(sc, o, d, entry, exit_)) return -1;
    float bx, by, bz;
    return kd_bounded<false, true>(sc, o, d, entry, exit_, -INFINITY, -1, bx, by, bz, hs, stk, c);
}

// Whether trace_ray hits with a ray parameter s < tmax (tmax > 1e-5: the
// caller's rule), for a ray inside the bound's domain (rt_bounded_ray and
// query.hip's gate).  The s_min query is capped at best0 = min(root exit,
// tmax): when nothing passes below best0 the answer is "no" without any KD
// descent — a reference hit needs s < its leaf's exit <= the root's exit, so
// any hit has s >= tmax — and every BVH box entered beyond tmax is culled.
// When something does, the capped query returns the uncapped one's s_min, T*
// and tie mark (a box it culls is entered above best0 > s_min and holds
// neither the minimum nor a tie of it; a test at s == best0 before any pass is
// no pass, as at the root's exit), and the KD phase is trace_bvh's.
// (No KD leaf is pruned by entry >= tmax: the reference's leaf test accepts s
// below the leaf's entry.)
// (early: whether the capped query alone answered — a counting build's figure, tools/occlusion_bench.py)
template <typename STACK>
__device__ __forceinline__ bool occluded_bvh(const RtDevScene &sc, const Vec3D o, const Vec3D d, const float tmax,
                                             STACK &stk, Cnt &c, bool &early)
{
    early = false;
    float entry, exit_;
    if (!bbox_hit(sc, o, d, entry, exit_)) return false;
    const float root_exit = exit_;
    const float best0 = fminf(root_exit, tmax);
    int tstar = -1;
    const float s_min =
        RT_BVH4 ? bvh4_bound<false>(sc, o, d, best0, stk, c, tstar) : bvh_bound<false>(sc, o, d, best0, stk, c);
    if (!(s_min < best0)) {
        early = true;
        return false;
    }
    float s = INFINITY, bx, by, bz;
    const int tri = kd_bounded<false, true>(sc, o, d, entry, root_exit, s_min, tstar, bx, by, bz, s, stk, c);
    return tri >= 0 && s < tmax;
}

} // namespace rtk
