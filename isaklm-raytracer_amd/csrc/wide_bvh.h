// wide_bvh.h — the s_min query of bvh_trace.h (step 2) for ONE ray per wave
// (wf_long's deep glass paths), level-synchronous over the RT_BVHW_ARITY-wide
// collapse of the conservative BVH (host/bvh_build.h collapse_bvh_wide).
//
// A deep bounce is a chain of dependent memory round trips on a wave that
// runs alone: its time is (rounds) x (latency of a round), not work.  The
// depth-first queries (bvh_bound, bvh4_query) take a round trip per node
// step; here every frontier node's children are box-tested in the same round,
// one (node, child) pair per lane, so a query is as many rounds as the wide
// tree is deep (5-6 at arity 16 on a 2M-triangle scene) plus one.
//
// Per round, with `best` frozen at its value at the round's start:
//  * the frontier's (node, child) pairs are spread over the lanes, 64 at a
//    time: a child box the ray meets within [0, best] (rt_bvh_box) goes to the
//    next frontier (inner) or to the next round's leaf list (leaf).  An item
//    is its node index alone, 4 B: a node whose own entry distance the round's
//    new best has overtaken is still expanded, and every child of it is then
//    culled by the same test (a child's box lies inside its parent's);
//  * the leaves listed by the PREVIOUS round are tested, 8 leaves x 8 slots
//    per 64 lanes, with leaf_scan_min's arithmetic (rt_tri_plane(.., INFINITY,
//    s), s <= best, rt_tri_bary).  The child records and the leaf records of a
//    round are loaded together: one memory round trip per round;
//  * a passing test lowers the wave's 64-bit LDS key (bits(s) << 32 | slot)
//    with atomicMin (s >= 1e-5 > 0: bit order is value order); when the value
//    it replaces, or fails to replace, holds the same s, that s is recorded as
//    tied (atomicMin on a second word).
// Result = bvh4_query's: best = the smallest passing s below best0 (best0 if
// none), tk = the slot that alone has it, RT_TK_TIE when a second slot passes
// at exactly that s (in the same round or a later one), -1 when none.  Both
// are functions of the SET of passing tests alone — the smallest s and how
// many slots share it —, and no box or test is culled that the depth-first
// query's own rule (tn <= best, s <= best, with any proven best) would keep,
// so the result does not depend on the order items are processed in.  A pass
// at s == best0 before any pass is no pass (bvh_trace.h leaf_scan_min): a
// test at s == best passes only once the key holds a hit.
//
// A frontier or leaf list that would outgrow its LDS array abandons the query
// (returns false): the caller traces the ray by the wide KD traversal.
//
// kd_bounded_wave, below, is step 3 (the bounded KD traversal) run by the same
// wave.  tests/native/wide_smin_check.cpp checks a host restatement of the
// query (host/wide_smin_host.h) against the sequential one (host/trace_host.h
// bvh4_smin); tools/deep_ray_work.cpp is its work model.
#pragma once
#include "bvh_trace.h"
#include "wide_bvh_caps.h"

namespace rtk {

#define WSM_KD_STACK 32 // the KD phase's stack: RT_STACK_DEPTH entries (its own LDS: the caller's)
// bytes of per-wave LDS: 2 frontiers and 2 leaf lists of u32 (the KD phase's node block reuses their start)
#define WSM_LDS_BYTES (2 * WSM_FCAP * 4 + 2 * WSM_LCAP * 4)

typedef __attribute__((address_space(3))) volatile uint32_t lds_vu32;

struct WsmLds {
    uint32_t *F;             // 2 x WSM_FCAP frontier items (this round's, the next one's): wide node indices
    uint32_t *L;             // 2 x WSM_LCAP leaf references
    unsigned long long *key; // [0] the winner key, [1] (low word) the smallest tied s
    int fcap, lcap;          // capacities in use (<= WSM_FCAP / WSM_LCAP; RT_DEBUG_WIDE_CAP1: 1)
};

// the KD phase's stack in LDS (kd_bounded_wave's STACK): every lane writes and reads the same values
struct LdsStack1 {
    uint2 *s;
    __device__ __forceinline__ void put(int k, uint32_t node, float t) { s[k] = make_uint2(node, __float_as_uint(t)); }
    __device__ __forceinline__ void get(int k, uint32_t &node, float &entry) const
    {
        const uint2 v = s[k];
        node = v.x;
        entry = __uint_as_float(v.y);
    }
    __device__ __forceinline__ uint32_t node_at(int k) const { return s[k].x; }
    __device__ __forceinline__ float entry_at(int k) const { return __uint_as_float(s[k].y); }
};

// the per-wave scratch carved out of `bytes` (>= WSM_LDS_BYTES, 8-aligned) of LDS
__device__ __forceinline__ WsmLds wsm_lds(void *bytes, unsigned long long *key, int cap1)
{
    uint32_t *f = reinterpret_cast<uint32_t *>(bytes);
    uint32_t *l = f + 2 * WSM_FCAP;
    return WsmLds{f, l, key, cap1 ? 1 : WSM_FCAP, cap1 ? 1 : WSM_LCAP};
}
// Call with all 64 lanes active and a wave-uniform ray.  true: best / tk hold
// the result (wave-uniform); false: abandoned (a list would overflow).
// COUNT (lane 0's counters): RT_CNT_WIDE_CALLS (queries), RT_CNT_WIDE_ROUNDS (dependent rounds),
// RT_CNT_B_BVH_NODE (wide nodes expanded), RT_CNT_B_BVH_TRI (leaf slots tested), RT_CNT_B_BARY
// (barycentric records evaluated) — the figures tools/deep_ray_work.cpp models.
template <bool COUNT>
__device__ __forceinline__ bool wide_smin(const RtDevScene &sc, Vec3D o, Vec3D d, float best0, const WsmLds &W,
                                          float &best_out, int &tk_out, Cnt &c)
{
    constexpr int A = RT_BVHW_ARITY;
    const int lane = __lane_id();
    const RtSlab sl = rt_slab(o, d, rt_ray_margin(o.x, o.y, o.z, sc.bvh_scale));
    lds_vu64 *vkey = (lds_vu64 *)W.key;
    lds_vu32 *F = (lds_vu32 *)W.F;
    lds_vu32 *L = (lds_vu32 *)W.L;
    if (lane == 0) {
        vkey[0] = ~0ull;
        vkey[1] = ~0ull;
        F[0] = 0u; // the root
    }
    int n = 1, nl = 0, cur = 0;
    float best = best0;
    bool have = false;
    if (COUNT && lane == 0) c.v[RT_CNT_WIDE_CALLS]++;
    while (n > 0 || nl > 0) {
        if (COUNT && lane == 0) c.v[RT_CNT_WIDE_ROUNDS]++;
        // (the halves by offset: an array of pointers indexed by `cur` would live in scratch)
        lds_vu32 *Fc = F + cur * WSM_FCAP, *Fn = F + (cur ^ 1) * WSM_FCAP;
        lds_vu32 *Lc = L + cur * WSM_LCAP, *Ln = L + (cur ^ 1) * WSM_LCAP;
        const int pairs = n * A, tests = nl * 8;
        int nn = 0, nln = 0;
        for (int base = 0; base < pairs || base < tests; base += 64) {
            const int p = base + lane;
            // ---- this chunk's loads: a child record and a leaf slot's records per lane (a lane with
            // nothing to do loads record 0 / slot 0: valid addresses, results unused)
            const bool ev = p < pairs;
            const uint32_t it = Fc[ev ? p / A : 0];
            const bool lv0 = p < tests;
            const uint32_t lref = Lc[lv0 ? p >> 3 : 0];
            const RtF4 *rec = sc.bvh_wide + 2 * ((size_t)(ev ? it : 0u) * A + (size_t)(p % A));
            const RtF4 r0 = ldf4(rec), r1 = ldf4(rec + 1);
            const bool lv = lv0 && (uint32_t)(p & 7) <= (lref & 7u);
            const uint32_t slot = lv ? ((lref & ~RT_BVH_LEAF) >> 3) + (uint32_t)(p & 7) : 0u;
            const RtF4 P = ldf4(sc.bvh_a + slot);
            const RtIsectBary *br = sc.bvh_bary + slot;
            const RtF4 B = ldf4(&br->b), C = ldf4(&br->c), D = ldf4(&br->d);
            const float rd = __uint_as_float(br->rd);
            // every load above is issued before the first use below: one memory round trip per chunk
            // (the compiler would otherwise sink the leaf records' loads under the box test)
            asm volatile("" ::"v"(r0.x), "v"(r1.x), "v"(P.x), "v"(B.x), "v"(C.x), "v"(D.x), "v"(rd));
            // ---- expansion: hit children appended in lane order (past the capacity: dropped, and
            // the query abandoned after the chunk loop)
            const uint32_t ref = __float_as_uint(r1.z);
            float tn;
            const bool hit = rt_bvh_box(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, sl, best, tn) && ev && ref != RT_BVH_EMPTY;
            const bool inner = hit && !(ref & RT_BVH_LEAF), leaf = hit && (ref & RT_BVH_LEAF);
            const unsigned long long mi = __ballot(inner), ml = __ballot(leaf);
            const int pi = nn + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mi >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mi, 0u));
            const int pl = nln + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ml >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ml, 0u));
            if (inner && pi < W.fcap) Fn[pi] = ref;
            if (leaf && pl < W.lcap) Ln[pl] = ref;
            nn += __popcll(mi);
            nln += __popcll(ml);
            // ---- leaf tests (leaf_scan_min's arithmetic; best frozen)
            float s;
            const bool plane = lv && rt_tri_plane(P, o, d, INFINITY, s) && (s < best || (s == best && have));
            if (COUNT) {
                const unsigned long long mn = __ballot(ev && p % A == 0), mt = __ballot(lv), mb = __ballot(plane);
                if (lane == 0) {
                    c.v[RT_CNT_B_BVH_NODE] += (unsigned long long)__popcll(mn);
                    c.v[RT_CNT_B_BVH_TRI] += (unsigned long long)__popcll(mt);
                    c.v[RT_CNT_B_BARY] += (unsigned long long)__popcll(mb);
                }
            }
            if (plane) {
                float cx, cy, cz;
                if (rt_tri_bary(B, C, D, rd, o, d, s, cx, cy, cz)) {
                    const uint32_t sb = __float_as_uint(s);
                    const unsigned long long old = atomicMin(W.key, (unsigned long long)sb << 32 | slot);
                    if ((uint32_t)(old >> 32) == sb) atomicMin(reinterpret_cast<uint32_t *>(W.key + 1), sb);
                }
            }
        }
        if (nn > W.fcap || nln > W.lcap) return false;
        const unsigned long long key = vkey[0];
        have = key != ~0ull;
        if (have) best = __uint_as_float((uint32_t)(key >> 32));
        n = nn;
        nl = nln;
        cur ^= 1;
    }
    const unsigned long long key = vkey[0], tie = vkey[1];
    best_out = best;
    tk_out = !have ? -1 : ((uint32_t)tie == (uint32_t)(key >> 32) ? RT_TK_TIE : (int)(uint32_t)key);
    return true;
}

// ---------------------------------------------------------------------------
// Step 3 of bvh_trace.h (kd_bounded) for one ray per wave.  A lone lane's
// descent is a chain of ~21 dependent 8-B node loads; here all 64 lanes run
// the same descent on the same (wave-uniform) ray, so a node that has to come
// from memory is fetched as a block of 64 consecutive nodes, one per lane, into
// LDS: the tree is in pre-order (child 1 = node + 1, a subtree is contiguous),
// so every step into child 1 and the whole bottom of the descent (a subtree
// of <= 63 nodes) is served from the block, and only a step into a child 2
// more than 63 nodes ahead costs a memory round trip.  A leaf's search for T*
// (kd_bounded's fast leaf) compares 64 entries per round trip.  Same
// decisions, same arithmetic, same result as kd_bounded — every lane computes
// it; call with all 64 lanes active.  (The split step and the pop are
// kd_bounded's own functions; the leaf visit is written out: see kd_bounded.)
#define WSM_KD_BLOCK 64 // nodes per block (512 B of the wave's LDS: the start of wide_smin's lists, dead by then)

// COUNT (lane 0's counters, as kd_bounded's): RT_CNT_NODE, RT_CNT_TRI, RT_CNT_HIT.
template <bool COUNT, typename STACK>
__device__ __forceinline__ int kd_bounded_wave(const RtDevScene &sc, const Vec3D o, const Vec3D d, float entry,
                                               const float root_exit, const float s_min, const int tstar, float &hbx,
                                               float &hby, float &hbz, STACK &stk, unsigned long long *block, Cnt &c)
{
    const int lane = __lane_id();
    lds_vu64 *blk = (lds_vu64 *)block;
    uint32_t base = 0xFFFFFFFFu; // first node of the block in LDS (none yet)
    const uint32_t last = (uint32_t)sc.node_count - 1u;
    auto fetch = [&](uint32_t node) -> uint2 {
        if (COUNT && lane == 0) c.v[RT_CNT_NODE]++;
        if (node - base >= (uint32_t)WSM_KD_BLOCK || base == 0xFFFFFFFFu) { // (wave-uniform)
            base = node;
            const uint32_t k = node + (uint32_t)lane;
            const uint2 v = ldc_u2(sc.nodes + 2 * (size_t)(k < last ? k : last)); // (past the end: the last node, unused)
            blk[lane] = (unsigned long long)v.y << 32 | v.x;
        }
        const unsigned long long v = blk[node - base];
        return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
    };
    float exit_ = root_exit;
    const Vec3D y = rt_v3(rt_recip_guard(d.x), rt_recip_guard(d.y), rt_recip_guard(d.z));
    int sp = 0;
    uint32_t node = 0;
    while (true) {
        uint2 nd = fetch(node);
        while ((nd.y & 3u) != RT_LEAF_TAG) {
            const uint32_t axis = nd.y & 3u;
            kd_split_step<KD_DEVICE_DIV, KD_BOUNDED>(nd, kd_axis(axis, o), kd_axis(axis, d), kd_axis(axis, y), s_min, node,
                                                     entry, exit_, sp, stk);
            nd = fetch(node);
        }
        const uint32_t count = nd.y >> 2;
        if (count > 0 && exit_ > s_min) {
            // trace_leaf_node (:115-172): closest starts at the leaf's exit
            float smallest = exit_;
            float bx = 0.0f, by = 0.0f, bz = 0.0f;
            int be = -1;
            const uint32_t e0 = nd.x, e1 = nd.x + count;
            if (tstar >= 0) {
                // T*'s first listing in this leaf (kd_bounded: its test is then the leaf's result)
                uint32_t at = e1;
                for (uint32_t e = e0; e < e1 && at == e1; e += 64) {
                    const uint32_t k = e + (uint32_t)lane;
                    const uint32_t id = *(const RT_CONST uint32_t *)(sc.isect_tri + (k < e1 ? k : e));
                    const unsigned long long m = __ballot(k < e1 && id == (uint32_t)tstar);
                    if (m) at = e + (uint32_t)(__ffsll((long long)m) - 1);
                }
                if (at != e1) {
                    float st, cx, cy, cz;
                    if (COUNT && lane == 0) c.v[RT_CNT_TRI] += 1;
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
            if (be < 0) { // the whole leaf (no T*, or a T* entry that did not pass)
                if (COUNT && lane == 0) c.v[RT_CNT_TRI] += count;
                Cnt none; // (leaf_scan<false> counts nothing: every lane runs it)
                be = leaf_scan<false>(sc.isect_a, sc.isect_bary, e0, e1, o, d, smallest, bx, by, bz, none);
            }
            const int best = be >= 0 ? (int)ldc_u2(&sc.isect_bary[be].rd).y : -1;
            if (best >= 0) {
                if (COUNT && lane == 0) c.v[RT_CNT_HIT]++;
                hbx = bx;
                hby = by;
                hbz = bz;
                return best;
            }
        }
        if (sp == 0) return -1;
        kd_pop(stk, sp, root_exit, node, entry, exit_);
    }
}

} // namespace rtk
