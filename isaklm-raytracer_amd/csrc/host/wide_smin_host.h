// wide_smin_host.h — host restatement of csrc/wide_bvh.h wide_smin: the
// level-synchronous s_min query over an `arity`-wide collapse of the
// conservative BVH (host/bvh_build.h collapse_bvh_wide), round for round:
// `best` frozen per round, the round's frontier expanded, the leaves the
// PREVIOUS round listed tested with leaf_scan_min's arithmetic, the winner
// kept as the 64-bit key (bits(s) << 32 | slot) lowered by min, a tied s
// recorded when the key a test meets holds the same s; a frontier item is
// its node alone (a node the new best has overtaken is expanded, its
// children culled).  `reversed` walks every list
// backwards: the result must not depend on the order.
//
// Not product code: shared by tests/native/wide_smin_check.cpp (the result
// against the sequential query's, host/trace_host.h bvh4_smin) and
// tools/deep_ray_work.cpp (the work model).  tk_out is bvh4_smin's tk.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../wide_bvh_caps.h"
#include "trace_host.h"

struct WsmWork {
    int rounds = 0;            // dependent rounds
    long long nodes = 0;       // wide nodes expanded
    long long tests = 0;       // leaf slots tested
    int frontier = 0;          // the largest frontier
    int leaves = 0;            // the largest leaf list of a round
    bool cross_round = false;  // a test passed at exactly the frozen best (the later-round tie path)
};

// false: a list outgrew its capacity (the device abandons the query)
inline bool wide_smin_host(const std::vector<RtF4> &wide, int arity, const rt_host::PreparedHost &h, Vec3D o, Vec3D d,
                           float best0, size_t fcap, size_t lcap, bool reversed, float &best_out, int &tk_out,
                           WsmWork &w)
{
    using trace_host::bitsf;
    using trace_host::fbits;
    const RtSlab sl = rt_slab(o, d, rt_ray_margin(o.x, o.y, o.z, h.bvh_scale));
    struct Item { uint32_t node; float tn; };
    std::vector<Item> F{{0u, -INFINITY}}, Fn;
    std::vector<uint32_t> L, Ln;
    unsigned long long key = ~0ull;
    uint32_t tie = 0xFFFFFFFFu;
    float best = best0;
    bool have = false;
    while (!F.empty() || !L.empty()) {
        ++w.rounds;
        w.frontier = (int)F.size() > w.frontier ? (int)F.size() : w.frontier;
        Fn.clear();
        Ln.clear();
        for (size_t q = 0; q < F.size(); ++q) {
            const Item it = F[reversed ? F.size() - 1 - q : q];
            ++w.nodes;
            for (int k = 0; k < arity; ++k) {
                const int c = reversed ? arity - 1 - k : k;
                const RtF4 *rec = &wide[2 * ((size_t)it.node * (size_t)arity + (size_t)c)];
                const uint32_t ref = fbits(rec[1].z);
                float tn;
                if (!rt_bvh_box(rec[0].x, rec[0].y, rec[0].z, rec[0].w, rec[1].x, rec[1].y, sl, best, tn) ||
                    ref == RT_BVH_EMPTY)
                    continue;
                if (ref & RT_BVH_LEAF) {
                    if (Ln.size() == lcap) return false;
                    Ln.push_back(ref);
                } else {
                    if (Fn.size() == fcap) return false;
                    Fn.push_back(Item{ref, tn});
                }
            }
        }
        for (size_t q = 0; q < L.size(); ++q) {
            const uint32_t ref = L[reversed ? L.size() - 1 - q : q];
            const uint32_t first = (ref & ~RT_BVH_LEAF) >> 3, cnt = (ref & 7u) + 1u;
            for (uint32_t k = 0; k < cnt; ++k) {
                const uint32_t slot = first + (reversed ? cnt - 1 - k : k);
                ++w.tests;
                float s, cx, cy, cz;
                if (!rt_tri_plane(h.bvh_a[slot], o, d, INFINITY, s)) continue;
                if (!(s < best || (s == best && have))) continue;
                const RtIsectBary &R = h.bvh_bary[slot];
                if (!rt_tri_bary(R.b, R.c, R.d, bitsf(R.rd), o, d, s, cx, cy, cz)) continue;
                if (s == best) w.cross_round = true;
                const uint32_t sb = fbits(s);
                const unsigned long long mine = (unsigned long long)sb << 32 | slot, old = key;
                key = mine < key ? mine : key;
                if ((uint32_t)(old >> 32) == sb) tie = sb < tie ? sb : tie;
            }
        }
        have = key != ~0ull;
        if (have) best = bitsf((uint32_t)(key >> 32));
        F.swap(Fn);
        L.swap(Ln);
        w.leaves = (int)L.size() > w.leaves ? (int)L.size() : w.leaves;
    }
    best_out = best;
    tk_out = !have ? -1 : (tie == (uint32_t)(key >> 32) ? trace_host::TK_TIE : (int)(uint32_t)key);
    return true;
}
