// wavefront.hip — the wavefront variant of the render hot path (kernel 1).
//
// The per-pixel loop of rt/path_tracing.cuh:268-325 is cut at its ray
// queries.  Each iteration runs two kernels over a compacted queue of rays:
//   wf_trace  — trace_ray (rt/trace_ray.cuh:244-318) for every queued ray;
//               nothing else, so it is small (VGPRs) and keeps more waves in
//               flight to hide the dependent node/triangle loads
//   wf_shade  — consumes each hit: emission, BSDF sample, NEE shadow-ray set
//               up, roulette, accumulation, and starts the pixel's next pass
//               (adaptive test + camera ray) when its path ends; appends the
//               next ray of every live path to the other queue
// Path state lives in HBM between kernels (SoA, ~72 B per pixel).  Queue
// order is arbitrary (wave-aggregated atomics) but every pixel's sequence of
// events is the reference's, so results are bit-identical to the megakernel
// and the CPU oracle.
//
// This file is the host side; the kernels are in the headers it includes, in
// their order of definition: wf_state.h, wf_queue_kernels.h, wf_shade.h,
// wf_finish_kernels.h, wf_long.h (one translation unit).
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <chrono>
#include <atomic>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

#include "bvh_trace.h"
#include "path_event.h"
#include "rt_kernels.h"
#include "rt_launch.h"
#include "rt_workspace.h"
#include "wf_check_grid.h"

using namespace rtk;

#include "wf_state.h"
#include "wf_queue_kernels.h"
#include "wf_shade.h"
#include "wf_finish_kernels.h"
#include "wf_long.h"

// ---------------------------------------------------------------- launcher
namespace {

// one launch for a counting call (K<true>) or a plain one (K<false>): the same grid, block, stream and arguments
#define WF_LAUNCH_COUNT(count, K, grid, block, stream, ...)                          \
    do {                                                                             \
        if (count) hipLaunchKernelGGL(K<true>, grid, block, 0, stream, __VA_ARGS__); \
        else hipLaunchKernelGGL(K<false>, grid, block, 0, stream, __VA_ARGS__);      \
    } while (0)

// One pipeline = its own ray queues, hits, counters, stack spill area and
// HIP stream over a disjoint set of 16x16 pixel tiles (tile % npipes).  The
// pipelines run concurrently (one host thread each), so the latency-bound
// tail of one pipeline's trace launches and its finisher overlap the other
// pipelines' bulk work.  Per-pixel path state is shared (pixels are disjoint).
// The whole-call mode uses pipeline 0 and runs its persistent wf_long on
// pipeline 1's or 2's stream (alternating per call: a chained call's wf_long
// may start while the previous one still runs deep paths).
struct Pipe {
    std::vector<std::pair<float, float>> trace_iv; // profiled trace launches: [start, end] ms after the call's start
    WfState st{};
    hipStream_t stream = nullptr;
    uint32_t *host_count = nullptr;
    hipEvent_t ev[6] = {};   // RtOptions.profile
    SerialEvent join;      // after the pipeline's last launch
    SerialEvent long_done; // whole-call mode: after a persistent wf_long on this stream
    hipEvent_t fin_done = nullptr; // after the finisher (the host polls it while kicking wf_long slices)
    RtProfile prof{};
};

// one whole call (launch_whole): what its launch, a coalesced batch and its chain's drain all go by
struct WholeCall {
    int dev = 0;
    RtDevScene sc{};
    RtDevFrame fr{};
    RtDevCamera cam{};
    hipStream_t stream = nullptr;
    int long_depth = 0;
    bool prof = false, overlap = false;
    uint32_t check_mask = 0;
    int debug = 0;
    bool count = false;
};

// the frame a chained call continues (RtOptions.overlap): everything a pixel's
// passes depend on besides its own G_Buffer state
struct ChainKey {
    const void *nodes, *bvh, *fb, *sq, *count, *rng;
    int width, height, adaptive, min_samples, max_depth, shard_id, num_shards, long_depth;
    float tolerance;
    RtDevCamera cam;
};

ChainKey chain_key(const WholeCall &c)
{
    const RtDevFrame &fr = c.fr;
    ChainKey key;
    memset(&key, 0, sizeof key);
    key.nodes = c.sc.nodes;
    key.bvh = c.sc.bvh_nodes;
    key.fb = fr.fb;
    key.sq = fr.sq;
    key.count = fr.count;
    key.rng = fr.rng;
    key.width = fr.width;
    key.height = fr.height;
    key.adaptive = fr.adaptive;
    key.min_samples = fr.min_samples;
    key.max_depth = fr.max_depth;
    key.shard_id = fr.shard_id;
    key.num_shards = fr.num_shards;
    key.long_depth = c.long_depth;
    key.tolerance = fr.tolerance;
    key.cam = c.cam;
    return key;
}

// Chained calls of fewer passes than RtOptions.coalesce_passes are coalesced
// on the host: such a call is recorded (its passes added to the pending batch
// of the same frame, options and stream) and the batch is launched as ONE
// chained call once it holds that many passes, or before anything that must
// see it (any other call, a join — rt_join and the library's readers —, the
// profile readers, rt_shutdown).  k chained calls of p passes are the same
// per-pixel pass sequence as one call of k*p passes: bit-identical.
struct Pending {
    bool on = false;
    WholeCall call{}; // (its fr.passes: the batch's)
    ChainKey key{};
};

// call c (its frame: key) may join the pending batch: the same options, stream and frame, and the passes fit
bool coalesces(const Pending &b, const WholeCall &c, const ChainKey &key)
{
    return b.call.dev == c.dev && b.call.stream == c.stream && b.call.prof == c.prof &&
           b.call.check_mask == c.check_mask && b.call.debug == c.debug && b.call.sc.nodes == c.sc.nodes &&
           memcmp(&key, &b.key, sizeof key) == 0 && (long long)b.call.fr.passes + c.fr.passes < (1LL << 28);
}

struct Workspace {
    Pending pend; // coalesced chained calls not yet launched
    size_t slots = 0;
    int grid = 0;
    int spill_pipes = 0;
    void *blob = nullptr;
    Pipe pipe[WF_MAX_PIPES];
    bool streams_ok = false;
    hipEvent_t fork = nullptr, ev0 = nullptr, ev1 = nullptr, fin_ready = nullptr;
    SerialEvent long_ev; // after the last wf_long slice on the caller's stream (queue mode)
    uint32_t *fin_live = nullptr; // 8 producer words (whole-call mode, one per call in flight: call % 8)
    uint32_t *heavy_list = nullptr; // (WfState.heavy_list: every pixel at most once)
    RtF4 *chk = nullptr;          // the exactness guard's records (2 x chk_cap x 3 RtF4; allocated on the
                                  // first call with the guard on, regrown for a larger frame) and their counter
    uint32_t chk_cap = 0;
    uint32_t *chk_ctr = nullptr;
    // the join's hand-off check (wf_verify): its result words (own allocation: they outlive a
    // blob reallocation), a whole call with the hand-off ran since the last check, a check's
    // result not yet read by a host join
    uint32_t *verify_res = nullptr;
    bool verify_pending = false;
    bool verify_unread = false;
    // after the last wf_verify (on whatever stream ran the join): every later launch on the workspace,
    // and the host's read of verify_res, wait for it — it rewrites every pixel's ownership word
    SerialEvent verify_ev;
    int cus = 0;                                // compute units of the device (the finisher's grid)
    unsigned long long *long_log_buf = nullptr; // RT_DEBUG_LONG_LOG records
    // the guard's wf_check per record parity on pipeline 2: the event after it (the call two
    // later, whose finisher writes the same records, waits for it)
    SerialEvent chk_done[2];
    // RtOptions.profile of whole calls: per profiled call its finisher's span on the device
    // ({first wave start, last wave end}, s_memrealtime) in a ring of WF_PROF_SLOTS, resolved
    // into RtProfile records by rt_last_profile / rt_profile_history (they join first)
    unsigned long long *spans = nullptr;
    unsigned long long prof_seq = 0;
    struct PendingProf {
        unsigned long long seq;
        int passes;
    };
    std::vector<PendingProf> prof_pending;
    std::vector<RtProfile> prof_hist; // resolved, since the last rt_profile_history reset (the newest
                                      // WF_PROF_HISTORY: a profiling caller that never reads it stays bounded)
    unsigned long long call_seq = 0;
    bool chain_open = false; // the last call was a whole-call call with RtOptions.overlap
    ChainKey key{};
    WholeCall last{};        // the last whole call, its fr.reset cleared (an open chain's drain runs with it)
    RtProfile prof{};        // last profiled call
};

// Per device (rt_workspace.h).  Every entry point of this file — rt_launch_wavefront, rt_wavefront_join,
// rt_wavefront_device_init, rt_last_profile, rt_profile_history, rt_wavefront_shutdown — takes g_ws.mu once,
// at its top, and holds it until its launches are enqueued (a queue-mode call: until launch_queue returns);
// everything below them takes a Workspace & and never locks, launch_queue's pipeline threads included.
DeviceSlots<Workspace> g_ws;

// What a join waits for, f(event) for each until one fails: the last hand-off check first (another stream
// may have run it, and it rewrites every ownership word), every pipeline's last launch and persistent
// wf_long, the queue mode's last wf_long slice
template <typename F>
bool each_tail(Workspace &w, F f)
{
    if (!f(w.verify_ev)) return false;
    for (Pipe &p : w.pipe)
        if (!f(p.join) || !f(p.long_done)) return false;
    return f(w.long_ev);
}

__global__ void wf_bind_stream() {}

// the pipelines' streams (created on first use, each bound to its hardware
// queue by an empty launch: the runtime maps a stream to a queue when it is
// first used, and streams created later share queues once the process has
// used its GPU_MAX_HW_QUEUES)
int ensure_streams(Workspace &w, int npipes)
{
    if (!w.streams_ok) {
        if (hipEventCreateWithFlags(&w.fork, hipEventDisableTiming) != hipSuccess) return -1;
        if (hipEventCreateWithFlags(&w.fin_ready, hipEventDisableTiming) != hipSuccess) return -1;
        if (!w.long_ev.create()) return -1;
        if (hipEventCreate(&w.ev0) != hipSuccess || hipEventCreate(&w.ev1) != hipSuccess) return -1;
        if (!w.verify_ev.create()) return -1;
        if (hipMalloc((void **)&w.verify_res, 64) != hipSuccess || hipMemset(w.verify_res, 0, 64) != hipSuccess)
            return -1;
        for (auto &e : w.chk_done)
            if (!e.create()) return -1;
        w.streams_ok = true;
    }
    for (int i = 0; i < npipes && i < WF_MAX_PIPES; ++i) {
        Pipe &p = w.pipe[i];
        if (p.stream) continue;
        if (hipStreamCreateWithFlags(&p.stream, hipStreamNonBlocking) != hipSuccess) return -1;
        if (hipHostMalloc((void **)&p.host_count, 64) != hipSuccess) return -1;
        if (!p.join.create() || !p.long_done.create()) return -1;
        if (hipEventCreateWithFlags(&p.fin_done, hipEventDisableTiming) != hipSuccess) return -1;
        for (auto &e : p.ev)
            if (hipEventCreate(&e) != hipSuccess) return -1;
        hipLaunchKernelGGL(wf_bind_stream, dim3(1), dim3(64), 0, p.stream);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(p.stream) != hipSuccess) return -1;
    }
    return 0;
}

int launch_drain(Workspace &w);
int flush_pending(Workspace &w);

#define WF_PROF_SLOTS 256 // profiled whole calls in flight before their spans are read back

// RtOptions.profile of a whole call: a span slot ({~0, 0}: the finisher's waves atomicMin their
// start and atomicMax their end into it), reset on the finisher's stream
int resolve_profiles(Workspace &w);
int prof_slot(Workspace &w, hipStream_t s, unsigned long long **span, int passes)
{
    if (!w.spans && hipMalloc((void **)&w.spans, 2 * sizeof(unsigned long long) * WF_PROF_SLOTS) != hipSuccess) {
        w.spans = nullptr;
        return -1;
    }
    if (w.prof_pending.size() >= WF_PROF_SLOTS && resolve_profiles(w) != 0) return -1;
    unsigned long long *p = w.spans + 2 * (size_t)(w.prof_seq % WF_PROF_SLOTS);
    if (hipMemsetD32Async((hipDeviceptr_t)p, (int)0xFFFFFFFF, 2, s) != hipSuccess ||
        hipMemsetAsync(p + 1, 0, 8, s) != hipSuccess)
        return -1;
    w.prof_pending.push_back({w.prof_seq, passes});
    ++w.prof_seq;
    *span = p;
    return 0;
}

#define WF_PROF_HISTORY 65536
void push_history(Workspace &w, const RtProfile &P)
{
    if (w.prof_hist.size() >= WF_PROF_HISTORY) // (drop the oldest half: amortised O(1))
        w.prof_hist.erase(w.prof_hist.begin(), w.prof_hist.begin() + WF_PROF_HISTORY / 2);
    w.prof_hist.push_back(P);
}

// the pending profiled whole calls' spans -> RtProfile records (waits for their finishers)
int resolve_profiles(Workspace &w)
{
    if (w.prof_pending.empty()) return 0;
    for (int pi : {0, 2})
        if (w.pipe[pi].stream && hipStreamSynchronize(w.pipe[pi].stream) != hipSuccess) return -1;
    std::vector<unsigned long long> sp(2 * WF_PROF_SLOTS);
    if (hipMemcpy(sp.data(), w.spans, sp.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    unsigned long long base = ~0ull; // (start_ms: relative to the earliest finisher start of the batch)
    for (const auto &q : w.prof_pending) base = std::min(base, sp[2 * (q.seq % WF_PROF_SLOTS)]);
    for (const auto &q : w.prof_pending) {
        const unsigned long long a = sp[2 * (q.seq % WF_PROF_SLOTS)], b = sp[2 * (q.seq % WF_PROF_SLOTS) + 1];
        RtProfile P{};
        P.start_ms = b > a ? (float)((double)(a - base) * 1e-5) : 0.0f;
        P.finish_launches = 1;
        P.pipelines = 1;
        P.finish_ms = b > a ? (float)((double)(b - a) * 1e-5) : 0.0f; // (s_memrealtime: 100 MHz)
        P.call_ms = P.finish_ms;
        push_history(w, P);
        w.prof = P;
    }
    w.prof_pending.clear();
    return 0;
}

// The blob's layout, every array named once: carve(p, n) gives p the next 256-byte-aligned offset and moves
// on by n entries of p's element type, or of `entry` bytes where an entry is not one element; zero() also
// lists the array among those that start as zeros.  Without a base it only sizes (the pointers come out null).
struct Carver {
    char *base;
    size_t off = 0;
    std::vector<std::pair<size_t, size_t>> zeroed; // {offset, bytes}
    template <typename T>
    void operator()(T *&p, size_t n, size_t entry = sizeof(T))
    {
        p = base ? (T *)(base + off) : nullptr;
        off += (n * entry + 255) & ~(size_t)255;
    }
    template <typename T>
    void zero(T *&p, size_t n, size_t entry = sizeof(T))
    {
        zeroed.emplace_back(off, n * entry);
        (*this)(p, n, entry);
    }
};

// lays the blob at `base` out into every pipeline's WfState and the workspace's own pointers (per-call
// fields zero: each launch sets its own); returns the pass: the blob's size (off) and its zeroed arrays
Carver carve_blob(Workspace &w, char *base, size_t slots, size_t spill_threads, int spill_pipes)
{
    Carver carve{base};
    const size_t ray = 2 * sizeof(RtF4); // a queued ray: {o.xyz, -}, {d.xyz, -}
    WfState st{};
    st.spill_threads = (int)spill_threads;
    st.long_cap = (uint32_t)slots;
    st.linger = WF_FIN_LINGER;
    // per pixel
    carve(st.passes_left, slots);
    carve(st.flags, slots);
    carve(st.T, slots);
    carve(st.L, slots);
    carve(st.cont, slots);
    carve(st.snorm, slots);
    carve(st.rp, slots);
    carve(st.light, slots);
    carve(st.ro, slots);
    carve(st.e_sh, slots);
    carve(st.e_ext, slots);
    carve.zero(st.pxo, slots); // no pixel out
    carve.zero(st.heavy, slots, 1); // no pixel heavy or listed yet
    carve.zero(st.listed, slots);
    carve(w.heavy_list, slots); // (WfState.heavy_list: set per call by launch_whole_now)
    carve.zero(st.heavy_n, 64);
    // long-path hand-off (shared by the pipelines), wf_long's stack-free wide traversal needs no spill
    carve(st.long_ent, slots);
    carve(st.long_ray, slots, ray);
    carve(st.long_ctr, 64);
    carve(st.ret_ring, slots);
    carve(st.ret_ctr, 64);
    uint32_t *ctl; // 256 control bytes: the producer words, the guard's counters (+64), the chain flag (+128)
    carve.zero(ctl, 64);
    if (ctl) {
        w.fin_live = ctl;
        w.chk_ctr = ctl + 16;
        st.chain_flag = ctl + 32;
    }
    // per pipeline (path lists sized for every pixel: a pipeline never holds
    // more; ray queues for two rays per path: a shadow and an extension ray)
    for (int i = 0; i < WF_MAX_PIPES; ++i) {
        WfState &ps = w.pipe[i].st = st;
        carve(ps.q_slot[0], slots);
        carve(ps.q_slot[1], slots);
        carve(ps.q_ray[0], 2 * slots, ray);
        carve(ps.q_ray[1], 2 * slots, ray);
        carve(ps.hits, 2 * slots);
        carve(ps.counts, 64);
        if (i < spill_pipes) carve(ps.spill, spill_threads * WF_SPILL_ENTRIES);
    }
    return carve;
}

int ensure(Workspace &w, size_t slots, int grid, int npipes)
{
    if (ensure_streams(w, npipes > WF_PIPES_DEFAULT ? npipes : WF_PIPES_DEFAULT) != 0) return -1;
    if (w.slots >= slots && w.grid >= grid && w.spill_pipes >= npipes) return 0;
    // traversal stack spill for the pipelines in use (at least the default 3)
    const int spill_pipes = npipes > WF_PIPES_DEFAULT ? npipes : WF_PIPES_DEFAULT;
    if (w.blob) {
        // (an open chain drained first: its wf_longs use the old blob until then)
        if (launch_drain(w) != 0) return -1;
        (void)hipDeviceSynchronize();
        (void)hipFree(w.blob);
    }
    w.blob = nullptr;
    w.slots = 0; // (nothing to reuse if the allocation below fails)
    const size_t spill_threads = (size_t)grid * WF_BLOCK;
    if (hipMalloc(&w.blob, carve_blob(w, nullptr, slots, spill_threads, spill_pipes).off) != hipSuccess) {
        w.blob = nullptr;
        return -1;
    }
    for (const auto &z : carve_blob(w, (char *)w.blob, slots, spill_threads, spill_pipes).zeroed)
        if (hipMemset((char *)w.blob + z.first, 0, z.second) != hipSuccess) return -1;
    w.chain_open = false;
    w.slots = slots;
    w.grid = grid;
    w.spill_pipes = spill_pipes;
    return 0;
}

float elapsed_ms(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f;
}

// the hand-off check (wf_verify) on `stream`, which has waited for all the workspace's work
int launch_verify(Workspace &w, hipStream_t stream)
{
    if (!w.verify_pending || !w.blob) return 0;
    w.verify_pending = false;
    const int blocks = (int)std::min<size_t>((w.slots + WF_BLOCK - 1) / WF_BLOCK, 1024);
    hipLaunchKernelGGL(wf_verify, dim3(blocks), dim3(WF_BLOCK), 0, stream, w.pipe[0].st, (uint32_t)w.slots,
                       w.verify_res, w.last.fr.dev_stats);
    // (every later launch on the workspace waits for it: join_all; and so does the host's read of its result)
    if (!w.verify_ev.record(stream)) return -1;
    w.verify_unread = true;
    return 0;
}

// `stream` waits for every call's device work on this workspace (the
// pipelines' last launches and every wf_long), an open chain drained first,
// and for the last hand-off check (which another stream may have run: it
// rewrites every ownership word); then the hand-off check runs on it
int join_all(Workspace &w, hipStream_t stream)
{
    if (launch_drain(w) != 0) return -1;
    if (!each_tail(w, [&](SerialEvent &e) { return e.wait_on(stream); })) return -1;
    return launch_verify(w, stream);
}

// RT_DEBUG_LONG_LOG: the deep samples wf_long logged (latest-ending, longest, per pixel), once the device is idle
int debug_long_log(unsigned long long *buf)
{
    (void)hipDeviceSynchronize();
    std::vector<unsigned long long> L(4 * 65536);
    (void)hipMemcpy(L.data(), buf, 8 * L.size(), hipMemcpyDeviceToHost);
    struct Rec { double start, end; unsigned long long bounces, slot; };
    std::vector<Rec> v;
    double last = 0;
    for (size_t e = 1; e < 65536; ++e)
        if (L[4 * e + 1]) {
            v.push_back({(L[4 * e] - L[0]) * 1e-5, (L[4 * e + 1] - L[0]) * 1e-5, L[4 * e + 2], L[4 * e + 3]});
            last = std::max(last, v.back().end);
        }
    std::sort(v.begin(), v.end(), [](const Rec &a, const Rec &b) { return a.end > b.end; });
    fprintf(stderr, "[wf long log] %zu deep samples, last end %.1f ms; latest 12 (start ms, end ms, bounces, us/bounce, slot):\n",
            v.size(), last);
    for (size_t i = 0; i < v.size() && i < 12; ++i)
        fprintf(stderr, "  %.1f %.1f %llu %.2f %llu\n", v[i].start, v[i].end, v[i].bounces,
                (v[i].end - v[i].start) * 1e3 / (double)(v[i].bounces ? v[i].bounces : 1), v[i].slot);
    std::sort(v.begin(), v.end(), [](const Rec &a, const Rec &b) { return a.bounces > b.bounces; });
    fprintf(stderr, "[wf long log] longest 8:\n");
    for (size_t i = 0; i < v.size() && i < 8; ++i)
        fprintf(stderr, "  %.1f %.1f %llu %.2f %llu\n", v[i].start, v[i].end, v[i].bounces,
                (v[i].end - v[i].start) * 1e3 / (double)(v[i].bounces ? v[i].bounces : 1), v[i].slot);
    // per pixel: deep samples, their summed time in wf_long, first claim and last end
    std::map<unsigned long long, Rec> px;
    std::map<unsigned long long, int> nd;
    for (const Rec &r : v) {
        auto it = px.find(r.slot);
        if (it == px.end()) {
            px[r.slot] = Rec{r.start, r.end, 0, (unsigned long long)0};
            it = px.find(r.slot);
        }
        it->second.start = std::min(it->second.start, r.start);
        it->second.end = std::max(it->second.end, r.end);
        it->second.slot += (unsigned long long)((r.end - r.start) * 1e3); // (us in wf_long)
        it->second.bounces += r.bounces;
        ++nd[r.slot];
    }
    std::vector<std::pair<unsigned long long, Rec>> pv(px.begin(), px.end());
    std::sort(pv.begin(), pv.end(), [](const auto &a, const auto &b) { return a.second.end > b.second.end; });
    fprintf(stderr, "[wf long log] %zu pixels; latest-ending 10 (slot, deep samples, bounces, ms in wf_long, first claim, last end):\n",
            pv.size());
    for (size_t i = 0; i < pv.size() && i < 10; ++i)
        fprintf(stderr, "  %llu %d %llu %.1f %.1f %.1f\n", pv[i].first, nd[pv[i].first], pv[i].second.bounces,
                pv[i].second.slot * 1e-3, pv[i].second.start, pv[i].second.end);
    return 0;
}

// The whole-call launch steps launch_whole_now and launch_drain share.
// The part of the finisher's WfState that follows from the call alone:
void whole_state(WfState &st, const WholeCall &c)
{
    st.long_depth = c.long_depth;
    st.long_return = c.long_depth > 0 ? 1 : 0;
    st.fresh = 1;
    st.debug_quit = (c.debug & RT_DEBUG_LONG_QUIT) ? 1 : 0;
    st.long_wide = c.sc.bvh_wide ? ((c.debug & RT_DEBUG_WIDE_CAP1) ? 2 : 1) : 0;
}

// the finisher on `s`.  Counting: the finisher's own work and wf_long's (RT_DEBUG_COUNT_LONG_ONLY: wf_long's
// alone, tools/wide_rounds.py); a grid of at most WF_FIN_SMALL_WAVES waves per SIMD takes the unspilled build
int launch_finisher(const Workspace &w, int fgrid, hipStream_t s, const WholeCall &c, const WfState &st, bool count)
{
    if (count && !(c.debug & RT_DEBUG_COUNT_LONG_ONLY))
        hipLaunchKernelGGL(wf_finish_bvh<true>, dim3(fgrid), dim3(WF_BLOCK), 0, s, c.sc, c.fr, c.cam, st, 0);
    else if (fgrid <= w.cus * WF_FIN_SMALL_WAVES)
        hipLaunchKernelGGL((wf_finish_bvh<false, 1>), dim3(fgrid), dim3(WF_BLOCK), 0, s, c.sc, c.fr, c.cam, st, 0);
    else hipLaunchKernelGGL(wf_finish_bvh<false>, dim3(fgrid), dim3(WF_BLOCK), 0, s, c.sc, c.fr, c.cam, st, 0);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the call's persistent wf_long on pipeline lp's stream, after event `after`
// (a counting call: wf_long counts its own work too — its bounded bounces' query rounds, wide nodes and
// tests, wide_bvh.h —, so that the device's work per deep bounce can be set against the host model's)
int launch_long(Pipe &lp, hipEvent_t after, const WholeCall &c, const WfState &st, bool count)
{
    if (hipStreamWaitEvent(lp.stream, after, 0) != hipSuccess) return -1;
    WF_LAUNCH_COUNT(count, wf_long, dim3(WF_LONG_BLOCKS), dim3(WF_BLOCK), lp.stream, c.sc, c.fr, c.cam, st, 1);
    return lp.long_done.record(lp.stream) ? 0 : -1;
}

// the guard's record buffer holds `cap` records per parity (regrown for more: after every wf_check that
// reads the old records)
int ensure_records(Workspace &w, uint32_t cap)
{
    if (cap <= w.chk_cap) return 0;
    if (w.chk) {
        if (hipDeviceSynchronize() != hipSuccess) return -1;
        (void)hipFree(w.chk);
        w.chk = nullptr;
        w.chk_cap = 0;
    }
    if (hipMalloc((void **)&w.chk, 2 * (size_t)cap * 3 * sizeof(RtF4)) != hipSuccess) {
        w.chk = nullptr;
        return -1;
    }
    w.chk_cap = cap;
    return 0;
}

// RT_DEBUG_CALL_LOG: the hand-off's counters once the finisher on `s` is done (`what`: the call or the drain)
void call_log(const char *what, unsigned long long seq, hipStream_t s, const WfState &st)
{
    (void)hipStreamSynchronize(s);
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    uint32_t lc[4] = {}, rc[7] = {};
    (void)hipMemcpy(lc, st.long_ctr, sizeof lc, hipMemcpyDeviceToHost);
    (void)hipMemcpy(rc, st.ret_ctr, sizeof rc, hipMemcpyDeviceToHost);
    fprintf(stderr,
            "[wf] %s %llu finisher done t %.4f; long entries %u claimed %u running %u; returns reserved %u claimed %u, "
            "finisher waves alive %u, pixels out %u; owed passes: most %u, pixels %u\n",
            what, seq, ts.tv_sec + ts.tv_nsec * 1e-9, lc[0], lc[1], lc[3], rc[0], rc[2], rc[1], rc[3], rc[5], rc[6]);
}

// The whole call in one persistent finisher (bounded traversal, the default):
// wf_finish_bvh takes the call's pixels itself (a lane claims a pixel, runs
// its passes to the end, one path at a time, and takes the next pixel), deep
// paths go to ONE persistent wf_long beside it, and wf_check re-traces the
// guard's sample after it.  Nothing here waits on the host: the call is
// enqueued and returns.
//
// RtOptions.overlap (chained calls): a call of the same frame as the previous
// overlapping call does not wait for that call at all.  Its finisher runs on
// the other of two finisher streams (pipelines 0 and 2), so it starts in the
// slots the previous finisher's tail frees, and a pixel still held there —
// by a previous finisher lane (BUSY) or by wf_long (OUT) — is owed this
// call's passes, which its holder runs before it lets go.  The caller's stream
// does not wait for the call either: rt_join and the library's readers of the
// frame do.  Results are bit-identical to unchained calls: a pixel's passes run
// in order whoever runs them.
int launch_whole_now(Workspace &w, const WholeCall &c)
{
    const RtDevScene &sc = c.sc;
    const RtDevFrame &fr = c.fr;
    const hipStream_t stream = c.stream;
    const int long_depth = c.long_depth, debug = c.debug;
    const uint32_t check_mask = c.check_mask;
    const size_t slots = (size_t)fr.width * fr.height;
    // a resetting call (sample_count 0) neither continues nor opens a chain: its reset of a pixel
    // must come before any later pass, and a chained lane may reach a pixel before it does
    const bool chain_asked = c.overlap; // (a chain's first, resetting call included: the next call's finisher follows it)
    const bool overlap = c.overlap && !fr.reset;
    // every wave slot at the finisher's occupancy (MI355X: 256 CUs x 4 SIMDs x 4 waves / 4 waves per
    // block = 1,024 blocks), the last WF_LONG_BLOCKS of them left to wf_long
    if (!w.cus) {
        hipDeviceProp_t prop;
        w.cus = hipGetDeviceProperties(&prop, c.dev) == hipSuccess && prop.multiProcessorCount > 0
                    ? prop.multiProcessorCount
                    : 256;
    }
    const int grid = w.cus * 4 * WF_FIN_BVH_WAVES / (WF_BLOCK / 64);
    const ChainKey key = chain_key(c);
    const bool chained = overlap && w.chain_open && !fr.reset && memcmp(&key, &w.key, sizeof key) == 0;
    // a fresh call: an open chain drained and every earlier call's work on the
    // workspace first (before a larger frame's workspace replaces the old one)
    if (!chained && join_all(w, stream) != 0) return -1;
    if (ensure(w, slots, grid, 1) != 0) return -1;
    // the finisher's stream (chained calls' finishers one after the other on it); its counters,
    // its stack spill area and its guard records go with it
    Pipe &pp = w.pipe[0];
    WfState st = pp.st;
    whole_state(st, c);
    const int long_return = st.long_return;
    st.fresh_n = (uint32_t)(((fr.width + 15) / 16) * ((fr.height + 15) / 16)) * 256u;
    st.linger = overlap ? 0ull : WF_FIN_LINGER;
    st.chk_mask = check_mask;
    // the guard's records per call parity (the call two later reuses them after this call's wf_check),
    // sized from the call's rays (wf_check_grid.h); wf_check's grid follows the same estimate
    const int par = (int)(w.call_seq & 1);
    unsigned long long chk_want = 0;
    if (ensure_records(w, wf_check_records(slots, (unsigned long long)fr.passes, check_mask,
                                           long_depth > 0 ? long_depth : RT_DEEP_PATH, WF_CHECK_CAP, &chk_want)) != 0)
        return -1;
    st.chk = check_mask == 0xFFFFFFFFu ? nullptr : w.chk + 3 * (size_t)w.chk_cap * (size_t)par;
    st.chk_cap = w.chk_cap;
    st.chk_ctr = w.chk_ctr + par;
    st.chk_fault = ((debug & RT_DEBUG_CHECK_FAULT) ? 1 : 0) | ((debug & RT_DEBUG_BUDGET1) ? WF_DEBUG_BUDGET1 : 0);
    // debug (RT_DEBUG_LONG_LOG): every deep sample's claim / end time and bounces
    if ((debug & RT_DEBUG_LONG_LOG) && !w.long_log_buf &&
        hipMalloc((void **)&w.long_log_buf, 8 * 4 * 65536) != hipSuccess) {
        w.long_log_buf = nullptr;
        return -1;
    }
    unsigned long long *const long_log_buf = w.long_log_buf;
    st.long_log = (debug & RT_DEBUG_LONG_LOG) ? long_log_buf : nullptr;
    // the finisher: every wave slot but wf_long's blocks, at most one lane per pixel
    int fgrid = (int)((slots + WF_BLOCK - 1) / WF_BLOCK);
    const int fmax = long_return ? grid - WF_LONG_BLOCKS : grid;
    fgrid = fgrid > fmax ? fmax : fgrid;
    const uint32_t k = (uint32_t)(w.call_seq % 8);
    st.fin_live = long_return ? w.fin_live + k : nullptr;
    st.call_id = (uint32_t)w.call_seq + 1u;
    if (!chained) {
        // the hand-off state from zero (nothing of it is in flight now; a ring a wf_long closed reopens)
        if (long_return) {
            // (the rings' whole capacity: the workspace may be sized for an earlier, larger frame, and a
            // stale tag beyond this frame's pixel count would look published to wf_long / the finishers)
            if (hipMemsetAsync(st.long_ctr, 0, 256, stream) != hipSuccess) return -1;
            if (hipMemsetAsync(st.long_ent, 0, (size_t)st.long_cap * 8, stream) != hipSuccess) return -1;
            if (hipMemsetAsync(st.ret_ring, 0, (size_t)st.long_cap * 8, stream) != hipSuccess) return -1;
            if (hipMemsetAsync(st.ret_ctr, 0, 256, stream) != hipSuccess) return -1;
        }
        if (st.long_log && hipMemsetAsync(long_log_buf, 0, 8 * 4 * 65536, stream) != hipSuccess) return -1;
    }
    ++w.call_seq;
    // fork: the finisher's stream starts after the caller's stream
    const hipStream_t s = pp.stream;
    if (hipEventRecord(w.fork, stream) != hipSuccess || hipStreamWaitEvent(s, w.fork, 0) != hipSuccess) return -1;
    if (hipMemsetAsync(st.counts, 0, 256, s) != hipSuccess) return -1;
    // (the producers' word: the finisher's wave count, no wave started yet)
    if (st.fin_live && hipMemsetD32Async((hipDeviceptr_t)st.fin_live, (int)(fgrid * (WF_BLOCK / 64)), 1, s) != hipSuccess)
        return -1;
    if (st.chk) { // (this parity's records: after the wf_check that last read them)
        if (!w.chk_done[par].wait_on(s)) return -1;
        if (hipMemsetAsync(st.chk_ctr, 0, 4, s) != hipSuccess) return -1;
    }
    if (long_return && hipMemsetD32Async((hipDeviceptr_t)st.chain_flag, overlap ? 1 : 0, 1, s) != hipSuccess) return -1;
    // RtOptions.profile: the finisher's span on the device (first wave start, last wave end)
    st.span = nullptr;
    if (c.prof && prof_slot(w, s, &st.span, fr.passes) != 0) return -1;
    // heavy pixels first (wf_heavy_list): listed and tagged with this call before the finisher
    st.heavy_list = nullptr;
    if (long_return && w.heavy_list && WF_HEAVY_FIRST) {
        st.heavy_list = w.heavy_list;
        if (hipMemsetAsync(st.heavy_n, 0, 4, s) != hipSuccess) return -1;
        // two classes: pixels handed over WF_HEAVY_SPLIT+ times so far, then the others
        hipLaunchKernelGGL(wf_heavy_list, dim3(WF_HEAVY_BLOCKS), dim3(WF_BLOCK), 0, s, fr, st, st.call_id,
                           (uint32_t)WF_HEAVY_SPLIT, 256u);
        hipLaunchKernelGGL(wf_heavy_list, dim3(WF_HEAVY_BLOCKS), dim3(WF_BLOCK), 0, s, fr, st, st.call_id, 1u,
                           (uint32_t)WF_HEAVY_SPLIT);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    if (hipEventRecord(w.fin_ready, s) != hipSuccess) return -1;
    Pipe *lp = long_return ? &w.pipe[1] : nullptr;
    // wf_long on pipeline 1's stream, after the finisher's set-up.  Normally it starts beside the
    // finisher; nothing relies on that (serialised dispatch runs either alone, in either order:
    // see the cross-kernel waits at WF_FIN_STARTED).  Debug: force one order —
    // RT_DEBUG_SERIAL_LONG_FIRST runs wf_long to its end before the finisher starts,
    // RT_DEBUG_SERIAL_FIN_FIRST the finisher to its end before wf_long starts
    const bool long_first = lp && (debug & RT_DEBUG_SERIAL_LONG_FIRST);
    const bool fin_first = lp && !long_first && (debug & RT_DEBUG_SERIAL_FIN_FIRST);
    const hipEvent_t long_after = fin_first ? pp.fin_done : w.fin_ready;
    if (long_first &&
        (launch_long(*lp, long_after, c, st, c.count) != 0 || !lp->long_done.wait_on(s)))
        return -1;
    if (launch_finisher(w, fgrid, s, c, st, c.count) != 0) return -1;
    if (hipEventRecord(pp.fin_done, s) != hipSuccess) return -1;
    if (lp && !long_first && launch_long(*lp, long_after, c, st, c.count) != 0) return -1;
    if (st.chk) {
        // the guard's re-traces on pipeline 2's stream after the finisher, beside whatever follows it on
        // pipeline 0 (the next call's finisher, a chain's drain); its KD stacks in pipeline 2's spill area
        Pipe &cp = w.pipe[2];
        WfState cs = st;
        cs.spill = cp.st.spill;
        if (!cs.spill) return -1;
        if (hipStreamWaitEvent(cp.stream, pp.fin_done, 0) != hipSuccess) return -1;
        // Its grid: WF_CHECK_BLOCKS beside a chain's next finisher; a call that overlaps nothing runs the check
        // alone on the chip, inside the caller's wait, and gets a lane per record it may hold.  At most
        // spill_threads / WF_BLOCK blocks either way: a lane's KD stack spills to cs.spill[gtid + k * spill_threads],
        // so a lane at or past spill_threads would write into its neighbours' entries and past the area's end
        const int cgrid = wf_check_grid(chain_asked, chk_want, cs.chk_cap, cs.spill_threads, WF_BLOCK, WF_CHECK_BLOCKS);
        if (cgrid < 1 || (size_t)cgrid * WF_BLOCK > (size_t)cs.spill_threads) {
            fprintf(stderr, "[wf] wf_check grid %d blocks exceeds the spill area's %d lanes\n", cgrid, cs.spill_threads);
            return -1;
        }
        hipLaunchKernelGGL(wf_check, dim3(cgrid), dim3(WF_BLOCK), 0, cp.stream, sc, cs, fr.dev_stats);
        if (!w.chk_done[par].record(cp.stream) || !cp.join.record(cp.stream)) return -1;
    }
    if (!pp.join.record(s)) return -1;
    // join: unless the call overlaps the next one, the caller's stream continues after the
    // finisher and after its wf_long (the guard's wf_check touches no frame data: its statistics
    // are read by rt_deviation_stats, which joins it)
    if (!overlap) {
        if (!pp.join.wait_on(stream)) return -1;
        if (lp && !lp->long_done.wait_on(stream)) return -1;
    }
    w.chain_open = overlap && long_return;
    w.verify_pending = w.verify_pending || long_return;
    w.key = key;
    w.last = c;
    w.last.fr.reset = 0;
    if (debug & RT_DEBUG_CALL_LOG) call_log(chained ? "chained call" : "call", w.call_seq, s, st);
    if (st.long_log && !overlap) return debug_long_log(long_log_buf);
    return 0;
}

// the pending batch of coalesced chained calls, launched as one chained call
int flush_pending(Workspace &w)
{
    if (!w.pend.on) return 0;
    WholeCall c = w.pend.call;
    w.pend.on = false;
    c.overlap = true;
    c.count = false;
    return launch_whole_now(w, c);
}

// rt_render's whole call (see launch_whole_now), with small chained calls
// coalesced (Pending; coalesce <= 0: off)
int launch_whole(Workspace &w, const WholeCall &c, int coalesce)
{
    // (debug diagnostics per call and forced dispatch orders are per launch: never coalesced)
    const bool can = c.overlap && !c.fr.reset && !c.count && coalesce > 0 && !c.fr.wave_times &&
                     !(c.debug & (RT_DEBUG_CALL_LOG | RT_DEBUG_LONG_LOG | RT_DEBUG_SERIAL_LONG_FIRST |
                                  RT_DEBUG_SERIAL_FIN_FIRST));
    if (w.pend.on) {
        if (can && coalesces(w.pend, c, chain_key(c))) {
            w.pend.call.fr.passes += c.fr.passes;
            return w.pend.call.fr.passes < coalesce ? 0 : flush_pending(w);
        }
        if (flush_pending(w) != 0) return -1;
    }
    if (can && c.fr.passes < coalesce) {
        w.pend.on = true;
        w.pend.call = c;
        w.pend.key = chain_key(c);
        return 0;
    }
    return launch_whole_now(w, c);
}

// The drain of an open chain (join_all, i.e. rt_join and every reader of the
// frame, or the next call that does not continue it): a chained call's
// finisher leaves pixels wf_long hands back after its pixel list ran out to
// the next call; here one more finisher with no pixels of its own takes them,
// runs their remaining passes (handing deep samples to its own wf_long again)
// and lingers while any pixel is still out.  Enqueued on pipeline 0 after the
// chain's last finishers on both finisher streams; join_all then waits for it
// and every wf_long.
int launch_drain(Workspace &w)
{
    if (flush_pending(w) != 0) return -1; // (coalesced chained calls: launched, then drained)
    if (!w.chain_open) return 0;
    w.chain_open = false;
    const WholeCall &c = w.last; // (a chained call with the hand-off: its long_return is 1)
    const size_t slots = (size_t)c.fr.width * c.fr.height;
    Pipe &pp = w.pipe[0];
    WfState st = pp.st;
    whole_state(st, c);
    st.fresh_n = 0; // (no pixels of its own)
    st.span = nullptr;
    st.linger = WF_FIN_LINGER; // (a pixel still out after it: wf_long runs it to the end)
    st.chk = nullptr;
    st.chk_mask = 0;
    st.chk_ctr = w.chk_ctr;
    st.chk_fault = 0;
    st.long_log = nullptr;
    int fgrid = (int)((slots + WF_BLOCK - 1) / WF_BLOCK);
    fgrid = fgrid > w.grid - WF_LONG_BLOCKS ? w.grid - WF_LONG_BLOCKS : fgrid;
    st.fin_live = w.fin_live + (uint32_t)(w.call_seq % 8);
    ++w.call_seq;
    const hipStream_t s = pp.stream;
    // no pixels (counts[4] = 0 of fresh_n 0), no linger seat taken yet
    if (hipMemsetAsync(st.counts, 0, 256, s) != hipSuccess) return -1;
    if (hipMemsetAsync(st.ret_ctr + 4, 0, 4, s) != hipSuccess) return -1;
    if (hipMemsetAsync(st.chain_flag, 0, 4, s) != hipSuccess) return -1; // the chain's wf_longs may leave once idle
    if (hipMemsetD32Async((hipDeviceptr_t)st.fin_live, (int)(fgrid * (WF_BLOCK / 64)), 1, s) != hipSuccess) return -1;
    if (hipEventRecord(w.fin_ready, s) != hipSuccess) return -1;
    if (launch_finisher(w, fgrid, s, c, st, false) != 0) return -1;
    if (launch_long(w.pipe[1], w.fin_ready, c, st, false) != 0) return -1;
    if (!pp.join.record(s)) return -1;
    w.verify_pending = true;
    if (c.debug & RT_DEBUG_CALL_LOG) call_log("drain", w.call_seq, s, st);
    return 0;
}

// The queue mode of rt_render (every wavefront call that is not a whole call: counting calls, the KD traversal,
// kernel variants 2 and 3, RtOptions.wf_tail): npipes pipelines of trace / shade iterations, one host thread each,
// then a finisher per pipeline; deep paths go to wf_long slices on the caller's stream
int launch_queue(Workspace &w, int dev, const RtDevScene &sc, const RtDevFrame &fr, const RtDevCamera &cam,
                 const RtOptions &o, int trace_kind, bool bounded, int long_depth)
{
    const hipStream_t stream = (hipStream_t)o.stream;
    const size_t slots = (size_t)fr.width * fr.height;
    const bool count = fr.counters != nullptr;
    const int debug = o.debug;
    // persistent-ish grid for trace/shade (grid-stride over the queue).  512
    // blocks = 2,048 waves = a third of the chip's 6,144 wave slots at the
    // trace kernel's 6 waves/SIMD: the 3 pipelines' launches share the chip,
    // and a launch's ~465k rays are ~3.5 per lane, so the lanes stay busy past
    // the launch's first round of rays (1,536 blocks: ~1.2 rays per lane, most
    // of the launch was its tail).  Measured 512 / 704 / 1,536: 37.5 / 37.6 /
    // 33.1 Msamples/s on room2m 1080p (tools/gpu_sweep.sh, profiles/r02).
    const int grid = 512;
    const int tgrid = grid * (WF_BLOCK / WF_TBLOCK); // the same waves in WF_TBLOCK-thread blocks
    // wf_shade: half the trace grid (~2 paths per lane per launch).  Measured
    // per 256-pass room2m call (2 rounds each): 64 / 128 / 256 / 384 / 512 /
    // 1,024 / 2,048 blocks: 13.27 / 12.82 / 12.78 / 12.78 / 12.87 / 13.01 /
    // 13.21 s
    const int sgrid = tgrid / 2 > 16 ? tgrid / 2 : 16;
    const bool prof = o.profile != 0;
    const int tiles = ((fr.width + 15) / 16) * ((fr.height + 15) / 16);
    int npipes = o.wf_pipelines > 0 ? o.wf_pipelines : WF_PIPES_DEFAULT;
    npipes = npipes > WF_MAX_PIPES ? WF_MAX_PIPES : npipes;
    npipes = npipes > tiles ? tiles : npipes;
    if (ensure(w, slots, grid, npipes) != 0) return -1;
    // below this many live paths the rest of the call runs in one finisher launch
    const uint32_t tail = o.wf_tail > 0 ? (uint32_t)o.wf_tail : WF_TAIL_DEFAULT;
    // the cooperative finisher runs on at most this many waves (up to 64 paths in flight each)
    // (small trees: rays are short, so more paths per finisher wave keep its
    // cooperative rounds full — the 36-triangle Cornell box at 256x256 runs
    // 124 vs 91 Msamples/s with 512 waves; room2m is flat from 1024 to 6144)
    const uint32_t finish_waves = o.wf_finish_waves > 0 ? (uint32_t)o.wf_finish_waves
                                  : sc.index_count >= WF_FIN_WIDE_MIN_ENTRIES ? WF_FINISH_WAVES_DEFAULT
                                                                              : WF_FINISH_WAVES_SMALL;
    // cooperative traversal: node fetches per descent round, pending lanes before a leaf test
    const int cap = o.wf_descent_cap > 0 ? o.wf_descent_cap : WF_DESCENT_CAP_DEFAULT;
    const int postpone = o.wf_postpone > 0 ? (o.wf_postpone > 64 ? 64 : o.wf_postpone) : WF_POSTPONE_DEFAULT;
    // trace launches: once the queue is empty, a wave with at most this many rays left finishes them wide;
    // finisher: a wave with at most this many live rays traces them one by one with all lanes
    const int wide_lanes = o.wf_wide < 0 ? 0 : (o.wf_wide > 0 ? (o.wf_wide > 64 ? 64 : o.wf_wide) : WF_WIDE_TAIL_LANES);
    // (finisher: tracing several rays one after the other with all lanes pays off
    // when a ray visits hundreds of nodes — large trees; on a small tree, e.g.
    // the 36-triangle Cornell box, a cooperative round of a few lanes is
    // cheaper, and only a lone ray goes wide.  Measured: room2m / cornell_blob
    // finisher time -18 % / -30 % at 32, the Cornell box 2x slower)
    const int wide = sc.index_count >= WF_FIN_WIDE_MIN_ENTRIES ? wide_lanes : (wide_lanes > 0 ? 1 : 0);
    const bool trace_iters = (debug & RT_DEBUG_CALL_LOG) != 0; // per-iteration queue sizes
    for (int pi = 0; pi < WF_MAX_PIPES; ++pi) {
        WfState &st = w.pipe[pi].st;
        st.long_depth = long_depth;
        st.long_return = 0;
        st.fin_live = nullptr;
        st.long_log = nullptr;
    }
    const WfState lst = w.pipe[0].st;

    // the workspace (per-pixel path state, long-path hand-off) is shared by every
    // call on this device: a call must not start before every earlier call's
    // pipelines and wf_long work are done (pixels may move to another pipeline
    // while the previous call's finisher still writes their path state)
    if (join_all(w, stream) != 0) return -1;
    w.chain_open = false;
    if (long_depth > 0) {
        // (the ring from zero — its whole capacity, see launch_whole; a pixel is handed over at most once
        // per call here)
        if (hipMemsetAsync(lst.long_ent, 0, (size_t)lst.long_cap * 8, stream) != hipSuccess) return -1;
        if (hipMemsetAsync(lst.long_ctr, 0, 256, stream) != hipSuccess) return -1;
    }
    // fork: every pipeline stream starts after the caller's stream
    if (hipEventRecord(w.fork, stream) != hipSuccess) return -1;
    if (prof && hipEventRecord(w.ev0, stream) != hipSuccess) return -1;
    std::mutex long_mu;
    bool long_final = false;
    int n_slices = 0; // (debug output)
    // launches a wf_long slice on the caller's stream unless the previous one
    // is still running; the final slice (every producer done) is queued after it
    auto kick_long = [&](bool final) -> int {
        if (long_depth <= 0) return 0;
        std::lock_guard<std::mutex> g(long_mu);
        if (long_final) return 0;
        if (!final) {
            const hipError_t q = w.long_ev.query();
            if (q == hipErrorNotReady) return 0;
            if (q != hipSuccess) return -1;
        }
        const int fin = final ? 1 : 0;
        WF_LAUNCH_COUNT(count, wf_long, dim3(WF_LONG_BLOCKS), dim3(WF_BLOCK), stream, sc, fr, cam, lst, fin);
        if (!w.long_ev.record(stream)) return -1;
        long_final = final;
        ++n_slices;
        return 0;
    };
    std::atomic<int> producing(npipes);
    bool produced_done[WF_MAX_PIPES] = {};
    // a pipeline's queue iterations are over (every shade launch that could
    // publish has completed: the host read its queue size): the last one
    // queues the final wf_long slice
    auto producer_done = [&](int pi) -> int {
        if (produced_done[pi]) return 0;
        produced_done[pi] = true;
        if (producing.fetch_sub(1) != 1) return 0;
        return kick_long(true);
    };

    auto run_pipe = [&](int pi) -> int {
        if (hipSetDevice(dev) != hipSuccess) return -1;
        Pipe &pp = w.pipe[pi];
        pp.trace_iv.clear();
        WfState &st = pp.st;
        hipStream_t s = pp.stream;
        if (hipStreamWaitEvent(s, w.fork, 0) != hipSuccess) return -1;
        RtProfile P{};
        auto mark = [&](int i) { return !prof || hipEventRecord(pp.ev[i], s) == hipSuccess; };
        if (!mark(0)) return -1;
        if (hipMemsetAsync(st.counts, 0, 256, s) != hipSuccess) return -1;
        WF_LAUNCH_COUNT(count, wf_start, dim3(tiles), dim3(WF_BLOCK), s, fr, cam, st, pi, npipes);
        if (!mark(1)) return -1;
        // run the `live` paths of queue qq to the end of the call in the finisher
        auto finish = [&](int qq, uint32_t live) -> int {
            if (!mark(2)) return -1;
            if (bounded) {
                // one path per lane (lanes refill from the list), within the spill area (grid blocks)
                int fgrid = (int)((live + WF_BLOCK - 1) / WF_BLOCK);
                fgrid = fgrid > grid ? grid : fgrid;
                if (hipMemsetAsync(st.counts + 4, 0, 4, s) != hipSuccess) return -1;
                WF_LAUNCH_COUNT(count, wf_finish_bvh, dim3(fgrid), dim3(WF_BLOCK), s, sc, fr, cam, st, qq);
            } else if (trace_kind == 1) {
                // paths per wave: spread over up to finish_waves waves, within the spill area (grid * WF_BLOCK threads)
                const uint32_t max_waves = (uint32_t)grid * (WF_BLOCK / 64);
                uint32_t ppw = (live + finish_waves - 1) / finish_waves;
                ppw = ppw < 1 ? 1 : (ppw > 64 ? 64 : ppw);
                uint32_t waves = (live + ppw - 1) / ppw;
                if (waves > finish_waves) waves = finish_waves;
                if (waves > max_waves) waves = max_waves; // persistent: lanes fetch paths until the queue is empty
                if (hipMemsetAsync(st.counts + 4, 0, 4, s) != hipSuccess) return -1;
                const int fgrid = (int)((waves + WF_BLOCK / 64 - 1) / (WF_BLOCK / 64));
                WF_LAUNCH_COUNT(count, wf_finish_coop, dim3(fgrid), dim3(WF_BLOCK), s, sc, fr, cam, st, qq, (int)ppw, cap,
                                postpone, wide);
            } else {
                // grid-stride loop: at most `grid` blocks, so gtid stays inside the spill area
                // (sized for grid * WF_BLOCK threads)
                int fgrid = (int)((live + WF_BLOCK - 1) / WF_BLOCK);
                fgrid = fgrid > grid ? grid : fgrid;
                WF_LAUNCH_COUNT(count, wf_finish, dim3(fgrid), dim3(WF_BLOCK), s, sc, fr, cam, st, qq);
            }
            if (hipGetLastError() != hipSuccess || !mark(3)) return -1;
            P.finish_launches = 1;
            return 0;
        };
        int rc = 0;
        // the bounded finisher publishes deep paths to wf_long too: its pipeline
        // is a producer until the finisher is done (meanwhile wf_long slices are
        // kicked as they end; the last producer queues the final slice)
        auto finish_and_release = [&](int qq, uint32_t live) -> int {
            const bool publishes = bounded && long_depth > 0;
            if (!publishes && producer_done(pi) != 0) return -1;
            if (finish(qq, live) != 0) return -1;
            if (!publishes) return 0;
            if (hipEventRecord(pp.fin_done, s) != hipSuccess) return -1;
            while (true) {
                const hipError_t e = hipEventQuery(pp.fin_done);
                if (e == hipSuccess) break;
                if (e != hipErrorNotReady) return -1;
                if (kick_long(false) != 0) return -1;
                std::this_thread::sleep_for(std::chrono::microseconds(200));
            }
            return producer_done(pi);
        };
        for (int it = 0;; ++it) {
            const int q = it & 1;
            if (hipMemsetAsync(st.counts + (q ^ 1), 0, 4, s) != hipSuccess) return -1;     // next ray queue
            if (hipMemsetAsync(st.counts + 6 + (q ^ 1), 0, 4, s) != hipSuccess) return -1; // next path list
            if (hipMemsetAsync(st.counts + 2 + q, 0, 4, s) != hipSuccess) return -1; // fetch cursor
            if (!mark(4)) return -1;
            // (a call counts iff fr.counters is set: the plain arms' counters are null, whichever way each was written)
            if (bounded) {
                WF_LAUNCH_COUNT(count, wf_trace_bvh_dyn, dim3(grid), dim3(WF_BLOCK), s, sc, st, q, fr.counters,
                                WF_BVH_DYN_CAP);
            } else if (trace_kind == 1) {
                const int li = it * npipes + pi;
                unsigned long long *tl = fr.wave_times && li < WF_TIMELINE_LAUNCHES ? fr.wave_times + 3 * li : nullptr;
                WF_LAUNCH_COUNT(count, wf_trace_coop, dim3(tgrid), dim3(WF_TBLOCK), s, sc, st, q, fr.counters, cap, postpone,
                                wide_lanes, tl);
            } else if (trace_kind == 3) {
                WF_LAUNCH_COUNT(count, wf_trace_dyn, dim3(grid), dim3(WF_BLOCK), s, sc, st, q, fr.counters);
            } else {
                WF_LAUNCH_COUNT(count, wf_trace, dim3(grid), dim3(WF_BLOCK), s, sc, st, q, fr.counters);
            }
            if (!mark(5)) return -1;
            WF_LAUNCH_COUNT(count, wf_shade, dim3(sgrid), dim3(WF_TBLOCK), s, sc, fr, cam, st, q);
            if (hipGetLastError() != hipSuccess) return -1;
            if (!mark(2)) return -1;
            if (hipMemcpyAsync(pp.host_count, st.counts, 32, hipMemcpyDeviceToHost, s) != hipSuccess)
                return -1;
            if (hipStreamSynchronize(s) != hipSuccess) return -1;
            const uint32_t live = pp.host_count[6 + (q ^ 1)]; // paths with rays in the next queue
            P.iterations = it + 1;
            if (prof) {
                P.trace_ms += elapsed_ms(pp.ev[4], pp.ev[5]);
                P.shade_ms += elapsed_ms(pp.ev[5], pp.ev[2]);
                pp.trace_iv.emplace_back(elapsed_ms(w.ev0, pp.ev[4]), elapsed_ms(w.ev0, pp.ev[5]));
            }
            if (trace_iters) {
                timespec ts;
                clock_gettime(CLOCK_MONOTONIC, &ts);
                fprintf(stderr, "[wf] pipe %d it %d live %u t %.4f\n", pi, it, live, ts.tv_sec + ts.tv_nsec * 1e-9);
            }
            if (kick_long(false) != 0) return -1; // paths published by this shade launch
            if (live == 0 || live < tail) {
                if (live != 0) rc = finish_and_release(q ^ 1, live);
                else if (producer_done(pi) != 0) return -1;
                break;
            }
        }
        if (rc != 0) return rc;
        if (!pp.join.record(s)) return -1;
        if (prof) {
            if (!mark(4) || hipEventSynchronize(pp.ev[4]) != hipSuccess) return -1;
            P.trace_launches = P.shade_launches = P.iterations;
            P.start_ms = elapsed_ms(pp.ev[0], pp.ev[1]);
            if (P.finish_launches) P.finish_ms = elapsed_ms(pp.ev[2], pp.ev[3]);
            P.call_ms = elapsed_ms(pp.ev[0], pp.ev[4]);
        }
        pp.prof = P;
        return 0;
    };

    int rcs[WF_MAX_PIPES] = {};
    std::thread threads[WF_MAX_PIPES];
    for (int pi = 1; pi < npipes; ++pi) threads[pi] = std::thread([&, pi] { rcs[pi] = run_pipe(pi); });
    rcs[0] = run_pipe(0);
    for (int pi = 1; pi < npipes; ++pi) threads[pi].join();
    if (!long_final) (void)kick_long(true); // a pipeline failed early: drain the published paths anyway
    if (trace_iters) {
        (void)hipStreamSynchronize(stream);
        uint32_t lc[4] = {};
        (void)hipMemcpy(lc, lst.long_ctr, sizeof lc, hipMemcpyDeviceToHost);
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        fprintf(stderr, "[wf] long paths %u claimed %u running %u; slices %d; caller stream done t %.4f\n", lc[0],
                lc[1], lc[3], n_slices, ts.tv_sec + ts.tv_nsec * 1e-9);
    }
    for (int pi = 0; pi < npipes; ++pi)
        if (rcs[pi] != 0) return rcs[pi];
    // join: the caller's stream continues after every pipeline
    for (int pi = 0; pi < npipes; ++pi)
        if (!w.pipe[pi].join.wait_on(stream)) return -1;
    if (prof) {
        RtProfile P{};
        for (int pi = 0; pi < npipes; ++pi) { // kernel times summed over the (concurrent) pipelines
            const RtProfile &q = w.pipe[pi].prof;
            P.iterations += q.iterations;
            P.trace_launches += q.trace_launches;
            P.shade_launches += q.shade_launches;
            P.finish_launches += q.finish_launches;
            P.start_ms += q.start_ms;
            P.trace_ms += q.trace_ms;
            P.shade_ms += q.shade_ms;
            P.finish_ms += q.finish_ms;
        }
        if (hipEventRecord(w.ev1, stream) != hipSuccess || hipEventSynchronize(w.ev1) != hipSuccess) return -1;
        P.call_ms = elapsed_ms(w.ev0, w.ev1); // wall time of the call
        std::vector<std::pair<float, float>> iv; // union of the pipelines' trace launch intervals
        for (int pi = 0; pi < npipes; ++pi) iv.insert(iv.end(), w.pipe[pi].trace_iv.begin(), w.pipe[pi].trace_iv.end());
        std::sort(iv.begin(), iv.end());
        float lo = 0.0f, hi = -1.0f;
        for (const auto &x : iv) {
            if (x.first > hi) {
                if (hi > lo) P.trace_union_ms += hi - lo;
                lo = x.first;
                hi = x.second;
            } else if (x.second > hi) {
                hi = x.second;
            }
        }
        if (hi > lo) P.trace_union_ms += hi - lo;
        P.pipelines = npipes;
        w.prof = P;
        push_history(w, P);
    }
    return 0;
}

} // namespace

// rt_set_device: the default pipelines' streams take their hardware queues
// before anything else in the process (RCCL's streams in a multi-GPU run)
int rt_wavefront_device_init()
{
    rt_register_shutdown();
    std::lock_guard<std::mutex> g(g_ws.mu);
    Workspace *w = g_ws.current();
    return w ? ensure_streams(*w, WF_PIPES_DEFAULT) : -1;
}

static thread_local char g_incomplete[256];

// the last RT_WAVEFRONT_INCOMPLETE's description (abi.hip: rt_last_error)
const char *rt_wavefront_incomplete_msg() { return g_incomplete; }

// rt_join: `stream` (NULL: the host) waits for every rt_render's device work
// on the current device, chained calls' deep-path tails included, and for the
// hand-off check after them.  A host join returns RT_WAVEFRONT_INCOMPLETE if
// that check, or one enqueued by an earlier stream join, found pixels that
// never came back from wf_long.  consume = 0 (the library's joins that do
// not report: rt_deviation_stats, buffer and scene teardown) leaves such a
// result for the next reporting join: the incomplete status is sticky.
int rt_wavefront_join(void *stream, int consume)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    std::lock_guard<std::mutex> g(g_ws.mu);
    Workspace *w = g_ws.find(); // (a device that never rendered: nothing to join, and nothing is made)
    if (!w) return 0;
    if (stream) return join_all(*w, (hipStream_t)stream);
    if (launch_drain(*w) != 0) return -1;
    if (!each_tail(*w, [](SerialEvent &e) { return e.wait_host(); })) return -1;
    // the hand-off check on pipeline 0's stream (idle: everything above is done)
    if (launch_verify(*w, w->pipe[0].stream) != 0) return -1;
    // (the last check may have run on a caller's stream: its result is read after it)
    if (!w->verify_ev.wait_host()) return -1;
    if (!w->verify_unread) return 0;
    uint32_t r[5] = {};
    if (hipMemcpy(r, w->verify_res, sizeof r, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (!consume) return 0;
    w->verify_unread = false;
    if (hipMemset(w->verify_res, 0, sizeof r) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    if (r[0] | r[1] | r[2] | r[3] | r[4]) {
        snprintf(g_incomplete, sizeof g_incomplete,
                 "%u pixels stranded in the deep-path hand-off (pixels out %u, returns unclaimed %u, hand-offs "
                 "unclaimed %u, finisher waves registered %u): the frame misses passes; RtDeviations counts it",
                 r[0], r[1], r[2], r[3], r[4]);
        return RT_WAVEFRONT_INCOMPLETE;
    }
    return 0;
}

// rt_shutdown: every stream, event and device blob of every device's
// workspace, after its device work is done: the blobs, the events, then each
// pipeline's stream in reverse creation order
void rt_wavefront_shutdown()
{
    g_ws.shutdown([](Workspace &w) {
        if (w.blob) (void)launch_drain(w); // (an open chain's wf_longs leave only after its drain)
        (void)hipDeviceSynchronize();
        for (void *p : {w.blob, (void *)w.chk, (void *)w.verify_res, (void *)w.long_log_buf, (void *)w.spans})
            if (p) (void)hipFree(p);
        (void)each_tail(w, [](SerialEvent &e) { return e.destroy(), true; });
        for (SerialEvent &e : w.chk_done) e.destroy();
        for (int i = WF_MAX_PIPES - 1; i >= 0; --i) {
            Pipe &p = w.pipe[i];
            for (hipEvent_t e : {p.ev[5], p.ev[4], p.ev[3], p.ev[2], p.ev[1], p.ev[0], p.fin_done})
                if (e) (void)hipEventDestroy(e);
            if (p.host_count) (void)hipHostFree(p.host_count);
            if (p.stream) (void)hipStreamDestroy(p.stream);
        }
        for (hipEvent_t e : {w.ev1, w.ev0, w.fin_ready, w.fork})
            if (e) (void)hipEventDestroy(e);
    });
}

extern "C" int rt_last_profile(RtProfile *out)
{
    if (!out) return RT_E_INVALID;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return RT_E_HIP;
    std::lock_guard<std::mutex> g(g_ws.mu);
    Workspace *w = g_ws.find();
    if (!w) {
        *out = RtProfile{};
        return RT_OK;
    }
    if (flush_pending(*w) != 0 || resolve_profiles(*w) != 0) return RT_E_HIP;
    *out = w->prof;
    return RT_OK;
}

extern "C" int rt_profile_history(RtProfile *out, int cap, int *count, int reset)
{
    if ((!out && cap > 0) || cap < 0 || !count) return RT_E_INVALID;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return RT_E_HIP;
    std::lock_guard<std::mutex> g(g_ws.mu);
    *count = 0;
    Workspace *wp = g_ws.find();
    if (!wp) return RT_OK;
    Workspace &w = *wp;
    if (flush_pending(w) != 0 || resolve_profiles(w) != 0) return RT_E_HIP;
    *count = (int)w.prof_hist.size();
    for (int i = 0; i < cap && i < *count; ++i) out[i] = w.prof_hist[i];
    if (reset) w.prof_hist.clear();
    return RT_OK;
}

int rt_launch_wavefront(const RtDevScene &sc, const RtDevFrame &fr, const RtDevCamera &cam, const RtOptions &o)
{
    // 1: wave-cooperative leaves (entries packed as k << 6 | lane: needs < 2^26 entries), 2: static, 3: per-lane fetch
    int trace_kind = o.kernel;
    if (trace_kind == 1 && sc.index_count >= (1 << 26)) trace_kind = 3;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    rt_register_shutdown();
    std::lock_guard<std::mutex> g(g_ws.mu);
    Workspace &w = g_ws.slots[dev];
    const size_t slots = (size_t)fr.width * fr.height;
    const bool count = fr.counters != nullptr;
    // the queue trace launches run the BVH-bounded traversal (counting calls: the KD one, whose counters are the reference's)
    const bool bounded = sc.bvh_nodes != nullptr && ((o.traversal == RT_TRAVERSAL_BOUNDED && !count) ||
                                                     o.traversal == RT_TRAVERSAL_BOUNDED_COUNTED);
    // paths deeper than this leave their pipeline for wf_long (cooperative trace only)
    // (at least WF_LONG_DEPTH_MIN: wf_long is sized for the rare deep paths — one path per wave on its 64
    // blocks —, and at depth 8 the hand-off took a third of all paths and ran 7x slower)
    const int long_opt = o.wf_long_depth;
    const int long_depth = trace_kind == 1 && long_opt >= 0
                               ? (long_opt > 0 ? (long_opt > WF_LONG_DEPTH_MIN ? long_opt : WF_LONG_DEPTH_MIN)
                                               : WF_LONG_DEPTH_DEFAULT)
                               : 0;
    // bounded traversal, not counting: the whole call in the finisher by default
    // — one path per lane to the end of its passes beats queue iterations once
    // a ray query is ~30 dependent loads: 1.22 vs 1.61 s per 256-pass room2m
    // call with deep paths cut (profiles/r03).  It runs as ONE pipeline whose
    // finisher spans the chip: three pipelines' fixed pixel sets finished up
    // to 0.7 s apart, each leaving its third of the chip idle.
    // (RT_TRAVERSAL_BOUNDED_COUNTED: the same whole call, its finisher counting its own work — the
    // bench's per-launch algorithmic bytes then describe the timed launch's own shape)
    const bool whole = bounded && (!count || o.traversal == RT_TRAVERSAL_BOUNDED_COUNTED) && trace_kind == 1 &&
                       (o.wf_tail <= 0 || (size_t)o.wf_tail > slots);
    if (!whole) return launch_queue(w, dev, sc, fr, cam, o, trace_kind, bounded, long_depth);
    WholeCall c;
    c.dev = dev;
    c.sc = sc;
    c.fr = fr;
    c.cam = cam;
    c.stream = (hipStream_t)o.stream;
    c.long_depth = long_depth;
    c.prof = o.profile != 0;
    c.overlap = o.overlap != 0 && !count;
    c.debug = o.debug;
    c.count = count;
    // the run-time exactness guard: 1 ray in check_interval (a power of two) re-traced by the KD traversal
    c.check_mask = 0xFFFFFFFFu;
    if (o.check_interval >= 0 && !count) {
        uint32_t iv = o.check_interval > 0 ? (uint32_t)o.check_interval : WF_CHECK_INTERVAL_DEFAULT;
        uint32_t p2 = 1;
        while (p2 < iv && p2 < (1u << 30)) p2 <<= 1;
        c.check_mask = p2 - 1;
    }
    return launch_whole(w, c, o.coalesce_passes < 0 ? 0 : (o.coalesce_passes > 0 ? o.coalesce_passes : WF_COALESCE_DEFAULT));
}
