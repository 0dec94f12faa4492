// Drives rt_workspace.h's slot table (both lookups), serial event (made on first use or ahead of it, waited
// for, queried) and shutdown walk with a stub resource and stub HIP entry points (no runtime linked): built
// with -fsanitize=address,undefined.
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <thread>
#include <vector>

#include "rt_workspace.h"

namespace {
int g_dev = 0, g_ndev = 4;
int g_fail_set = -1; // a device hipSetDevice refuses
std::set<int *> g_events; // live events (heap cells: a leak or double destroy is ASan's to find too)
int g_stream_waits = 0, g_host_waits = 0, g_records = 0, g_queries = 0;
hipError_t g_launch_error = hipSuccess;
hipError_t g_query_result = hipSuccess; // what the recorded work's state is
} // namespace

extern "C" {
hipError_t hipGetDevice(int *d) { *d = g_dev; return hipSuccess; }
hipError_t hipSetDevice(int d)
{
    if (d < 0 || d >= g_ndev || d == g_fail_set) return hipErrorInvalidDevice;
    g_dev = d;
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned)
{
    int *p = new int(g_dev);
    g_events.insert(p);
    *e = (hipEvent_t)p;
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    int *p = (int *)e;
    assert(g_events.count(p) == 1);
    assert(*p == g_dev); // destroyed with its own device current
    g_events.erase(p);
    delete p;
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t e, unsigned)
{
    assert(g_events.count((int *)e) == 1);
    ++g_stream_waits;
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    assert(g_events.count((int *)e) == 1);
    ++g_host_waits;
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t e)
{
    assert(g_events.count((int *)e) == 1);
    ++g_queries;
    return g_query_result;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t)
{
    assert(g_events.count((int *)e) == 1);
    ++g_records;
    return hipSuccess;
}
hipError_t hipGetLastError(void)
{
    const hipError_t e = g_launch_error;
    g_launch_error = hipSuccess;
    return e;
}
}

struct Res { // a workspace: one heap buffer and its serial event
    int *buf = nullptr;
    size_t n = 0;
    SerialEvent serial;
};

static int g_live_bufs = 0;

// what every user does (rt_workspace.h's order)
static bool use(DeviceSlots<Res> &t, size_t n)
{
    std::lock_guard<std::mutex> g(t.mu);
    Res *r = t.current();
    if (!r) return false;
    if (r->n < n) {
        if (!r->serial.wait_host()) return false;
        if (r->buf) { delete[] r->buf; --g_live_bufs; }
        r->buf = new int[n];
        ++g_live_bufs;
        r->n = n;
    }
    if (!r->serial.wait_on(nullptr)) return false;
    r->buf[n - 1] = 1; // "the launch"
    return r->serial.record(nullptr);
}

static void release(Res &r)
{
    r.serial.destroy();
    if (r.buf) { delete[] r.buf; --g_live_bufs; }
}

int main()
{
    DeviceSlots<Res> t;
    // first use: no wait of either kind, one record
    assert(use(t, 8));
    assert(g_stream_waits == 0 && g_host_waits == 0 && g_records == 1 && g_events.size() == 1);
    // same size: a stream wait only
    assert(use(t, 8));
    assert(g_stream_waits == 1 && g_host_waits == 0 && g_records == 2);
    // growth: the host waits before the buffer is replaced
    assert(use(t, 64));
    assert(g_host_waits == 1 && g_live_bufs == 1);
    // a failed launch: reported, the event not recorded anew
    g_launch_error = hipErrorLaunchFailure;
    assert(!use(t, 8));
    assert(g_records == 3);
    assert(use(t, 8));
    // other devices get their own slots
    for (int d = 1; d < g_ndev; ++d) {
        g_dev = d;
        assert(use(t, 16 + d));
    }
    assert(t.slots.size() == 4 && g_events.size() == 4 && g_live_bufs == 4);
    // many threads on one table (the mutex is the caller's: TSan-free here, but ASan sees a torn map)
    g_dev = 2;
    std::vector<std::thread> th;
    for (int k = 0; k < 8; ++k) th.emplace_back([&t, k] { for (int i = 0; i < 200; ++i) (void)use(t, 8 + (size_t)((i * 7 + k) % 50)); });
    for (auto &x : th) x.join();
    // the walk: every slot released with its device current, a device that cannot be entered is skipped (its
    // resources are the runtime's to reclaim), the caller's device restored, the table empty
    g_dev = 2;
    g_fail_set = 3;
    int *leaked_ev = nullptr, *leaked_buf = t.slots[3].buf;
    leaked_ev = (int *)t.slots[3].serial.ev;
    t.shutdown(release);
    assert(g_dev == 2 && t.slots.empty());
    assert(g_events.size() == 1 && g_live_bufs == 1);
    g_fail_set = -1;
    g_events.erase(leaked_ev); // (the stub's skipped device: freed here so that LeakSanitizer sees only real leaks)
    delete leaked_ev;
    delete[] leaked_buf;
    --g_live_bufs;
    // a second walk over the empty table, and use after shutdown
    t.shutdown(release);
    assert(use(t, 4));
    t.shutdown(release);
    assert(g_events.empty() && g_live_bufs == 0 && g_dev == 2);
    // an event made ahead of its first use (the wavefront workspace's): once; nothing recorded is done
    // without a runtime call, and neither wait calls one; recorded work's state is the runtime's
    {
        SerialEvent e;
        const int sw = g_stream_waits, hw = g_host_waits;
        assert(e.query() == hipSuccess && g_queries == 0 && g_events.empty());
        assert(e.create() && g_events.size() == 1);
        hipEvent_t first = e.ev;
        assert(e.create() && e.ev == first && g_events.size() == 1);
        assert(e.query() == hipSuccess && g_queries == 0);
        assert(e.wait_on(nullptr) && e.wait_host() && g_stream_waits == sw && g_host_waits == hw);
        assert(e.ev == first && g_events.size() == 1);
        assert(e.record(nullptr));
        g_query_result = hipErrorNotReady;
        assert(e.query() == hipErrorNotReady && g_queries == 1);
        g_query_result = hipErrorLaunchFailure;
        assert(e.query() == hipErrorLaunchFailure && g_queries == 2);
        g_query_result = hipSuccess;
        assert(e.query() == hipSuccess && g_queries == 3);
        assert(e.wait_on(nullptr) && g_stream_waits == sw + 1);
        e.destroy();
        assert(g_events.empty() && g_host_waits == hw + 1);
    }
    // a lookup that makes nothing (a join on a device that never rendered), then the slot current() made
    {
        DeviceSlots<Res> u;
        std::lock_guard<std::mutex> g(u.mu);
        g_dev = 1;
        assert(u.find() == nullptr && u.slots.empty());
        Res *made = u.current();
        assert(made && u.find() == made && u.slots.size() == 1);
        g_dev = 2;
        assert(u.find() == nullptr && u.slots.size() == 1);
    }
    // a table without an event (the deviation block's shape)
    DeviceSlots<int *> blocks;
    {
        std::lock_guard<std::mutex> g(blocks.mu);
        int **p = blocks.current();
        assert(p && *p == nullptr);
        *p = new int[4];
    }
    blocks.shutdown([](int *&p) { delete[] p; });
    assert(blocks.slots.empty());
    printf("workspace_check OK: stream waits %d, host waits %d, records %d, queries %d\n", g_stream_waits, g_host_waits,
           g_records, g_queries);
    return 0;
}
