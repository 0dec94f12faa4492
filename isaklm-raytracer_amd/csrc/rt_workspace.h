// rt_workspace.h — one workspace per device, its users ordered by an event
// (host only): the megakernel's spill area (path_kernel.hip), the query
// workspace (query.hip), the denoiser's buffers (denoise.hip), the wavefront
// workspace (wavefront.hip; several events, one per stream that may run last)
// and the deviation block (abi.hip; no event, nothing in it is replaced).
//
// The order every user follows, under the table's mutex until its launch is
// enqueued: (1) a buffer of the wrong size is replaced only after
// serial.wait_host() — its last user may still be running, on any stream;
// (2) serial.wait_on(stream); (3) the launches; (4) serial.record(stream),
// their launch status and the event the next user waits for.
#pragma once
#include <hip/hip_runtime_api.h>

#include <map>
#include <mutex>

struct SerialEvent {
    hipEvent_t ev = nullptr; // after the last launch that used the workspace
    bool recorded = false;

    // the event ahead of its first use (wait_on makes it otherwise)
    bool create() { return ev || hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess; }
    // `stream` waits for the previous user, whatever stream that was on
    bool wait_on(hipStream_t stream)
    {
        return create() && (!recorded || hipStreamWaitEvent(stream, ev, 0) == hipSuccess);
    }
    // the host waits for the previous user: before a buffer is freed or replaced
    bool wait_host() { return !recorded || hipEventSynchronize(ev) == hipSuccess; }
    // the previous user's state, without waiting: hipSuccess (done, or there was none), hipErrorNotReady, or its failure
    hipError_t query() { return recorded ? hipEventQuery(ev) : hipSuccess; }
    // after this user's launches on `stream` (false: one of them failed, or the record did)
    bool record(hipStream_t stream)
    {
        if (hipGetLastError() != hipSuccess || hipEventRecord(ev, stream) != hipSuccess) return false;
        recorded = true;
        return true;
    }
    // waits for the last user; the buffers may be freed afterwards
    void destroy()
    {
        (void)wait_host();
        if (ev) (void)hipEventDestroy(ev);
    }
};

template <typename R>
struct DeviceSlots {
    std::mutex mu; // held by the caller from current() / find() until its launch is enqueued
    std::map<int, R> slots;

    // the current device's slot, default-constructed on first use (nullptr: no current device)
    R *current()
    {
        int dev = 0;
        return hipGetDevice(&dev) == hipSuccess ? &slots[dev] : nullptr;
    }
    // the current device's slot if it has one (nullptr: none yet, and none is made)
    R *find()
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return nullptr;
        auto it = slots.find(dev);
        return it == slots.end() ? nullptr : &it->second;
    }
    // release(slot) for every device's slot with that device current; the
    // table is empty afterwards and the caller's device current again
    template <typename F>
    void shutdown(F release)
    {
        std::lock_guard<std::mutex> g(mu);
        int cur = 0;
        (void)hipGetDevice(&cur);
        for (auto &kv : slots)
            if (hipSetDevice(kv.first) == hipSuccess) release(kv.second);
        slots.clear();
        (void)hipSetDevice(cur);
    }
};
