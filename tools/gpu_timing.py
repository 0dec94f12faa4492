"""How the per-call tools time a span on the GPU: one stream, two events, the variants of a
comparison alternating in one process so that clock and thermal drift hit them alike.

Importing this module puts the binding, the oracle and the tests' helpers on sys.path, as every tool needs.
"""
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "isaklm-raytracer_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

_hip = None


def hip():
    """libamdhip64 with the argtypes of the calls the tools make (every one returns a hipError_t)"""
    global _hip
    if _hip is None:
        vp, H = ctypes.c_void_p, ctypes.CDLL("libamdhip64.so")
        H.hipStreamCreate.argtypes = H.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
        for name in ("hipStreamDestroy", "hipStreamSynchronize", "hipEventDestroy", "hipEventSynchronize"):
            getattr(H, name).argtypes = [vp]
        H.hipEventRecord.argtypes = [vp, vp]
        H.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
        H.hipMemcpyAsync.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, vp]
        _hip = H
    return _hip


def require_device(tool):
    """device 0 made current, or the tool's exit: a timing needs a GPU"""
    import helpers
    import rt

    if not helpers.gpu_has_device():
        raise SystemExit(f"{tool}: no HIP device (nothing is measured without one)")
    rt.check(rt.lib().rt_set_device(0))


class Timer:
    """one stream and two events; a context manager that destroys them"""

    def __init__(self):
        self.stream, self.e0, self.e1 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        assert hip().hipStreamCreate(ctypes.byref(self.stream)) == 0
        assert hip().hipEventCreate(ctypes.byref(self.e0)) == 0 and hip().hipEventCreate(ctypes.byref(self.e1)) == 0

    @property
    def s(self):
        """the stream as the integer the binding's `stream` arguments take"""
        return self.stream.value

    def start(self):
        assert hip().hipEventRecord(self.e0, self.stream) == 0

    def stop(self):
        assert hip().hipEventRecord(self.e1, self.stream) == 0

    def elapsed_ms(self):
        """between start() and stop(), once the device has passed both"""
        ms = ctypes.c_float()
        assert hip().hipEventElapsedTime(ctypes.byref(ms), self.e0, self.e1) == 0
        return ms.value

    def synchronize(self):
        assert hip().hipStreamSynchronize(self.stream) == 0

    def span(self, fn, batch=1):
        """fn() `batch` times between the two events on the stream, ending in the event synchronise:
        (device ms per call, host ms of the whole span)"""
        t0 = time.perf_counter()
        self.start()
        for _ in range(batch):
            fn()
        self.stop()
        assert hip().hipEventSynchronize(self.e1) == 0
        host_ms = (time.perf_counter() - t0) * 1e3
        return self.elapsed_ms() / batch, host_ms

    def close(self):
        if self.stream:
            assert hip().hipEventDestroy(self.e0) == 0 and hip().hipEventDestroy(self.e1) == 0
            assert hip().hipStreamDestroy(self.stream) == 0
            self.stream = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def interleaved(variants, launch, warmup, reps):
    """{variant: [launch(variant) of each of `reps` rounds]}: every round launches every variant once, in order;
    the first `warmup` rounds are discarded"""
    results = {v: [] for v in variants}
    for r in range(warmup + reps):
        for v in variants:
            x = launch(v)
            if r >= warmup:
                results[v].append(x)
    return results


def summary(ms, digits):
    """the record of a variant's timings: spread = (max - min) / median"""
    med = statistics.median(ms)
    return {"reps": len(ms), "ms_median": round(med, digits), "ms_min": round(min(ms), digits),
            "ms_max": round(max(ms), digits), "spread": round((max(ms) - min(ms)) / med, 4)}


def write_lines(path, records):
    """one JSON line per record, printed and written to `path`"""
    import json

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for rec in records:
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
