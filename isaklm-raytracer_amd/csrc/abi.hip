// abi.hip — implementation of include/isaklm_rt.h (the drop-in boundary).
//
// Thin by design: host scene code lives in host/*.cpp, kernels in
// path_kernel.hip.  Every entry point checks its arguments and every HIP
// call, returning RT_E_* instead of the reference's silent failures
// (SURVEY §5 "Failure detection").
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "camera_math.h"
#include "convergence_math.h"
#include "denoise_math.h"
#include "host/rt_host.h"
#include "reproject_math.h"
#include "rt_launch.h"
#include "rt_workspace.h"
#include "sampler_math.h"

// host/reproject_host.cpp: the overlap rule
bool rt_rp_frames_overlap(const void *src_fb, const void *src_sq, const void *src_count, const void *dst_fb,
                          const void *dst_sq, const void *dst_count, size_t n);
// ... and rt_reproject_sampler's rule for its two samplers (nullptr, or the text of the rule that failed)
const char *rt_rp_resolve_samplers(const RtSampler *src, const RtSampler *dst, RtDevSampler *s, RtDevSampler *d);

static thread_local std::string g_error;

void rt_set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}

#define HIPCHK(expr)                                                                                 \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            rt_set_error("%s failed: %s", #expr, hipGetErrorString(e_));                             \
            return RT_E_HIP;                                                                         \
        }                                                                                            \
    } while (0)

// rt_wavefront_join with the ABI's status: RT_E_INCOMPLETE when the join's
// hand-off check found stranded pixels (a chained render's frame misses
// passes), RT_E_HIP on a HIP failure; `who` names the entry point
// (consume = 0: a stranded-pixel result is left for the next reporting join)
static int join_status(void *stream, const char *who, int consume = 1)
{
    const int rc = rt_wavefront_join(stream, consume);
    if (rc == 0) return RT_OK;
    if (rc == RT_WAVEFRONT_INCOMPLETE) {
        rt_set_error("%s: %s", who, rt_wavefront_incomplete_msg());
        return RT_E_INCOMPLETE;
    }
    rt_set_error("%s: join: %s", who, hipGetErrorString(hipGetLastError()));
    return RT_E_HIP;
}

// the tail of every entry point that launches: the launcher's status (the HIP error's text with it), and a
// call on the null stream returns with its work done
static int launch_done(const char *who, int launch, hipStream_t stream)
{
    if (launch != 0) { rt_set_error("%s: launch failed: %s", who, hipGetErrorString(hipGetLastError())); return RT_E_HIP; }
    if (!stream) HIPCHK(hipStreamSynchronize(nullptr));
    return RT_OK;
}

struct RtPreparedScene {
    RtDevScene dev;
    std::vector<void *> allocs;
    size_t bytes = 0;
    int ntris = 0, nnodes = 0, nindices = 0, max_depth = 0;
};

namespace {

template <typename T>
int upload_vec(RtPreparedScene &s, const std::vector<T> &v, const T **out)
{
    void *p = nullptr;
    size_t n = v.size() * sizeof(T);
    // 64 zero bytes of slack after every array: the traversal's 16-B node-pair
    // loads read one node past the last (never used: the last node in
    // pre-order is a leaf)
    HIPCHK(hipMalloc(&p, n + 64));
    s.allocs.push_back(p);
    s.bytes += n;
    HIPCHK(hipMemset(p, 0, n + 64));
    if (n) HIPCHK(hipMemcpy(p, v.data(), n, hipMemcpyHostToDevice));
    *out = (const T *)p;
    return RT_OK;
}

void release(RtPreparedScene *s)
{
    if (!s) return;
    for (void *p : s->allocs) (void)hipFree(p);
    delete s;
}

int upload_prepared(const rt_host::PreparedHost &h, int ntris, int nindices, rt_scene_t *out)
{
    RtPreparedScene *s = new RtPreparedScene();
    int rc = RT_OK;
    const uint32_t *nodes = nullptr;
    const int *lights = nullptr;
    const RtF4 *a = nullptr, *sh = nullptr;
    const RtIsectBary *bary = nullptr;
    const uint32_t *itri = nullptr;
    const RtDevMaterial *mats = nullptr;
    if ((rc = upload_vec(*s, h.nodes, &nodes)) || (rc = upload_vec(*s, h.isect_a, &a)) ||
        (rc = upload_vec(*s, h.isect_bary, &bary)) || (rc = upload_vec(*s, h.isect_tri, &itri)) ||
        (rc = upload_vec(*s, h.shade, &sh)) ||
        (rc = upload_vec(*s, h.materials, &mats)) || (rc = upload_vec(*s, h.lights, &lights))) {
        release(s);
        return rc;
    }
    RtDevScene &dv = s->dev;
    dv.bvh_nodes = nullptr;
    dv.bvh4 = nullptr;
    dv.bvh_wide = nullptr;
    dv.bvh_a = nullptr;
    dv.bvh_bary = nullptr;
    dv.bvh_scale = h.bvh_scale;
    dv.split_vals = nullptr;
    dv.kd_rows = nullptr;
    dv.kd_cell = nullptr;
    dv.kd_grid = 0;
    for (int a = 0; a < 3; ++a) dv.kd_gscale[a] = h.kd_grid_scale[a];
    for (int a = 0; a < 4; ++a) dv.split_off[a] = h.split_off[a];
    if (h.bvh_depth >= 0 && ((rc = upload_vec(*s, h.bvh_nodes, &dv.bvh_nodes)) ||
                             (rc = upload_vec(*s, h.bvh4, &dv.bvh4)) ||
                             (rc = upload_vec(*s, h.bvh_wide, &dv.bvh_wide)) ||
                             (rc = upload_vec(*s, h.bvh_a, &dv.bvh_a)) ||
                             (rc = upload_vec(*s, h.bvh_bary, &dv.bvh_bary)) ||
                             (rc = upload_vec(*s, h.split_vals, &dv.split_vals)))) {
        release(s);
        return rc;
    }
    // the root-path records and the grid (wf_long's deep bounces enter at the origin's cell)
    if (!h.kd_rows.empty() && ((rc = upload_vec(*s, h.kd_rows, &dv.kd_rows)) ||
                               (h.kd_grid > 0 && (rc = upload_vec(*s, h.kd_cell, &dv.kd_cell))))) {
        release(s);
        return rc;
    }
    if (dv.kd_cell) dv.kd_grid = h.kd_grid;
    // the T* certificate's tables (bvh_common.h rt_kd_cert)
    dv.kd_cert = RtKdCert{nullptr, nullptr, {0, 0, 0}, {31, 31, 31}, h.bvh_scale};
    if (h.bvh_depth >= 0 && !h.kd_safe.empty()) {
        if ((rc = upload_vec(*s, h.kd_safe, &dv.kd_cert.safe)) || (rc = upload_vec(*s, h.split_hash, &dv.kd_cert.hash))) {
            release(s);
            return rc;
        }
        for (int a = 0; a < 3; ++a) {
            dv.kd_cert.hoff[a] = h.split_hoff[a];
            dv.kd_cert.hshift[a] = h.split_hshift[a];
        }
    }
    dv.nodes = nodes;
    dv.isect_a = a;
    dv.isect_bary = bary;
    dv.isect_tri = itri;
    dv.shade = sh;
    dv.materials = mats;
    dv.lights = lights;
    dv.light_count = h.light_count;
    dv.triangle_count = ntris;
    dv.index_count = nindices;
    dv.node_count = (int)(h.nodes.size() / 2);
    dv.bmin[0] = h.bounds.min.x; dv.bmin[1] = h.bounds.min.y; dv.bmin[2] = h.bounds.min.z;
    dv.bmax[0] = h.bounds.max.x; dv.bmax[1] = h.bounds.max.y; dv.bmax[2] = h.bounds.max.z;
    s->ntris = ntris;
    s->nnodes = (int)(h.nodes.size() / 2);
    s->nindices = nindices;
    s->max_depth = h.max_depth;
    *out = s;
    return RT_OK;
}

// always-on deviation statistics (RT_DEV_*), one zeroed block per device (never replaced: no event)
DeviceSlots<unsigned long long *> g_dev_stats;

unsigned long long *dev_stats_block()
{
    std::lock_guard<std::mutex> g(g_dev_stats.mu);
    unsigned long long **slot = g_dev_stats.current();
    if (!slot) return nullptr;
    if (*slot) return *slot;
    void *p = nullptr;
    if (hipMalloc(&p, RT_DEV_WORDS * 8) != hipSuccess) return nullptr;
    if (hipMemset(p, 0, RT_DEV_WORDS * 8) != hipSuccess) {
        (void)hipFree(p);
        return nullptr;
    }
    return *slot = (unsigned long long *)p;
}

} // namespace

// rt_shutdown at exit, registered once by rt_set_device / the first render:
// atexit handlers run in reverse registration order, so this one (registered
// after the HIP runtime initialised) runs before the runtime's own finalisers
// and the library's streams, events and blobs are gone before they run
void rt_register_shutdown()
{
    static std::once_flag once;
    std::call_once(once, [] { atexit(rt_shutdown); });
}

extern "C" {

const char *rt_last_error(void) { return g_error.c_str(); }
const char *rt_version(void) { return "isaklm-raytracer_amd 0.3 (gfx950)"; }
int rt_abi_version(void) { return RT_ABI_VERSION; }

void rt_shutdown(void)
{
    rt_wavefront_shutdown();
    rt_path_shutdown();
    rt_query_shutdown();
    rt_denoise_shutdown();
    g_dev_stats.shutdown([](unsigned long long *&p) { (void)hipFree(p); });
}

int rt_join(void *stream) { return join_status(stream, "rt_join"); }

int rt_deviation_stats(RtDeviations *out, int reset)
{
    if (!out) { rt_set_error("rt_deviation_stats: null out"); return RT_E_INVALID; }
    unsigned long long *d = dev_stats_block();
    if (!d) { rt_set_error("rt_deviation_stats: no device block"); return RT_E_HIP; }
    unsigned long long w[RT_DEV_WORDS];
    // (chained renders joined first, so their statistics are complete; stranded
    // pixels are not an error here — stranded_pixels reports them — and stay the
    // next reporting join's RT_E_INCOMPLETE: rt_join, rt_download, rt_synchronize ...)
    const int jr = join_status(nullptr, "rt_deviation_stats", 0);
    if (jr != RT_OK && jr != RT_E_INCOMPLETE) return jr;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(w, d, sizeof w, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    out->watchdog_paths = w[RT_DEV_WATCHDOG];
    out->cut_paths = w[RT_DEV_CUT];
    out->max_deep_depth = w[RT_DEV_MAXDEPTH];
    for (int k = 0; k < RT_DEV_HIST_BINS; ++k) {
        out->deep_hist[k] = w[RT_DEV_HIST + k];
        out->deep_paths += w[RT_DEV_HIST + k];
    }
    out->bounded_checked = w[RT_DEV_CHECKED];
    out->bounded_mismatches = w[RT_DEV_MISMATCH];
    for (int k = 0; k < 3; ++k) {
        const uint32_t hi = (uint32_t)(w[RT_DEV_MISRAY + 1 + k] >> 32), lo = (uint32_t)w[RT_DEV_MISRAY + 1 + k];
        memcpy(&out->mismatch_ray[2 * k], &hi, 4);
        memcpy(&out->mismatch_ray[2 * k + 1], &lo, 4);
    }
    out->owed_pixels = w[RT_DEV_OWED_PIXELS];
    out->owed_passes = w[RT_DEV_OWED_PASSES];
    out->long_safety_quits = w[RT_DEV_LONG_QUIT];
    out->stranded_pixels = w[RT_DEV_STRANDED];
    out->check_dropped = w[RT_DEV_CHK_DROP];
    out->linger_expiries = w[RT_DEV_LINGER_EXP];
    out->long_closed = w[RT_DEV_LONG_CLOSED];
    out->wide_overflows = w[RT_DEV_WIDE_OVERFLOW];
    if (reset) HIPCHK(hipMemset(d, 0, RT_DEV_WORDS * 8));
    return RT_OK;
}

// the T* certificate's counters of counting renders (RT_DEV_CERT_*; zeroed by rt_deviation_stats' reset too)
int rt_kd_cert_stats(unsigned long long *certified, unsigned long long *fallback, int reset)
{
    unsigned long long *d = dev_stats_block();
    if (!d) { rt_set_error("rt_kd_cert_stats: no device block"); return RT_E_HIP; }
    const int jr = join_status(nullptr, "rt_kd_cert_stats", 0);
    if (jr != RT_OK && jr != RT_E_INCOMPLETE) return jr;
    HIPCHK(hipDeviceSynchronize());
    unsigned long long w[2];
    HIPCHK(hipMemcpy(w, d + RT_DEV_CERT_OK, sizeof w, hipMemcpyDeviceToHost));
    if (certified) *certified = w[0];
    if (fallback) *fallback = w[1];
    if (reset) HIPCHK(hipMemset(d + RT_DEV_CERT_OK, 0, sizeof w));
    return RT_OK;
}

// ---------------- device memory ----------------
int rt_device_alloc(void **ptr, size_t bytes)
{
    if (!ptr) { rt_set_error("rt_device_alloc: null out"); return RT_E_INVALID; }
    HIPCHK(hipMalloc(ptr, bytes ? bytes : 16));
    return RT_OK;
}
int rt_free(void *ptr)
{
    if (ptr) HIPCHK(hipFree(ptr));
    return RT_OK;
}
int rt_upload(void *dst, const void *src, size_t bytes)
{
    if (bytes == 0) return RT_OK;
    if (!dst || !src) { rt_set_error("rt_upload: null pointer"); return RT_E_INVALID; }
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return RT_OK;
}
int rt_download(void *dst, const void *src, size_t bytes)
{
    if (bytes == 0) return RT_OK;
    if (!dst || !src) { rt_set_error("rt_download: null pointer"); return RT_E_INVALID; }
    // (cudaMemcpy after a render waits for it; so does this, chained renders' tails included)
    const int jr = join_status(nullptr, "rt_download");
    if (jr != RT_OK) return jr;
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}
int rt_memset(void *dst, int value, size_t bytes)
{
    if (bytes == 0) return RT_OK;
    HIPCHK(hipMemset(dst, value, bytes));
    return RT_OK;
}
int rt_device_count(int *count)
{
    if (!count) return RT_E_INVALID;
    HIPCHK(hipGetDeviceCount(count));
    return RT_OK;
}
int rt_set_device(int device)
{
    HIPCHK(hipSetDevice(device));
    rt_register_shutdown();
    if (rt_wavefront_device_init() != 0) { // the pipelines' streams take their hardware queues first
        rt_set_error("rt_set_device: wavefront streams: %s", hipGetErrorString(hipGetLastError()));
        return RT_E_HIP;
    }
    return RT_OK;
}
int rt_synchronize(void)
{
    // (chained renders' open chain drained first: hipDeviceSynchronize alone never
    // enqueues the drain, and their owed passes would never run)
    const int jr = join_status(nullptr, "rt_synchronize");
    if (jr != RT_OK) return jr;
    HIPCHK(hipDeviceSynchronize());
    return RT_OK;
}
void rt_host_free(void *p) { free(p); }

// ---------------- texture decoding (make_texture's stbi_load, rt/scene.cuh:33) ----------------
static int decode_out(int rc, const std::vector<uint8_t> &rgba, const std::string &err, int w, int h,
                      uint8_t **rgba_out, int *width, int *height)
{
    if (rc != RT_OK) {
        rt_set_error("rt_decode_image: %s", err.c_str());
        return rc;
    }
    uint8_t *p = (uint8_t *)malloc(rgba.size() ? rgba.size() : 1);
    if (!p) { rt_set_error("rt_decode_image: out of host memory"); return RT_E_NOMEM; }
    memcpy(p, rgba.data(), rgba.size());
    *rgba_out = p;
    *width = w;
    *height = h;
    return RT_OK;
}

int rt_decode_image(const char *path, uint8_t **rgba_out, int *width, int *height)
{
    if (!path || !rgba_out || !width || !height) { rt_set_error("rt_decode_image: null argument"); return RT_E_INVALID; }
    std::vector<uint8_t> rgba;
    std::string err;
    int w = 0, h = 0;
    const int rc = rt_host::decode_image_file(path, rgba, w, h, err);
    return decode_out(rc, rgba, err, w, h, rgba_out, width, height);
}

int rt_decode_image_memory(const void *data, size_t size, uint8_t **rgba_out, int *width, int *height)
{
    if (!data || !rgba_out || !width || !height) {
        rt_set_error("rt_decode_image_memory: null argument");
        return RT_E_INVALID;
    }
    std::vector<uint8_t> rgba;
    std::string err;
    int w = 0, h = 0;
    const int rc = rt_host::decode_image_memory((const uint8_t *)data, size, rgba, w, h, err);
    return decode_out(rc, rgba, err, w, h, rgba_out, width, height);
}

// ---------------- G_Buffer ----------------
int rt_gbuffer_seeds(uint32_t *out, size_t count, uint64_t skip)
{
    if (!out && count) { rt_set_error("rt_gbuffer_seeds: null out"); return RT_E_INVALID; }
    rt_host::mt19937_seeds(out, count, skip);
    return RT_OK;
}

static void gbuffer_free(G_Buffer *g)
{
    (void)hipFree(g->frame_buffer);
    (void)hipFree(g->squared_luminance);
    (void)hipFree(g->sample_count);
    (void)hipFree(g->random_numbers);
    memset(g, 0, sizeof *g);
}

int rt_gbuffer_create(int w, int h, uint64_t skip, G_Buffer *g)
{
    if (!g || w <= 0 || h <= 0) { rt_set_error("rt_gbuffer_create: bad arguments"); return RT_E_INVALID; }
    const size_t n = (size_t)w * (size_t)h;
    memset(g, 0, sizeof *g);
    std::vector<uint32_t> seeds(n);
    rt_host::mt19937_seeds(seeds.data(), n, skip);
    const int rc = [&]() -> int {
        HIPCHK(hipMalloc((void **)&g->frame_buffer, n * sizeof(Vec3D)));
        HIPCHK(hipMalloc((void **)&g->squared_luminance, n * sizeof(float)));
        HIPCHK(hipMalloc((void **)&g->sample_count, n * sizeof(int)));
        HIPCHK(hipMalloc((void **)&g->random_numbers, n * sizeof(uint32_t)));
        HIPCHK(hipMemset(g->frame_buffer, 0, n * sizeof(Vec3D)));
        HIPCHK(hipMemset(g->squared_luminance, 0, n * sizeof(float)));
        HIPCHK(hipMemset(g->sample_count, 0, n * sizeof(int)));
        HIPCHK(hipMemcpy(g->random_numbers, seeds.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
        return RT_OK;
    }();
    if (rc != RT_OK) gbuffer_free(g); // what the failing path had allocated; *g zeroed again
    return rc;
}

int rt_gbuffer_destroy(G_Buffer *g)
{
    if (!g) return RT_E_INVALID;
    (void)rt_wavefront_join(nullptr, 0); // (a chained render's tail may still write it)
    gbuffer_free(g);
    return RT_OK;
}

// ---------------- checkpoint / resume ----------------
// file: "RTGBUF01", int32 width, height, sample_count, 0; then fb (12 B/px),
// sq, count, rng (4 B/px each), host byte order
static const char kGbufMagic[8] = {'R', 'T', 'G', 'B', 'U', 'F', '0', '1'};

int rt_gbuffer_save(G_Buffer g, int width, int height, int sample_count, const char *path)
{
    if (!path || width <= 0 || height <= 0 || !g.frame_buffer || !g.squared_luminance || !g.sample_count ||
        !g.random_numbers) {
        rt_set_error("rt_gbuffer_save: bad arguments");
        return RT_E_INVALID;
    }
    const size_t n = (size_t)width * height;
    std::vector<uint8_t> buf(n * 24);
    // rt_render's pipelines run on their own non-blocking streams, and a chained render's
    // owed passes run only in the open chain's drain: join (drain) first, then synchronise
    const int jr = join_status(nullptr, "rt_gbuffer_save");
    if (jr != RT_OK) return jr;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(buf.data(), g.frame_buffer, n * 12, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(buf.data() + n * 12, g.squared_luminance, n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(buf.data() + n * 16, g.sample_count, n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(buf.data() + n * 20, g.random_numbers, n * 4, hipMemcpyDeviceToHost));
    // write beside the target and rename over it: an interrupted save never
    // leaves a torn checkpoint in place of the previous one
    const std::string tmp = std::string(path) + ".tmp";
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) {
        rt_set_error("rt_gbuffer_save: cannot write %s", tmp.c_str());
        return RT_E_IO;
    }
    const int32_t hdr[4] = {width, height, sample_count, 0};
    const bool ok = fwrite(kGbufMagic, 1, 8, f) == 8 && fwrite(hdr, 4, 4, f) == 4 &&
                    fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    if (fclose(f) != 0 || !ok || rename(tmp.c_str(), path) != 0) {
        remove(tmp.c_str());
        rt_set_error("rt_gbuffer_save: write error on %s", path);
        return RT_E_IO;
    }
    return RT_OK;
}

int rt_gbuffer_load(const char *path, G_Buffer g, int width, int height, int *sample_count_out)
{
    if (!path) {
        rt_set_error("rt_gbuffer_load: null path");
        return RT_E_INVALID;
    }
    FILE *f = fopen(path, "rb");
    if (!f) {
        rt_set_error("rt_gbuffer_load: cannot read %s", path);
        return RT_E_IO;
    }
    char magic[8];
    int32_t hdr[4];
    if (fread(magic, 1, 8, f) != 8 || memcmp(magic, kGbufMagic, 8) != 0 || fread(hdr, 4, 4, f) != 4) {
        fclose(f);
        rt_set_error("rt_gbuffer_load: %s is not a G_Buffer checkpoint", path);
        return RT_E_PARSE;
    }
    if (hdr[0] != width || hdr[1] != height || !g.frame_buffer || !g.squared_luminance || !g.sample_count ||
        !g.random_numbers) {
        fclose(f);
        rt_set_error("rt_gbuffer_load: checkpoint is %dx%d, G_Buffer %dx%d", hdr[0], hdr[1], width, height);
        return RT_E_INVALID;
    }
    const size_t n = (size_t)width * height;
    std::vector<uint8_t> buf(n * 24);
    const bool ok = fread(buf.data(), 1, buf.size(), f) == buf.size();
    fclose(f);
    if (!ok) {
        rt_set_error("rt_gbuffer_load: %s is truncated", path);
        return RT_E_PARSE;
    }
    // no render may still be writing this G_Buffer (a chained render's tail drained and
    // joined first; the chain is closed, so the next call does not continue it)
    const int jr = join_status(nullptr, "rt_gbuffer_load", 0); // (a stranded result stays the next join's)
    if (jr != RT_OK && jr != RT_E_INCOMPLETE) return jr;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(g.frame_buffer, buf.data(), n * 12, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(g.squared_luminance, buf.data() + n * 12, n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(g.sample_count, buf.data() + n * 16, n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(g.random_numbers, buf.data() + n * 20, n * 4, hipMemcpyHostToDevice));
    if (sample_count_out) *sample_count_out = hdr[2];
    return RT_OK;
}

// ---------------- host scene ----------------
int rt_host_scene_create(RtHostScene **out)
{
    if (!out) return RT_E_INVALID;
    *out = new RtHostScene();
    return RT_OK;
}
void rt_host_scene_destroy(RtHostScene *s) { delete s; }

int rt_host_scene_load_mesh(RtHostScene *s, const char *obj, const char *mat, const float offset[3],
                            const float m[9], int smooth)
{
    if (!s || !obj || !mat || !offset || !m) { rt_set_error("rt_host_scene_load_mesh: null argument"); return RT_E_INVALID; }
    RtM3 M = {rt_v3(m[0], m[1], m[2]), rt_v3(m[3], m[4], m[5]), rt_v3(m[6], m[7], m[8])};
    return rt_host::load_mesh(*s, obj, mat, rt_v3(offset[0], offset[1], offset[2]), M, smooth != 0);
}

int rt_host_scene_load_file(RtHostScene *s, const char *path, Camera *cam)
{
    if (!s || !path) { rt_set_error("rt_host_scene_load_file: null argument"); return RT_E_INVALID; }
    return rt_host::load_scene_file(*s, path, cam);
}

int rt_host_scene_triangles(const RtHostScene *s, const Triangle **tris, int *count)
{
    if (!s || !tris || !count) return RT_E_INVALID;
    *tris = s->tris.data();
    *count = (int)s->tris.size();
    return RT_OK;
}

int rt_build_kd_tree(const Triangle *tris, int n, KD_Tree_Node **nodes_out, int *node_count, int **idx_out,
                     int *index_count, Bounding_Box *bounds)
{
    if (!tris || n <= 0 || !nodes_out || !node_count || !idx_out || !index_count || !bounds) {
        rt_set_error("rt_build_kd_tree: bad arguments");
        return RT_E_INVALID;
    }
    std::vector<KD_Tree_Node> nodes;
    std::vector<int> idx;
    int rc = rt_host::build_kd_tree(tris, n, nodes, idx, *bounds);
    if (rc) return rc;
    *nodes_out = (KD_Tree_Node *)malloc(nodes.size() * sizeof(KD_Tree_Node));
    *idx_out = (int *)malloc((idx.size() ? idx.size() : 1) * sizeof(int));
    if (!*nodes_out || !*idx_out) { rt_set_error("out of host memory"); return RT_E_NOMEM; }
    memcpy(*nodes_out, nodes.data(), nodes.size() * sizeof(KD_Tree_Node));
    memcpy(*idx_out, idx.data(), idx.size() * sizeof(int));
    *node_count = (int)nodes.size();
    *index_count = (int)idx.size();
    return RT_OK;
}

// create_scene (rt/create_scene.cuh:18-73)
// device textures uploaded by rt_create_scene, per device triangle array (freed by rt_destroy_scene)
static std::mutex g_tex_mu;
static std::map<const void *, std::vector<void *>> g_scene_textures;

static void scene_free(Scene *s)
{
    (void)hipFree(s->triangles);
    (void)hipFree(s->light_indicies);
    (void)hipFree(s->kd_tree.nodes);
    (void)hipFree(s->kd_tree.triangle_indicies);
    memset(s, 0, sizeof *s);
}

int rt_create_scene(const RtHostScene *s, Scene *out, int *node_count, int *index_count)
{
    if (!s || !out || s->tris.empty()) { rt_set_error("rt_create_scene: bad arguments"); return RT_E_INVALID; }
    memset(out, 0, sizeof *out);
    const int n = (int)s->tris.size();
    std::vector<KD_Tree_Node> nodes;
    std::vector<int> idx;
    Bounding_Box bb;
    int rc = rt_host::build_kd_tree(s->tris.data(), n, nodes, idx, bb);
    if (rc) return rc;
    const std::vector<int> lights = rt_host::light_list(s->tris.data(), n);
    std::vector<void *> owned; // the textures' device copies
    rc = [&]() -> int {
        HIPCHK(hipMalloc((void **)&out->triangles, (size_t)n * sizeof(Triangle)));
        if (s->textures.empty()) {
            HIPCHK(hipMemcpy(out->triangles, s->tris.data(), (size_t)n * sizeof(Triangle), hipMemcpyHostToDevice));
        } else {
            // make_texture's cudaMalloc/cudaMemcpy (rt/scene.cuh:58-59): one device
            // copy per decoded texture (with its zero pad), triangles re-pointed to it
            std::map<const void *, RtUChar4 *> dev;
            for (const auto &t : s->textures) {
                RtUChar4 *d = nullptr;
                const size_t bytes = t->texels.size() * sizeof(RtUChar4);
                HIPCHK(hipMalloc((void **)&d, bytes));
                owned.push_back(d);
                HIPCHK(hipMemcpy(d, t->texels.data(), bytes, hipMemcpyHostToDevice));
                dev[t->texels.data()] = d;
            }
            std::vector<Triangle> tris(s->tris);
            for (Triangle &t : tris)
                if (t.material.texture.buffer) {
                    auto it = dev.find(t.material.texture.buffer);
                    if (it == dev.end()) {
                        rt_set_error("rt_create_scene: triangle texture not owned by the host scene");
                        return RT_E_INVALID;
                    }
                    t.material.texture.buffer = it->second;
                }
            HIPCHK(hipMemcpy(out->triangles, tris.data(), (size_t)n * sizeof(Triangle), hipMemcpyHostToDevice));
        }
        out->triangle_count = n;
        HIPCHK(hipMalloc((void **)&out->light_indicies, (lights.size() + 1) * sizeof(int)));
        if (!lights.empty())
            HIPCHK(hipMemcpy(out->light_indicies, lights.data(), lights.size() * sizeof(int), hipMemcpyHostToDevice));
        out->light_count = (int)lights.size();
        HIPCHK(hipMalloc((void **)&out->kd_tree.nodes, nodes.size() * sizeof(KD_Tree_Node)));
        HIPCHK(hipMemcpy(out->kd_tree.nodes, nodes.data(), nodes.size() * sizeof(KD_Tree_Node), hipMemcpyHostToDevice));
        HIPCHK(hipMalloc((void **)&out->kd_tree.triangle_indicies, (idx.size() + 1) * sizeof(int)));
        if (!idx.empty())
            HIPCHK(hipMemcpy(out->kd_tree.triangle_indicies, idx.data(), idx.size() * sizeof(int),
                             hipMemcpyHostToDevice));
        return RT_OK;
    }();
    if (rc != RT_OK) { // what the failing path had allocated; *out zeroed again
        for (void *d : owned) (void)hipFree(d);
        scene_free(out);
        return rc;
    }
    if (!owned.empty()) {
        std::lock_guard<std::mutex> g(g_tex_mu);
        g_scene_textures[out->triangles] = owned;
    }
    out->kd_tree.bounding_box = bb;
    if (node_count) *node_count = (int)nodes.size();
    if (index_count) *index_count = (int)idx.size();
    return RT_OK;
}

int rt_destroy_scene(Scene *s)
{
    if (!s) return RT_E_INVALID;
    {
        std::lock_guard<std::mutex> g(g_tex_mu);
        auto it = g_scene_textures.find(s->triangles);
        if (it != g_scene_textures.end()) {
            for (void *d : it->second) (void)hipFree(d);
            g_scene_textures.erase(it);
        }
    }
    scene_free(s);
    return RT_OK;
}

// ---------------- prepared scene ----------------
int rt_scene_prepare_host(const Triangle *tris, int ntris, const KD_Tree_Node *nodes, int nnodes, const int *idx,
                          int nidx, const int *lights, int nlights, Bounding_Box bounds, rt_scene_t *out)
{
    if (!out) return RT_E_INVALID;
    rt_host::PreparedHost h;
    int rc = rt_host::prepare_host(tris, ntris, nodes, nnodes, idx, nidx, lights, nlights, bounds, h);
    if (rc) return rc;
    return upload_prepared(h, ntris, nidx, out);
}

// bytes from p to the end of the device allocation that holds it
static int bytes_to_alloc_end(const void *p, size_t *bytes)
{
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (!p || hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess || !base) {
        (void)hipGetLastError();
        return -1;
    }
    *bytes = (size_t)((const char *)base + size - (const char *)p);
    return 0;
}

// The reference's Scene (rt/scene.cuh:107-121) carries no node or index
// count (they are locals of create_kd_tree, rt/create_kd_tree.cuh:286,300),
// so they are recovered from the device tree itself: the tree is walked
// pre-order from node 0 over a copy of its allocation (hipMemGetAddressRange
// bounds the copy); node_count = highest reachable node + 1, index_count =
// the largest offset + count of a non-empty leaf.  A child index outside the
// allocation, a cycle or a shared subtree is an error.
int rt_scene_prepare(const Scene *ds, rt_scene_t *out)
{
    if (!ds || !out || ds->triangle_count <= 0 || ds->light_count < 0 || !ds->kd_tree.nodes || !ds->triangles) {
        rt_set_error("rt_scene_prepare: bad arguments");
        return RT_E_INVALID;
    }
    size_t node_bytes = 0, index_bytes = 0;
    if (bytes_to_alloc_end(ds->kd_tree.nodes, &node_bytes) != 0) {
        rt_set_error("rt_scene_prepare: kd_tree.nodes is not a device allocation of this process");
        return RT_E_INVALID;
    }
    const size_t max_nodes = node_bytes / sizeof(KD_Tree_Node);
    if (max_nodes == 0 || max_nodes >= (1u << 30)) {
        rt_set_error("rt_scene_prepare: node allocation of %zu bytes", node_bytes);
        return RT_E_INVALID;
    }
    std::vector<KD_Tree_Node> nodes(max_nodes);
    HIPCHK(hipMemcpy(nodes.data(), ds->kd_tree.nodes, max_nodes * sizeof(KD_Tree_Node), hipMemcpyDeviceToHost));
    std::vector<uint8_t> seen(max_nodes, 0);
    std::vector<int> stack{0};
    long long max_node = 0, index_count = 0;
    while (!stack.empty()) {
        const int i = stack.back();
        stack.pop_back();
        if (i < 0 || (size_t)i >= max_nodes || seen[(size_t)i]) {
            rt_set_error("rt_scene_prepare: KD node index %d outside the node allocation, or reached twice", i);
            return RT_E_INVALID;
        }
        seen[(size_t)i] = 1;
        max_node = i > max_node ? i : max_node;
        const KD_Tree_Node &n = nodes[(size_t)i];
        if (n.is_leaf_node) {
            if (n.triangle_count > 0) {
                const long long end = (long long)n.index_offset + n.triangle_count;
                index_count = end > index_count ? end : index_count;
            }
        } else {
            stack.push_back(n.child_index2);
            stack.push_back(n.child_index1);
        }
    }
    if (index_count > 0 && (bytes_to_alloc_end(ds->kd_tree.triangle_indicies, &index_bytes) != 0 ||
                            (size_t)index_count > index_bytes / sizeof(int))) {
        rt_set_error("rt_scene_prepare: leaves address %lld triangle indices beyond the index allocation",
                     index_count);
        return RT_E_INVALID;
    }
    return rt_scene_prepare_counts(ds, (int)(max_node + 1), (int)index_count, out);
}

int rt_scene_prepare_counts(const Scene *ds, int node_count, int index_count, rt_scene_t *out)
{
    if (!ds || !out || ds->triangle_count <= 0 || node_count <= 0 || index_count < 0 || ds->light_count < 0) {
        rt_set_error("rt_scene_prepare: bad arguments");
        return RT_E_INVALID;
    }
    std::vector<Triangle> tris((size_t)ds->triangle_count);
    std::vector<KD_Tree_Node> nodes((size_t)node_count);
    std::vector<int> idx((size_t)index_count), lights((size_t)ds->light_count);
    HIPCHK(hipMemcpy(tris.data(), ds->triangles, tris.size() * sizeof(Triangle), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(nodes.data(), ds->kd_tree.nodes, nodes.size() * sizeof(KD_Tree_Node), hipMemcpyDeviceToHost));
    if (index_count)
        HIPCHK(hipMemcpy(idx.data(), ds->kd_tree.triangle_indicies, idx.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (ds->light_count)
        HIPCHK(hipMemcpy(lights.data(), ds->light_indicies, lights.size() * sizeof(int), hipMemcpyDeviceToHost));
    return rt_scene_prepare_host(tris.data(), ds->triangle_count, nodes.data(), node_count, idx.data(), index_count,
                                 lights.data(), ds->light_count, ds->kd_tree.bounding_box, out);
}

int rt_scene_release(rt_scene_t s)
{
    (void)rt_wavefront_join(nullptr, 0); // (a chained render's tail may still read it)
    release(s);
    return RT_OK;
}

int rt_scene_info(rt_scene_t s, size_t *bytes, int *ntris, int *nnodes, int *nidx, int *max_depth)
{
    if (!s) return RT_E_INVALID;
    if (bytes) *bytes = s->bytes;
    if (ntris) *ntris = s->ntris;
    if (nnodes) *nnodes = s->nnodes;
    if (nidx) *nidx = s->nindices;
    if (max_depth) *max_depth = s->max_depth;
    return RT_OK;
}

// ---------------- render ----------------
void rt_default_options(RtOptions *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->width = 1920;       // rt/macros.h:3
    o->height = 1080;      // rt/macros.h:4
    o->passes = 1;
    o->adaptive = 1;
    o->min_samples = 100;  // rt/macros.h:13
    o->tolerance = 0.05f;  // rt/macros.h:17
    o->max_depth = 0;
}

// render (rt/render.cuh:62-76)
int rt_render(rt_scene_t scene, G_Buffer g, Camera cam, int sample_count, const RtOptions *opt)
{
    RtOptions o;
    if (opt) o = *opt; else rt_default_options(&o);
    if (!scene || !g.frame_buffer || !g.squared_luminance || !g.sample_count || !g.random_numbers) {
        rt_set_error("rt_render: null scene or G_Buffer array");
        return RT_E_INVALID;
    }
    if (o.width <= 0 || o.height <= 0 || o.width < 2 || o.passes < 0 || o.min_samples < 0 ||
        (long long)o.width * o.height > (1LL << 31) - 1) {
        rt_set_error("rt_render: bad frame size / passes");
        return RT_E_INVALID;
    }
    if (o.num_shards > 1 && (o.shard_id < 0 || o.shard_id >= o.num_shards)) {
        rt_set_error("rt_render: shard_id %d out of [0, %d)", o.shard_id, o.num_shards);
        return RT_E_INVALID;
    }
    RtDevFrame fr;
    fr.fb = g.frame_buffer;
    fr.sq = g.squared_luminance;
    fr.count = g.sample_count;
    fr.rng = g.random_numbers;
    fr.width = o.width;
    fr.height = o.height;
    fr.half_w = o.width / 2;   // SCREEN_W / 2 (integer division)
    fr.half_h = o.height / 2;
    fr.passes = o.passes;
    fr.adaptive = o.adaptive;
    fr.min_samples = o.min_samples;
    fr.tolerance = o.tolerance;
    fr.z_const = rt_adaptive_z(o.tolerance);
    fr.max_depth = o.max_depth;
    fr.reset = sample_count == 0;
    fr.shard_id = o.num_shards > 1 ? o.shard_id : 0;
    fr.num_shards = o.num_shards > 1 ? o.num_shards : 1;
    fr.counters = o.counters_device;
    fr.wave_times = o.wave_times_device;
    fr.dev_stats = dev_stats_block();
    if (!fr.dev_stats) {
        rt_set_error("rt_render: deviation statistics block: %s", hipGetErrorString(hipGetLastError()));
        return RT_E_HIP;
    }

    // Camera::rotation() and tanf(FOV / 2) are frame constants (camera_math.h, shared with rt_reproject_host)
    const RtDevCamera dc = rt_device_camera(cam);

    hipStream_t stream = (hipStream_t)o.stream;
    if (o.kernel >= RT_KERNEL_WAVEFRONT && o.kernel <= 3) {
        if (scene->max_depth > RT_STACK_DEPTH || rt_launch_wavefront(scene->dev, fr, dc, o) != 0) {
            rt_set_error("rt_render: wavefront launch failed: %s", hipGetErrorString(hipGetLastError()));
            return RT_E_HIP;
        }
    } else {
        const int jr = join_status(stream, "rt_render"); // (chained wavefront calls' tails first: same frame state)
        if (jr != RT_OK) return jr;
        if (rt_launch_path(scene->dev, fr, dc, scene->max_depth, stream, o.traversal) != 0) {
            rt_set_error("rt_render: kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
            return RT_E_HIP;
        }
    }
    return launch_done("rt_render", 0, stream);
}

// ---------------- ray queries and first-hit AOVs (query.hip) ----------------
void rt_default_query_options(RtQueryOptions *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->traversal = RT_TRAVERSAL_BOUNDED;
}

static bool misaligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// (false: the error text is set; the caller returns RT_E_INVALID, or RT_E_UNSUPPORTED for the stack depth)
static bool count_ok(const char *who, long long n)
{
    if (n >= 0 && n <= (1LL << 31) - 1) return true;
    rt_set_error("%s: n = %lld out of [0, 2^31 - 1]", who, n);
    return false;
}
static bool traversal_ok(const char *who, int t)
{
    if (t == RT_TRAVERSAL_BOUNDED || t == RT_TRAVERSAL_KD || t == RT_TRAVERSAL_BOUNDED_COUNTED) return true;
    rt_set_error("%s: traversal %d", who, t);
    return false;
}
static bool stack_depth_ok(const char *who, rt_scene_t scene)
{
    if (scene->max_depth <= RT_STACK_DEPTH) return true;
    rt_set_error("%s: KD tree depth %d beyond the traversal stack (%d)", who, scene->max_depth, RT_STACK_DEPTH);
    return false;
}

// the checks every query shares, before any GPU call
static int query_options(const char *who, rt_scene_t scene, const RtQueryOptions *opt, RtQueryOptions *o)
{
    if (opt) *o = *opt; else rt_default_query_options(o);
    if (!scene) { rt_set_error("%s: null scene", who); return RT_E_INVALID; }
    if (!traversal_ok(who, o->traversal)) return RT_E_INVALID;
    if (misaligned(o->stats_device, 8)) { rt_set_error("%s: stats_device is not 8-byte aligned", who); return RT_E_INVALID; }
    return stack_depth_ok(who, scene) ? RT_OK : RT_E_UNSUPPORTED;
}

int rt_trace_rays(rt_scene_t scene, const float *rays, long long n, RtRayHit *hits, RtRaySurface *surface,
                  const RtQueryOptions *opt)
{
    static_assert(sizeof(RtRayHit) == 16 && sizeof(RtRaySurface) == 80, "query records");
    RtQueryOptions o;
    if (!rays || !hits) { rt_set_error("rt_trace_rays: null rays or hits"); return RT_E_INVALID; }
    if (!count_ok("rt_trace_rays", n)) return RT_E_INVALID;
    if (misaligned(rays, 8) || misaligned(hits, 16) || misaligned(surface, 16)) {
        rt_set_error("rt_trace_rays: misaligned pointer (rays 8 B, hits and surface 16 B)");
        return RT_E_INVALID;
    }
    const int rc = query_options("rt_trace_rays", scene, opt, &o);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    rt_register_shutdown();
    hipStream_t stream = (hipStream_t)o.stream;
    return launch_done("rt_trace_rays",
                       rt_launch_trace_rays(scene->dev, rays, n, hits, surface, o.traversal, o.stats_device, stream),
                       stream);
}

int rt_occluded(rt_scene_t scene, const float *rays, const float *tmax, long long n, uint8_t *occluded,
                const RtQueryOptions *opt)
{
    RtQueryOptions o;
    if (!rays || !occluded) { rt_set_error("rt_occluded: null rays or output"); return RT_E_INVALID; }
    if (!count_ok("rt_occluded", n)) return RT_E_INVALID;
    if (misaligned(rays, 8) || misaligned(tmax, 4)) {
        rt_set_error("rt_occluded: misaligned pointer (rays 8 B, tmax 4 B)");
        return RT_E_INVALID;
    }
    const int rc = query_options("rt_occluded", scene, opt, &o);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    rt_register_shutdown();
    hipStream_t stream = (hipStream_t)o.stream;
    return launch_done("rt_occluded",
                       rt_launch_occluded(scene->dev, rays, tmax, n, occluded, o.traversal, o.stats_device, stream),
                       stream);
}

void rt_default_path_options(RtPathOptions *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->samples = 1;
    o->traversal = RT_TRAVERSAL_BOUNDED;
}

int rt_trace_paths(rt_scene_t scene, const float *rays, uint32_t *rng, long long n, float *radiance, float *sq_luminance,
                   const RtPathOptions *opt)
{
    RtPathOptions o;
    if (opt) o = *opt; else rt_default_path_options(&o);
    if (!scene) { rt_set_error("rt_trace_paths: null scene"); return RT_E_INVALID; }
    if (!rays || !rng || !radiance) { rt_set_error("rt_trace_paths: null rays, rng or radiance"); return RT_E_INVALID; }
    if (!count_ok("rt_trace_paths", n)) return RT_E_INVALID;
    if (misaligned(rays, 8) || misaligned(rng, 4) || misaligned(radiance, 4) || misaligned(sq_luminance, 4) ||
        misaligned(o.stats_device, 8)) {
        rt_set_error("rt_trace_paths: misaligned pointer (rays and stats_device 8 B, rng, radiance and sq_luminance 4 B)");
        return RT_E_INVALID;
    }
    if (o.samples < 0 || o.samples > (1 << 20) || o.max_depth < 0 || o.max_depth > RT_WATCHDOG_BOUNCES ||
        (o.accumulate != 0 && o.accumulate != 1)) {
        rt_set_error("rt_trace_paths: samples %d (0 .. 2^20), max_depth %d (0 .. 2^24 - 1) or accumulate %d (0 / 1)",
                     o.samples, o.max_depth, o.accumulate);
        return RT_E_INVALID;
    }
    if (!traversal_ok("rt_trace_paths", o.traversal)) return RT_E_INVALID;
    if (n == 0) return RT_OK;
    if (!stack_depth_ok("rt_trace_paths", scene)) return RT_E_UNSUPPORTED;
    rt_register_shutdown();
    hipStream_t stream = (hipStream_t)o.stream;
    return launch_done("rt_trace_paths",
                       rt_launch_trace_paths(scene->dev, rays, rng, n, radiance, sq_luminance, o.samples ? o.samples : 1,
                                             o.max_depth, o.accumulate, o.traversal, o.stats_device, stream),
                       stream);
}

// rt_trace_paths for rays a sampler draws on the device (sampler_math.h); adaptive: NULL, or the adaptive test's
// constants (rt_render's MIN_SAMPLES / MAX_TOLERANCE) — who: the entry point's name
static int sample_paths(const char *who, rt_scene_t scene, const RtSampler *sampler, uint32_t *rng, long long n,
                        float *radiance, float *sq_luminance, int *sample_count, const RtPathOptions *opt,
                        const RtAdaptive *adaptive)
{
    RtPathOptions o;
    if (opt) o = *opt; else rt_default_path_options(&o);
    if (!scene) { rt_set_error("%s: null scene", who); return RT_E_INVALID; }
    if (!rng || !radiance) { rt_set_error("%s: null rng or radiance", who); return RT_E_INVALID; }
    if (!count_ok(who, n)) return RT_E_INVALID;
    if (misaligned(rng, 4) || misaligned(radiance, 4) || misaligned(sq_luminance, 4) || misaligned(sample_count, 4) ||
        misaligned(o.stats_device, 8)) {
        rt_set_error("%s: misaligned pointer (stats_device 8 B, rng, radiance, sq_luminance and "
                     "sample_count 4 B)", who);
        return RT_E_INVALID;
    }
    if (o.samples < 0 || o.samples > (1 << 20) || o.max_depth < 0 || o.max_depth > RT_WATCHDOG_BOUNCES ||
        (o.accumulate != 0 && o.accumulate != 1)) {
        rt_set_error("%s: samples %d (0 .. 2^20), max_depth %d (0 .. 2^24 - 1) or accumulate %d (0 / 1)", who,
                     o.samples, o.max_depth, o.accumulate);
        return RT_E_INVALID;
    }
    if (!traversal_ok(who, o.traversal)) return RT_E_INVALID;
    RtDevSampler smp;
    if (const char *why = rt_sampler_resolve(sampler, n, &smp)) {
        rt_set_error("%s: %s", who, why);
        return RT_E_INVALID;
    }
    if (adaptive && (!sq_luminance || !sample_count)) {
        rt_set_error("%s: the adaptive test needs sq_luminance and sample_count", who);
        return RT_E_INVALID;
    }
    if (adaptive && adaptive->min_samples < 0) {
        rt_set_error("%s: min_samples %d < 0", who, adaptive->min_samples);
        return RT_E_INVALID;
    }
    if (n == 0) return RT_OK;
    if (!stack_depth_ok(who, scene)) return RT_E_UNSUPPORTED;
    rt_register_shutdown();
    hipStream_t stream = (hipStream_t)o.stream;
    RtCvParams test;
    if (adaptive) test = rt_cv_params(adaptive->min_samples, adaptive->tolerance); // (the tolerance unchecked, as rt_render's)
    return launch_done(who,
                       rt_launch_sample_paths(scene->dev, smp, rng, n, radiance, sq_luminance, sample_count,
                                              o.samples ? o.samples : 1, o.max_depth, o.accumulate, o.traversal,
                                              o.stats_device, stream, adaptive ? &test : nullptr),
                       stream);
}

int rt_sample_paths(rt_scene_t scene, const RtSampler *sampler, uint32_t *rng, long long n, float *radiance,
                    float *sq_luminance, int *sample_count, const RtPathOptions *opt)
{
    return sample_paths("rt_sample_paths", scene, sampler, rng, n, radiance, sq_luminance, sample_count, opt, nullptr);
}

int rt_sample_paths_adaptive(rt_scene_t scene, const RtSampler *sampler, uint32_t *rng, long long n, float *radiance,
                             float *sq_luminance, int *sample_count, const RtPathOptions *opt,
                             const RtAdaptive *adaptive)
{
    return sample_paths(adaptive ? "rt_sample_paths_adaptive" : "rt_sample_paths", scene, sampler, rng, n, radiance,
                        sq_luminance, sample_count, opt, adaptive);
}

int rt_sampler_rays(const RtSampler *sampler, uint32_t *rng, long long n, float *rays, void *stream)
{
    if (!rays || misaligned(rays, 8) || misaligned(rng, 4)) {
        rt_set_error("rt_sampler_rays: null or misaligned rays (8 B), or misaligned rng (4 B)");
        return RT_E_INVALID;
    }
    if (!count_ok("rt_sampler_rays", n)) return RT_E_INVALID;
    RtDevSampler smp;
    if (const char *why = rt_sampler_resolve(sampler, n, &smp)) {
        rt_set_error("rt_sampler_rays: %s", why);
        return RT_E_INVALID;
    }
    if (!rng && smp.kind == RT_SAMPLER_HEMISPHERE) {
        rt_set_error("rt_sampler_rays: a hemisphere sampler has no centre ray (null rng)");
        return RT_E_INVALID;
    }
    if (n == 0) return RT_OK;
    return launch_done("rt_sampler_rays", rt_launch_sampler_rays(smp, rng, n, rays, (hipStream_t)stream),
                       (hipStream_t)stream);
}

// (min_width 2: the camera's half width divides; the denoiser has no camera and takes a 1-pixel column)
static int frame_size_ok(const char *who, int width, int height, int min_width = 2)
{
    if (width < min_width || height <= 0 || (long long)width * height > (1LL << 31) - 1) {
        rt_set_error("%s: bad frame size %d x %d", who, width, height);
        return RT_E_INVALID;
    }
    return RT_OK;
}

int rt_camera_rays(Camera cam, int width, int height, float *rays, void *stream)
{
    if (!rays || misaligned(rays, 8)) { rt_set_error("rt_camera_rays: null or misaligned rays"); return RT_E_INVALID; }
    const int rc = frame_size_ok("rt_camera_rays", width, height);
    if (rc != RT_OK) return rc;
    return launch_done("rt_camera_rays",
                       rt_launch_camera_rays(rt_device_camera(cam), width, height, rays, (hipStream_t)stream),
                       (hipStream_t)stream);
}

int rt_render_aov(rt_scene_t scene, Camera cam, int width, int height, const RtAovBuffers *b, const RtQueryOptions *opt)
{
    RtQueryOptions o;
    if (!b) { rt_set_error("rt_render_aov: null buffers"); return RT_E_INVALID; }
    if (misaligned(b->depth, 4) || misaligned(b->normal, 4) || misaligned(b->albedo, 4) || misaligned(b->triangle, 4)) {
        rt_set_error("rt_render_aov: misaligned buffer");
        return RT_E_INVALID;
    }
    int rc = frame_size_ok("rt_render_aov", width, height);
    if (rc != RT_OK) return rc;
    rc = query_options("rt_render_aov", scene, opt, &o);
    if (rc != RT_OK) return rc;
    if (!b->depth && !b->normal && !b->albedo && !b->triangle && !o.stats_device) return RT_OK; // nothing asked for
    rt_register_shutdown();
    hipStream_t stream = (hipStream_t)o.stream;
    return launch_done("rt_render_aov",
                       rt_launch_render_aov(scene->dev, rt_device_camera(cam), width, height, b->depth, b->normal,
                                            b->albedo, b->triangle, o.traversal, o.stats_device, stream),
                       stream);
}

int rt_sample_aov(rt_scene_t scene, const RtSampler *sampler, long long n, const RtAovBuffers *b, const RtQueryOptions *opt)
{
    RtQueryOptions o;
    if (!b) { rt_set_error("rt_sample_aov: null buffers"); return RT_E_INVALID; }
    if (misaligned(b->depth, 4) || misaligned(b->normal, 4) || misaligned(b->albedo, 4) || misaligned(b->triangle, 4)) {
        rt_set_error("rt_sample_aov: misaligned buffer");
        return RT_E_INVALID;
    }
    if (!count_ok("rt_sample_aov", n)) return RT_E_INVALID;
    RtDevSampler smp;
    if (const char *why = rt_sampler_resolve(sampler, n, &smp)) {
        rt_set_error("rt_sample_aov: %s", why);
        return RT_E_INVALID;
    }
    if (smp.kind == RT_SAMPLER_HEMISPHERE) {
        rt_set_error("rt_sample_aov: a hemisphere sampler has no centre ray");
        return RT_E_INVALID;
    }
    const int rc = query_options("rt_sample_aov", scene, opt, &o);
    if (rc != RT_OK) return rc;
    if (n == 0) return RT_OK;
    if (!b->depth && !b->normal && !b->albedo && !b->triangle && !o.stats_device) return RT_OK; // nothing asked for
    rt_register_shutdown();
    hipStream_t stream = (hipStream_t)o.stream;
    return launch_done("rt_sample_aov",
                       rt_launch_sample_aov(scene->dev, smp, n, b->depth, b->normal, b->albedo, b->triangle, o.traversal,
                                            o.stats_device, stream),
                       stream);
}

int rt_tonemap(G_Buffer g, uint8_t *rgba, int w, int h, void *stream)
{
    if (!rgba || !g.frame_buffer || !g.sample_count || w <= 0 || h <= 0) {
        rt_set_error("rt_tonemap: bad arguments");
        return RT_E_INVALID;
    }
    const int jr = join_status(stream, "rt_tonemap"); // chained renders' deep-path tails first
    if (jr != RT_OK) return jr;
    return launch_done("rt_tonemap",
                       rt_launch_tonemap(g.frame_buffer, g.sample_count, (RtUChar4 *)rgba, w * h, (hipStream_t)stream),
                       (hipStream_t)stream);
}

// ---------------- convergence (convergence.hip; rt_convergence_host: host/convergence_host.cpp) ----------------
int rt_convergence(const float *radiance, const float *sq_luminance, const int *sample_count, long long n,
                   int min_samples, float tolerance, float *rel_error, unsigned long long *stats, void *stream)
{
    if (const char *why = rt_cv_check(radiance, sq_luminance, sample_count, n, min_samples, rel_error)) {
        rt_set_error("rt_convergence: %s", why);
        return RT_E_INVALID;
    }
    if (misaligned(stats, 8)) { rt_set_error("rt_convergence: stats_device is not 8-byte aligned"); return RT_E_INVALID; }
    if (n == 0) return RT_OK;
    const int jr = join_status(stream, "rt_convergence"); // chained renders' deep-path tails first, as rt_tonemap
    if (jr != RT_OK) return jr;
    return launch_done("rt_convergence",
                       rt_launch_convergence(radiance, sq_luminance, sample_count, n, rt_cv_params(min_samples, tolerance),
                                             rel_error, stats, (hipStream_t)stream),
                       (hipStream_t)stream);
}

// ---------------- denoising (denoise.hip; rt_denoise_host and the default options: host/denoise_host.cpp) ----------------
// rt_denoise and rt_denoise_sampler (who; sampler: NULL, or the frame's sampler — its size is the frame's, and an
// EQUIRECT one makes the x axis periodic)
static int denoise(const char *who, G_Buffer g, const RtAovBuffers *aov, const RtSampler *sampler, int width, int height,
                   float *rgb_out, const RtDenoiseOptions *opt)
{
    RtDnParams prm;
    if (!rt_dn_resolve(opt, &prm)) {
        rt_set_error("%s: option out of range (iterations 1..%d, normal_log2 1..%d, demodulate -1..1, "
                     "sigmas finite and >= 0)", who, RT_DN_MAX_ITERATIONS, RT_DN_MAX_NORMAL_LOG2);
        return RT_E_INVALID;
    }
    if (!g.frame_buffer || !g.squared_luminance || !g.sample_count || !rgb_out || !aov || !aov->depth ||
        !aov->normal || (prm.demodulate && !aov->albedo)) {
        rt_set_error("%s: null G_Buffer array, AOV buffer or output", who);
        return RT_E_INVALID;
    }
    if (misaligned(rgb_out, 4) || misaligned(aov->depth, 4) || misaligned(aov->normal, 4) || misaligned(aov->albedo, 4)) {
        rt_set_error("%s: misaligned buffer", who);
        return RT_E_INVALID;
    }
    int wrap_x = 0;
    if (sampler) {
        RtDevSampler smp;
        if (const char *why = rt_sampler_resolve_frame(sampler, &smp)) {
            rt_set_error("%s: %s", who, why);
            return RT_E_INVALID;
        }
        width = smp.width;
        height = smp.height;
        wrap_x = smp.kind == RT_SAMPLER_EQUIRECT;
    }
    const int rc = frame_size_ok(who, width, height, 1);
    if (rc != RT_OK) return rc;
    hipStream_t stream = (hipStream_t)(opt ? opt->stream : nullptr);
    const int jr = join_status(stream, who); // chained renders' deep-path tails first, as rt_tonemap
    if (jr != RT_OK) return jr;
    rt_register_shutdown();
    return launch_done(who,
                       rt_launch_denoise(g.frame_buffer, g.squared_luminance, g.sample_count, aov->depth, aov->normal,
                                         aov->albedo, width, height, rgb_out, prm, stream, wrap_x),
                       stream);
}

int rt_denoise(G_Buffer g, const RtAovBuffers *aov, int width, int height, float *rgb_out, const RtDenoiseOptions *opt)
{
    return denoise("rt_denoise", g, aov, nullptr, width, height, rgb_out, opt);
}

int rt_denoise_sampler(G_Buffer g, const RtAovBuffers *aov, const RtSampler *sampler, float *rgb_out,
                       const RtDenoiseOptions *opt)
{
    if (!sampler) { rt_set_error("rt_denoise_sampler: null sampler"); return RT_E_INVALID; }
    return denoise("rt_denoise_sampler", g, aov, sampler, 0, 0, rgb_out, opt);
}

// ---------------- temporal reprojection (reproject.hip; rt_reproject_host and the default options:
// host/reproject_host.cpp) ----------------
// rt_reproject and rt_reproject_sampler (who) on the two views' frame constants; model: RT_SAMPLER_PINHOLE ..
// RT_SAMPLER_ORTHO
static int reproject(const char *who, G_Buffer src, const RtAovBuffers *sa, const RtDevCamera &src_cam,
                     const RtAovBuffers *da, const RtDevCamera &dst_cam, int model, const RtRpLens &lens, int width,
                     int height, G_Buffer dst, const RtReprojectOptions *opt, const RtRpParams &prm)
{
    if (!src.frame_buffer || !src.squared_luminance || !src.sample_count || !dst.frame_buffer ||
        !dst.squared_luminance || !dst.sample_count || !sa || !da || !sa->depth || !sa->normal || !da->depth ||
        !da->normal) {
        rt_set_error("%s: null G_Buffer array or AOV buffer", who);
        return RT_E_INVALID;
    }
    if (misaligned(sa->depth, 4) || misaligned(sa->normal, 4) || misaligned(sa->triangle, 4) ||
        misaligned(da->depth, 4) || misaligned(da->normal, 4) || misaligned(da->triangle, 4) ||
        misaligned(opt ? opt->stats_device : nullptr, 8)) {
        rt_set_error("%s: misaligned buffer", who);
        return RT_E_INVALID;
    }
    const int rc = frame_size_ok(who, width, height, 1);
    if (rc != RT_OK) return rc;
    if (rt_rp_frames_overlap(src.frame_buffer, src.squared_luminance, src.sample_count, dst.frame_buffer,
                             dst.squared_luminance, dst.sample_count, (size_t)width * height)) {
        rt_set_error("%s: dst's arrays overlap src's (the call is a gather)", who);
        return RT_E_INVALID;
    }
    hipStream_t stream = (hipStream_t)(opt ? opt->stream : nullptr);
    const int jr = join_status(stream, who); // chained renders' deep-path tails first, as rt_tonemap
    if (jr != RT_OK) return jr;
    rt_register_shutdown();
    const RtRpFrame sf = {src.frame_buffer, src.squared_luminance, src.sample_count, sa->depth, sa->normal, sa->triangle};
    return launch_done(who,
                       rt_launch_reproject(sf, src_cam, da->depth, da->normal, da->triangle, dst_cam, width, height, prm,
                                           dst.frame_buffer, dst.squared_luminance, dst.sample_count,
                                           opt ? opt->stats_device : nullptr, stream, model, lens),
                       stream);
}

static bool reproject_options_ok(const char *who, const RtReprojectOptions *opt, RtRpParams *prm)
{
    if (rt_rp_resolve(opt, prm)) return true;
    rt_set_error("%s: option out of range (max_history 1..%d, match_triangle -1..1, depth_tol finite "
                 "and >= 0, normal_min in (-1, 1])", who, RT_RP_MAX_HISTORY);
    return false;
}

int rt_reproject(G_Buffer src, const RtAovBuffers *sa, Camera src_cam, const RtAovBuffers *da, Camera dst_cam, int width,
                 int height, G_Buffer dst, const RtReprojectOptions *opt)
{
    RtRpParams prm;
    if (!reproject_options_ok("rt_reproject", opt, &prm)) return RT_E_INVALID;
    return reproject("rt_reproject", src, sa, rt_rp_camera(src_cam), da, rt_rp_camera(dst_cam), RT_SAMPLER_PINHOLE,
                     RtRpLens{0.0f, 0.0f, 0.0f, 0.0f}, width, height, dst, opt, prm);
}

int rt_reproject_sampler(G_Buffer src, const RtAovBuffers *sa, const RtSampler *src_sampler, const RtAovBuffers *da,
                         const RtSampler *dst_sampler, G_Buffer dst, const RtReprojectOptions *opt)
{
    RtRpParams prm;
    if (!reproject_options_ok("rt_reproject_sampler", opt, &prm)) return RT_E_INVALID;
    RtDevSampler ss, ds;
    if (const char *why = rt_rp_resolve_samplers(src_sampler, dst_sampler, &ss, &ds)) {
        rt_set_error("rt_reproject_sampler: %s", why);
        return RT_E_INVALID;
    }
    return reproject("rt_reproject_sampler", src, sa, ss.cam, da, ds.cam, ds.kind, rt_rp_lens(ss, ds), ds.width, ds.height,
                     dst, opt, prm);
}

int rt_tonemap_rgb(const float *rgb, uint8_t *rgba, int w, int h, void *stream)
{
    if (!rgb || !rgba || misaligned(rgb, 4) || misaligned(rgba, 4)) {
        rt_set_error("rt_tonemap_rgb: null or misaligned buffer");
        return RT_E_INVALID;
    }
    const int rc = frame_size_ok("rt_tonemap_rgb", w, h, 1);
    if (rc != RT_OK) return rc;
    return launch_done("rt_tonemap_rgb", rt_launch_tonemap_rgb(rgb, (RtUChar4 *)rgba, w * h, (hipStream_t)stream),
                       (hipStream_t)stream);
}

// save_render (rt/save_render.cuh:25-67): tonemap on the GPU, flip rows, PNG
int rt_save_render(G_Buffer g, int w, int h, const char *path)
{
    if (!path || w <= 0 || h <= 0) { rt_set_error("rt_save_render: bad arguments"); return RT_E_INVALID; }
    const size_t n = (size_t)w * h;
    uint8_t *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, n * 4));
    int rc = rt_tonemap(g, d, w, h, nullptr);
    std::vector<uint8_t> img(n * 4), flipped(n * 4);
    if (rc == RT_OK && hipMemcpy(img.data(), d, n * 4, hipMemcpyDeviceToHost) != hipSuccess) {
        rt_set_error("rt_save_render: download failed");
        rc = RT_E_HIP;
    }
    (void)hipFree(d);
    if (rc) return rc;
    for (int y = 0; y < h; ++y) // flipped_pixel_index = (H - y - 1) * W + x  (:55)
        memcpy(&flipped[(size_t)(h - y - 1) * w * 4], &img[(size_t)y * w * 4], (size_t)w * 4);
    return rt_host::write_png(path, flipped.data(), w, h);
}

int rt_write_png(const char *path, const uint8_t *rgba, int w, int h)
{
    if (!path || !rgba || w <= 0 || h <= 0) { rt_set_error("rt_write_png: bad arguments"); return RT_E_INVALID; }
    return rt_host::write_png(path, rgba, w, h);
}

} // extern "C"
