/*
 * isaklm_rt.h — C-ABI of the MI355X-native path-tracing hot path.
 *
 * Drop-in boundary for INDA23PlusPlus/isaklm-raytracer's render path
 * (SURVEY §8b).  Paths below are relative to /root/reference/isaklm-raytracer
 * and abbreviated "rt/".
 *
 *   reference                                   this ABI
 *   -------------------------------------------------------------------------
 *   cudaMalloc / cudaMemcpy on the host path     rt_device_alloc / rt_upload /
 *     (rt/create_scene.cuh:33-34,62-63,            rt_download / rt_free
 *      rt/create_kd_tree.cuh:319-324,
 *      rt/scene.cuh:58-59, rt/screen.cuh:24-45)
 *   G_Buffer::G_Buffer()  rt/screen.cuh:22-46     rt_gbuffer_create / rt_gbuffer_seeds
 *   load_mesh()           rt/mesh_loading.cuh:221 rt_host_scene_load_mesh
 *   create_models()       rt/create_models.cuh:17 rt_host_scene_load_file (scene text file)
 *   create_kd_tree()      rt/create_kd_tree.cuh:267  rt_build_kd_tree
 *   create_scene()        rt/create_scene.cuh:18  rt_create_scene
 *   (new) device re-layout                        rt_scene_prepare
 *   render()              rt/render.cuh:62        rt_render
 *   reset_frame<<<>>>     rt/render.cuh:18        (inside rt_render, sample_count==0)
 *   draw_frame<<<>>>      rt/render.cuh:37        rt_tonemap (into an HBM RGBA8 buffer)
 *   save_render()         rt/save_render.cuh:25   rt_save_render (PNG, same flip)
 *
 * Conventions: every function returns 0 on success and a negative RT_E_*
 * code otherwise (rt_last_error() describes the last failure of the calling
 * thread).  Pointers named *_device are HIP device pointers.  The caller owns
 * every allocation and frees it explicitly (the reference leaks; see
 * rt/screen.cuh:24-31); rt_shutdown releases the library's own per-device
 * workspaces (it is also registered to run at exit).  Calls are synchronous
 * unless an RtOptions.stream is given, in which case the default render (the
 * bounded traversal, one persistent finisher per call) and the megakernel
 * only enqueue; the queue variants (RT_TRAVERSAL_KD, counting calls) block the
 * calling thread until their queue iterations are done (their host threads
 * read each iteration's live path count).  Consecutive calls may use
 * different streams: a call waits for the previous calls' device work first
 * (they share the per-device workspace) — except a chained call
 * (RtOptions.overlap), see there.  Calls on one device from several host
 * threads are serialised by the library.
 */
#ifndef ISAKLM_RT_H
#define ISAKLM_RT_H

#include <stddef.h>
#include <stdint.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version: 3 = rt_scene_prepare(const Scene *, rt_scene_t *) without
 * counts (the counted form is rt_scene_prepare_counts), RtDeviations and
 * rt_deviation_stats, rt_abi_version; 4 = RT_CNT_COUNT 40 (the optional
 * counters buffer grew); 5 = RtOptions.traversal; 6 = RtOptions.overlap /
 * check_interval / debug, RtDeviations' bounded-traversal guard fields,
 * rt_join, rt_shutdown; 7 = RtDeviations' hand-off fields (owed passes,
 * safety-net exits, stranded pixels, dropped guard records, linger
 * expiries), RT_E_INCOMPLETE from the joins, rt_profile_history; 8 =
 * RtDeviations.long_closed, RtOptions.coalesce_passes (both structs grew);
 * 9 = RtDeviations.wide_overflows (the struct grew), RT_DEBUG_WIDE_CAP1,
 * RT_DEBUG_COUNT_LONG_ONLY; 10 = the ray-query API (rt_trace_rays,
 * rt_camera_rays, rt_render_aov, RtRayHit, RtRaySurface, RtQueryOptions,
 * RtAovBuffers): an addition only; 11 = the denoiser (rt_denoise,
 * rt_denoise_host, rt_default_denoise_options, RtDenoiseOptions) and
 * rt_tonemap_rgb: additions only; 12 = the occlusion query (rt_occluded):
 * an addition only.  The radiance query (rt_trace_paths, RtPathOptions,
 * rt_default_path_options) was added within version 12 — new symbols and a
 * new struct, nothing existing moved; RT_HAS_TRACE_PATHS is its compile-time
 * feature test.  Temporal reprojection (rt_reproject, rt_reproject_host,
 * rt_default_reproject_options, RtReprojectOptions) was added within version
 * 12 in the same way; RT_HAS_REPROJECT is its feature test.  So were the
 * path samplers (rt_sample_paths, rt_sampler_rays, rt_sampler_rays_host,
 * RtSampler); RT_HAS_PATH_SAMPLERS is their feature test.  So were the
 * adaptive samplers (rt_sample_paths_adaptive, RtAdaptive;
 * RT_HAS_ADAPTIVE_SAMPLERS) and the convergence query (rt_convergence,
 * rt_convergence_host; RT_HAS_CONVERGENCE): new symbols, no struct grew.
 * An integrator checks
 * rt_abi_version() == RT_ABI_VERSION at start-up: a binary built against an
 * older header would otherwise link (C linkage) and mis-pass arguments. */
#define RT_ABI_VERSION 12

/* CUDA uchar4, used for texels (rt/scene.cuh:18) */
typedef struct RtUChar4 { uint8_t x, y, z, w; } RtUChar4;

/* ---------------- reference-layout types (byte-identical) ----------------
 * A C++ caller that brings the reference's own types — the reference is one
 * translation unit (rt/main.cu:8-14) whose headers define Vec2D, Vec3D
 * (rt/math_library.cuh:55,99), Texture, Material, Triangle, KD_Tree_Node,
 * Bounding_Box, KD_Tree, Scene (rt/scene.cuh:16-121), G_Buffer
 * (rt/screen.cuh:15) and Camera (rt/camera.cuh:15) — defines
 * ISAKLM_RT_CALLER_TYPES before including this header.  The definitions
 * below are then replaced by forward declarations, so the header can come
 * BEFORE those types (G_Buffer's constructor, rt/screen.cuh:22-46, already
 * calls the allocation functions) or after them; the functions take the
 * caller's types (C linkage: type names do not enter the symbols).  Once all
 * of them are defined, the caller writes ISAKLM_RT_CHECK_LAYOUT(); at
 * namespace scope: the static_asserts of the byte layout this library
 * assumes.  See INTEGRATION.md and tests/native/ref_main_shape.cpp. */
#ifdef ISAKLM_RT_CALLER_TYPES
#ifndef __cplusplus
#error "ISAKLM_RT_CALLER_TYPES: the reference's types are C++ (anonymous unions, constructors)"
#endif
struct Vec2D;
struct Vec3D;
struct Texture;
struct Material;
struct Triangle;
struct KD_Tree_Node;
struct Bounding_Box;
struct KD_Tree;
struct Scene;
struct G_Buffer;
struct Camera;
#else

/* rt/math_library.cuh:71-82 (union {x,u},{y,v}) */
typedef struct Vec2D { float x, y; } Vec2D;
/* rt/math_library.cuh:115-131 (union {x,r},{y,g},{z,b}) */
typedef struct Vec3D { float x, y, z; } Vec3D;

/* rt/scene.cuh:16-21 */
typedef struct Texture {
    RtUChar4 *buffer; /* device RGBA8 texels, NULL = no texture */
    int width;
    int height;
} Texture;

/* rt/scene.cuh:65-74 */
typedef struct Material {
    Vec3D albedo;
    Vec3D emittance;
    float roughness;
    float refractive_index;
    float extinction;
    bool transparent;
    Texture texture;
} Material;

/* rt/scene.cuh:76-82 */
typedef struct Triangle {
    Vec3D p1, p2, p3;
    Vec3D n1, n2, n3;
    Vec2D uv1, uv2, uv3;
    Material material;
} Triangle;

/* rt/scene.cuh:84-100 */
typedef struct KD_Tree_Node {
    union { int index_offset; int child_index1; };
    union { int triangle_count; int child_index2; };
    uint8_t plane_axis;
    float plane_offset;
    bool is_leaf_node;
} KD_Tree_Node;

/* rt/scene.cuh:102-105 */
typedef struct Bounding_Box { Vec3D min, max; } Bounding_Box;

/* rt/scene.cuh:107-112 */
typedef struct KD_Tree {
    Bounding_Box bounding_box;
    KD_Tree_Node *nodes;       /* device, pre-order (rt/create_kd_tree.cuh:286-298) */
    int *triangle_indicies;    /* device (rt/create_kd_tree.cuh:300-312) */
} KD_Tree;

/* rt/scene.cuh:114-121 */
typedef struct Scene {
    Triangle *triangles;       /* device AoS */
    int triangle_count;
    int *light_indicies;       /* device */
    int light_count;
    KD_Tree kd_tree;
} Scene;

/* rt/screen.cuh:15-21 (per-pixel SoA device arrays, row-major, row 0 = bottom) */
typedef struct G_Buffer {
    Vec3D *frame_buffer;
    float *squared_luminance;
    int *sample_count;
    uint32_t *random_numbers;
} G_Buffer;

/* rt/camera.cuh:15-26 */
typedef struct Camera {
    Vec3D position;
    float yaw, pitch;
    float FOV;
    float aperture_radius;
} Camera;

#endif /* ISAKLM_RT_CALLER_TYPES */

#ifdef __cplusplus
/* the reference's byte layout */
#define ISAKLM_RT_CHECK_LAYOUT()                                                                              \
static_assert(sizeof(Vec2D) == 8, "Vec2D"); \
static_assert(sizeof(Vec3D) == 12, "Vec3D"); \
static_assert(sizeof(Texture) == 16, "Texture"); \
static_assert(sizeof(Material) == 56 && offsetof(Material, roughness) == 24 && \
              offsetof(Material, transparent) == 36 && offsetof(Material, texture) == 40, "Material"); \
static_assert(sizeof(Triangle) == 152 && offsetof(Triangle, n1) == 36 && offsetof(Triangle, uv1) == 72 && \
              offsetof(Triangle, material) == 96, "Triangle"); \
static_assert(sizeof(KD_Tree_Node) == 20 && offsetof(KD_Tree_Node, plane_axis) == 8 && \
              offsetof(KD_Tree_Node, plane_offset) == 12 && offsetof(KD_Tree_Node, is_leaf_node) == 16, \
              "KD_Tree_Node"); \
static_assert(sizeof(Bounding_Box) == 24, "Bounding_Box"); \
static_assert(sizeof(KD_Tree) == 40, "KD_Tree"); \
static_assert(sizeof(Scene) == 72 && offsetof(Scene, light_indicies) == 16 && offsetof(Scene, kd_tree) == 32, \
              "Scene"); \
static_assert(sizeof(G_Buffer) == 32, "G_Buffer"); \
static_assert(sizeof(Camera) == 28 && offsetof(Camera, FOV) == 20, "Camera");
#ifndef ISAKLM_RT_CALLER_TYPES
ISAKLM_RT_CHECK_LAYOUT()
#endif
#endif

/* ---------------- status codes ---------------- */
#define RT_OK 0
#define RT_E_INVALID (-1)   /* bad argument / shape */
#define RT_E_HIP (-2)       /* HIP runtime failure */
#define RT_E_IO (-3)        /* file could not be read / written */
#define RT_E_PARSE (-4)     /* malformed OBJ / .mat / scene file */
#define RT_E_UNSUPPORTED (-5) /* e.g. KD tree deeper than the traversal stack */
#define RT_E_NOMEM (-6)
#define RT_E_INCOMPLETE (-7) /* a join found pixels whose deep-path samples never came back
                              * (RtDeviations.stranded_pixels): the frame misses passes */

const char *rt_last_error(void);
const char *rt_version(void);
int rt_abi_version(void); /* RT_ABI_VERSION of the built library */

/* ---------------- texture decoding ----------------
 * stbi_load(path, &w, &h, &n, 4) as make_texture (rt/scene.cuh:25-63) calls
 * it: RGBA8 rows in file order (no flip).  PNG (all colour types / depths,
 * Adam7, tRNS) and baseline / extended-sequential / progressive JPEG,
 * bit-identical to stb_image v2.28; other formats -> RT_E_UNSUPPORTED.
 * The pixels are a host array (rt_host_free).  rt_host_scene_load_mesh decodes
 * a material's `texture` with it, and rt_create_scene uploads each texture
 * with width + 1 zero texels after the image: mod(uv, 1) can return 1.0, so
 * sample_texture's index reaches width*height + width.  Callers
 * of rt_scene_prepare_host that supply their own device texels should pad
 * them the same way. */
int rt_decode_image(const char *path, uint8_t **rgba_out, int *width, int *height);
int rt_decode_image_memory(const void *data, size_t size, uint8_t **rgba_out, int *width, int *height);

/* ---------------- device memory (hipMalloc/hipMemcpy stand-ins) ---------------- */
int rt_device_alloc(void **ptr_device, size_t bytes);
int rt_free(void *ptr_device);
int rt_upload(void *dst_device, const void *src_host, size_t bytes);
int rt_download(void *dst_host, const void *src_device, size_t bytes);
int rt_memset(void *dst_device, int value, size_t bytes);
int rt_device_count(int *count);
/* selects the device for the calling thread and creates the wavefront
 * pipelines' streams there (call it before other GPU users of the process,
 * e.g. RCCL, take the hardware queues) */
int rt_set_device(int device);
/* hipDeviceSynchronize after rt_join(NULL): chained renders are complete */
int rt_synchronize(void);
/* `stream` (NULL: the calling thread) waits for every rt_render's device work
 * on the current device, including the deep-path tails that chained calls
 * (RtOptions.overlap) leave running past their stream point (an open chain is
 * drained first: one more finisher launch for the pixels still owed passes).
 * After the drain every pixel handed to the long-path kernel must be back; a
 * check kernel verifies it (and releases any that are not).  Host joins
 * (NULL, and rt_synchronize, rt_download, rt_tonemap / rt_save_render without
 * a stream, rt_gbuffer_save) return RT_E_INCOMPLETE if that check — theirs or
 * an earlier stream join's — found stranded pixels; RtDeviations counts them. */
int rt_join(void *stream);
/* releases the library's per-device workspaces (streams, events, device
 * buffers) after their device work is done; registered with atexit by
 * rt_set_device / the first render.  Renders after it create them again. */
void rt_shutdown(void);
void rt_host_free(void *ptr_host);  /* frees host arrays returned by this library */

/* ---------------- G_Buffer (rt/screen.cuh:22-46) ---------------- */
/* outputs [skip, skip+count) of std::mt19937 (default seed 5489) through
 * uniform_int_distribution<uint32_t>(0, UINT32_MAX), i.e. the raw engine words
 * (rt/screen.cuh:34-45).  Shard g of an spp-sliced render uses skip = g*W*H. */
int rt_gbuffer_seeds(uint32_t *host_out, size_t count, uint64_t skip);
/* allocates the four arrays for width*height pixels, zeroes fb/sq/count
 * (the reference leaves them uninitialised until reset_frame) and uploads the
 * seeds */
int rt_gbuffer_create(int width, int height, uint64_t seed_skip, G_Buffer *out);
int rt_gbuffer_destroy(G_Buffer *g);
/* checkpoint / resume: the G_Buffer is a frame's whole
 * progressive state (the reference keeps it in device memory only).  Save it
 * with the caller's sample count; loading it into a G_Buffer of the same size
 * and calling rt_render with that sample count continues the render bit for
 * bit.  Errors: RT_E_IO (file), RT_E_PARSE (not a checkpoint / truncated),
 * RT_E_INVALID (size mismatch). */
int rt_gbuffer_save(G_Buffer g_buffer, int width, int height, int sample_count, const char *path);
int rt_gbuffer_load(const char *path, G_Buffer g_buffer, int width, int height, int *sample_count_out);

/* ---------------- host scene path ---------------- */
typedef struct RtHostScene RtHostScene;
int rt_host_scene_create(RtHostScene **out);
void rt_host_scene_destroy(RtHostScene *scene);
/* load_mesh (rt/mesh_loading.cuh:221-440): appends the OBJ's triangles,
 * materials from the .mat file, re-centred on the mesh AABB and transformed by
 * `matrix` (column vectors i,j,k = matrix[0..2],[3..5],[6..8]) + `offset`. */
int rt_host_scene_load_mesh(RtHostScene *scene, const char *obj_path, const char *mat_path,
                            const float offset[3], const float matrix[9], int smooth_normals);
/* scene text file: "mesh <obj> <mat> ox oy oz yaw pitch scale smooth" lines
 * (create_models' rotation_matrix(yaw,pitch)*scale transforms,
 * rt/create_models.cuh:21-39) and one "camera px py pz yaw pitch fov aperture"
 * line (rt/main.cu:101-104).  Relative paths resolve against the file's dir. */
int rt_host_scene_load_file(RtHostScene *scene, const char *scene_path, Camera *camera_out);
int rt_host_scene_triangles(const RtHostScene *scene, const Triangle **triangles, int *count);
/* Synthetic scenes for BASELINE.json's configs (the reference's OBJ models
 * are unpublished): writes OBJ + .mat + scene.txt into out_dir and
 * returns the scene.txt path.  Names: cornell (cfg 1), cornell_blob (cfg 2),
 * room2m (cfg 3/4), room2m_glass (cfg 5), room_small (tests). */
int rt_generate_scene(const char *name, const char *out_dir, char *scene_path_out, size_t cap);

/* create_kd_tree (rt/create_kd_tree.cuh:267-328) on the host: identical tree,
 * node numbering and index order.  Outputs are host arrays (rt_host_free). */
int rt_build_kd_tree(const Triangle *host_triangles, int triangle_count, KD_Tree_Node **nodes_out,
                     int *node_count, int **indices_out, int *index_count, Bounding_Box *bounds_out);

/* create_scene (rt/create_scene.cuh:18-73): uploads triangles, the light list
 * and the KD tree into a reference-layout device Scene. */
int rt_create_scene(const RtHostScene *scene, Scene *out, int *node_count, int *index_count);
int rt_destroy_scene(Scene *scene);

/* ---------------- prepared (MI355X-layout) scene ---------------- */
typedef struct RtPreparedScene *rt_scene_t;
/* Re-lays a reference-layout device Scene into the traversal layout (SoA
 * nodes, precomputed triangle planes).  Bit-preserving: every precomputed
 * value is the reference's own expression evaluated once.  Takes the Scene
 * exactly as the reference's `Scene create_scene()` (rt/create_scene.cuh:
 * 18-73) returns it: the KD node and index counts, which Scene does not carry
 * (rt/scene.cuh:107-121), are recovered by walking the device tree
 * pre-order from node 0 within its device allocation.  The arrays must be
 * device allocations of this process (rt_device_alloc / hipMalloc). */
int rt_scene_prepare(const Scene *device_scene, rt_scene_t *out);
/* the same with the counts given (e.g. memory from a sub-allocator that
 * hipMemGetAddressRange cannot bound) */
int rt_scene_prepare_counts(const Scene *device_scene, int node_count, int index_count, rt_scene_t *out);
/* same from host arrays (skips a device round trip) */
int rt_scene_prepare_host(const Triangle *triangles, int triangle_count, const KD_Tree_Node *nodes,
                          int node_count, const int *indices, int index_count, const int *lights,
                          int light_count, Bounding_Box bounds, rt_scene_t *out);
int rt_scene_release(rt_scene_t scene);
/* device bytes held by the prepared scene */
int rt_scene_info(rt_scene_t scene, size_t *device_bytes, int *triangle_count, int *node_count,
                  int *index_count, int *max_depth);

/* ---------------- render (rt/render.cuh:62-76) ---------------- */
/* work counters (SURVEY §8d algorithmic bytes) */
enum {
    RT_CNT_NODE = 0,   /* KD node fetches */
    RT_CNT_TRI = 1,    /* triangle tests */
    RT_CNT_HIT = 2,    /* closest-hit shadings */
    RT_CNT_TEXEL = 3,  /* texel reads */
    RT_CNT_NEE = 4,    /* next-event estimations */
    RT_CNT_SAMPLE = 5, /* samples traced */
    RT_CNT_SKIP = 6,   /* pixel-passes skipped by the adaptive test */
    RT_CNT_RAY = 7,    /* trace_ray calls */
    RT_CNT_WATCHDOG = 8, /* paths cut by the bounce watchdog */
    RT_CNT_MAXDEPTH = 9, /* longest path (extension rays) seen: atomic max, not a sum */
    /* the part of NODE / TRI / RAY done by the wavefront finisher launch
     * (already included in the totals above) */
    RT_CNT_FIN_NODE = 10,
    RT_CNT_FIN_TRI = 11,
    RT_CNT_FIN_RAY = 12,
    /* cooperative traversal diagnostics: plane-test prescreen survivors and
     * exact plane-test passes (barycentric tests) */
    RT_CNT_CAND = 13,
    RT_CNT_PLANE = 14,
    /* traversal pushes at stack index >= 19: each would write past the
     * reference's 19-entry stack arrays (rt/trace_ray.cuh:246-248);
     * reference-comparable, the oracle counts the same */
    RT_CNT_DEEP_PUSH = 15,
    /* cooperative trace, counting build only: wave-time (shader clocks,
     * summed over waves) in descent / leaf tests / ray fetch, and the number
     * of rounds, 64-entry plane chunks and barycentric batches */
    RT_CNT_T_DESCEND = 16,
    RT_CNT_T_LEAVES = 17,
    RT_CNT_T_FETCH = 18,
    RT_CNT_ROUNDS = 19,
    RT_CNT_CHUNKS = 20,
    RT_CNT_BARY = 21,
    /* finisher, counting build only: wide_trace calls / rounds / wave-time */
    RT_CNT_WIDE_CALLS = 22,
    RT_CNT_WIDE_ROUNDS = 23,
    RT_CNT_T_WIDE = 24,
    RT_CNT_T_WIDE_LOAD = 25,   /* wide_trace phases: frontier + node load, */
    RT_CNT_T_WIDE_LEAF = 26,   /* leaf batch, */
    RT_CNT_T_WIDE_EXPAND = 27, /* expansion */
    /* cooperative leaf test, counting build only: wave-time in the chunk
     * loop's plane-load wait, chunk set-up (owner scan, next load issue),
     * plane test + candidate append, and the barycentric stages */
    RT_CNT_T_LEAF_WAIT = 28,
    RT_CNT_T_LEAF_SETUP = 29,
    RT_CNT_T_LEAF_TEST = 30,
    RT_CNT_T_LEAF_BARY = 31,
    /* cooperative trace, counting build only: traversal-stack pushes and
     * pops beyond the LDS part of the stack (HBM spill), pending lanes summed
     * over the wave's leaf tests and the number of those tests, and the
     * descent's wave-time waiting for node loads */
    RT_CNT_SPILL_PUSH = 32,
    RT_CNT_SPILL_POP = 33,
    RT_CNT_PEND_LANES = 34,
    RT_CNT_LEAF_TESTS = 35,
    RT_CNT_T_DESC_WAIT = 36,
    /* RtOptions.traversal = RT_TRAVERSAL_BOUNDED_COUNTED only: the bounded
     * queue trace kernel's own work (RT_CNT_NODE / _TRI then count its KD
     * nodes / plane tests): BVH nodes, BVH plane tests, and the barycentric
     * records read by both phases */
    RT_CNT_B_BVH_NODE = 37,
    RT_CNT_B_BVH_TRI = 38,
    RT_CNT_B_BARY = 39,
    RT_CNT_COUNT = 40
};

#define RT_KERNEL_MEGA 0
#define RT_KERNEL_WAVEFRONT 1

typedef struct RtOptions {
    int width, height;   /* frame (rt/macros.h:3-4: 1920x1080) */
    int passes;          /* passes per call; the reference runs 1 per render() */
    int adaptive;        /* 1: rt/path_tracing.cuh:352-376 test; 0: always sample */
    int min_samples;     /* MIN_SAMPLES (rt/macros.h:13) */
    float tolerance;     /* MAX_TOLERANCE (rt/macros.h:17) */
    int max_depth;       /* 0 = unbounded (reference); else max extension rays per path */
    int kernel;          /* RT_KERNEL_MEGA (one launch) or RT_KERNEL_WAVEFRONT (trace/shade queues) */
    void *stream;        /* hipStream_t; NULL = synchronous on the null stream */
    unsigned long long *counters_device; /* optional RT_CNT_COUNT u64 counters (adds) */
    unsigned long long *wave_times_device; /* optional debug: megakernel (with counters): 2 u64 per wave;
                          * wavefront: 3 u64 per trace launch (first start, first queue
                          * exhaustion, ~last end; s_memrealtime, 100 MHz), pre-set to ~0 */
    /* wavefront tuning (0 = default): below wf_tail (default 65536) live
     * paths the rest of the call runs in one cooperative finisher launch on at
     * most wf_finish_waves waves (default 2048; 512 for trees with fewer than
     * 2^18 leaf entries, whose short rays keep fuller waves busy);
     * wf_tail > width*height runs the whole call in the finisher (persistent
     * per-wave path fetch, no queue iterations) */
    int wf_tail;
    int wf_finish_waves;
    int profile;         /* 1: time the wavefront kernels with HIP events (rt_last_profile) */
    /* cooperative traversal tuning (0 = default): node fetches per descent
     * round, and pending lanes (of 64) before a wave's leaf test runs */
    int wf_descent_cap;
    int wf_postpone;
    int wf_wide;         /* wide single-ray traversal (all 64 lanes on one ray, one ray after the other):
                          * < 0 off; else for the rays of a finisher wave with at most wf_wide live rays
                          * and, once a trace launch's queue is empty, of a trace wave with at most
                          * wf_wide rays left (0 = default 32) */
    /* row-interleaved sharding (the parity-exact option): with
     * num_shards > 1 only rows y % num_shards == shard_id are rendered (the
     * others are left untouched); every shard uses the single-stream seeds,
     * so each owned pixel is bit-identical to the one-GPU render, adaptive
     * sampling included, and a sum of the shards' zero-initialised buffers
     * (rt_reduce_shards) is the one-GPU frame.  The spp-slice sharding of the
     * north star needs no option: seed shard g's G_Buffer from mt19937 outputs
     * [g*W*H, (g+1)*W*H) (rt_gbuffer_seeds skip). */
    int shard_id;
    int num_shards;
    /* wavefront: concurrent pipelines over disjoint pixel tiles, each with
     * its own queues and stream, so one pipeline's latency-bound launch
     * tails and finisher overlap the others' bulk work (0 = default 3, max 3:
     * with the caller's stream that is the 4 hardware queues of a process) */
    int wf_pipelines;
    /* wavefront: a path deeper than this many bounces (total internal
     * reflection loops in glass reach 10^4 and more) is handed to a kernel
     * running beside the pipelines, which finishes it one ray per wave with
     * all 64 lanes (0 = default 64, < 0 = off; values below 16 are raised to
     * 16: the long-path kernel is sized for rare deep paths, and at 8 it took
     * a third of all paths and ran 7x slower) */
    int wf_long_depth;
    /* ray queries (identical results either way): RT_TRAVERSAL_BOUNDED
     * (default) first finds a lower bound of the ray's first hit distance in
     * a conservative BVH built by rt_scene_prepare and skips the KD subtrees
     * the reference would test for nothing; RT_TRAVERSAL_KD runs the KD
     * traversal alone.  Calls with counters_device run the KD traversal (its
     * counters are the reference's) unless traversal is
     * RT_TRAVERSAL_BOUNDED_COUNTED: the wavefront queue trace launches then
     * run the bounded traversal and count its own work (RT_CNT_RAY, _NODE,
     * _TRI, _HIT, RT_CNT_B_*; measurement: the finisher and the long-path
     * kernel are not counted; the megakernel then runs its counting KD build). */
    int traversal;
    /* chained calls (default render only: bounded traversal, not counting).
     * 0: the call is complete at its stream point.  1: the call is only
     * enqueued — the caller's stream does not wait for it — and the NEXT call
     * of the same frame — same scene, G_Buffer, camera and frame options,
     * sample_count != 0, overlap 1 — is enqueued right behind it: its path
     * kernel starts when the previous one ends, without waiting for the
     * long-path kernel, whose deep glass paths (10^4+ bounces) run on beside
     * it; the pixels those paths still hold are owed the new call's passes and
     * run them before they are let go.  Every pixel's passes
     * run in the reference's order, so the frame is bit-identical to
     * unchained calls.  A call with sample_count 0 (reset_frame) is never
     * chained: it completes before the next call starts.  Whatever reads the frame in
     * between must join first: rt_join(stream), rt_synchronize, or the
     * library's own readers (rt_tonemap, rt_save_render, rt_gbuffer_save,
     * rt_reduce_shards, rt_deviation_stats), which join by themselves.  A
     * join of an open chain first enqueues its drain (the pixels still owed
     * passes run to the end); so do a call that does not continue the chain
     * and rt_shutdown.  The
     * reference's render() (rt/render.cuh:62-76) has no such tail: a call is
     * complete when its launches are (rt/main.cu:114-155). */
    int overlap;
    /* run-time exactness guard of the bounded traversal (default render):
     * 1 ray in check_interval (rounded up to a power of two; 0 = 4096) of
     * those the finisher traces is recorded with its result and traced again
     * by the plain KD traversal after the call; disagreements are counted in
     * RtDeviations.bounded_mismatches.  < 0: off. */
    int check_interval;
    int debug;           /* RT_DEBUG_* bits: stderr diagnostics of the wavefront calls */
    /* chained calls (overlap 1) of fewer passes than this are coalesced on
     * the host (ABI 8): such a call is recorded and returns; the pending
     * calls of the same frame, options and stream are launched as ONE chained
     * call once they hold this many passes, or before anything that must see
     * them — another call, rt_join and the library's readers of the frame,
     * rt_last_profile / rt_profile_history (one record per launched batch),
     * rt_shutdown.  k calls of p passes run each pixel's passes in the same
     * order as one call of k*p: bit-identical.  0 = default 256; < 0 = off
     * (every call launches). */
    int coalesce_passes;
} RtOptions;

#define RT_TRAVERSAL_BOUNDED 0
#define RT_TRAVERSAL_KD 1
#define RT_TRAVERSAL_BOUNDED_COUNTED 2
#define RT_DEBUG_CALL_LOG 1  /* per call / queue iteration: counters and host times */
#define RT_DEBUG_LONG_LOG 2  /* every deep sample's claim / end time and bounces (unchained calls) */
#define RT_DEBUG_CHECK_FAULT 4 /* tests of the guard: every checked ray is recorded with a wrong result */
#define RT_DEBUG_LONG_QUIT 8   /* tests of the failure path: the long-path kernel leaves at once, as if its
                                * safety net fired, stranding every pixel handed to it */
#define RT_DEBUG_SERIAL_LONG_FIRST 16 /* tests of serialised dispatch (a profiler's counter collection): the
                                       * long-path kernel runs to its end before the path kernel starts */
#define RT_DEBUG_SERIAL_FIN_FIRST 32  /* ... the path kernel runs to its end before the long-path kernel starts */
#define RT_DEBUG_WIDE_CAP1 64 /* tests of the long-path kernel's wave-wide bound query: its lists hold one item, so
                              * every query overflows and the ray is traced the other way (identical results,
                              * RtDeviations.wide_overflows counts them) */
#define RT_DEBUG_COUNT_LONG_ONLY 128 /* measurement (RT_TRAVERSAL_BOUNDED_COUNTED calls): only the long-path kernel
                                     * counts, so the counters hold the deep bounces' work alone */
#define RT_DEBUG_BUDGET1 256 /* tests of the path kernel's parked bound queries (RT_TRAVERSAL_BOUNDED_COUNTED calls): a
                             * wave parks its unfinished queries after one step of work instead of the shipped
                             * budget (identical results and counters); added within ABI 12, no struct changed */
/* (calls with RT_DEBUG_CALL_LOG, _LONG_LOG or _SERIAL_* are never coalesced) */

/* Per-call kernel timing of the last rt_render on this device with
 * RtOptions.profile = 1 (wavefront kernels: HIP events on the pipelines'
 * streams for the queue variants, the finisher's device span for the default
 * render; reading it waits for that call's kernels). */
typedef struct RtProfile {
    int iterations;      /* trace/shade queue iterations */
    int trace_launches, shade_launches, finish_launches;
    float start_ms;      /* wf_start */
    float trace_ms;      /* sum over the call's trace launches */
    float shade_ms;      /* sum over the call's shade launches */
    float finish_ms;     /* the finisher launches (0 or 1 per pipeline) */
    float call_ms;       /* first to last event of the call */
    float trace_union_ms; /* wall time with at least one trace launch running (launches of
                          * concurrent pipelines overlap: trace_ms sums their durations) */
    int pipelines;
} RtProfile;
int rt_last_profile(RtProfile *out);
/* every profiled rt_render's RtProfile on this device since the last reset,
 * oldest first: up to `cap` into out, the number recorded into *count.  For
 * the default render (one finisher launch per call) finish_ms and call_ms are
 * the finisher's span on the device, from its first wave's start to its last
 * wave's end (chained calls' finishers overlap: their spans do too), and
 * start_ms its start relative to the earliest start among the calls resolved
 * together (by this call or rt_last_profile).  Waits for those calls'
 * finishers. */
int rt_profile_history(RtProfile *out, int cap, int *count, int reset);

/* Always-on deviation statistics of every rt_render on the current device
 * since the last reset (recorded by every kernel, counting or not, at one
 * device-scope atomic per rare event).  The reference's bounce loop is
 * unbounded (rt/path_tracing.cuh:279-319); the build stops a path only at a
 * watchdog of 2^24 - 1 extension rays or at RtOptions.max_depth.
 * deep_hist[k] counts paths that ended at depth d (extension rays, as
 * RT_CNT_MAXDEPTH) with 64 * 2^k <= d < 64 * 2^(k+1); max_deep_depth is the
 * longest of them (0 if no path reached depth 64).  reset != 0 zeroes the
 * statistics after reading them.  Synchronises the device. */
#define RT_DEV_HIST_BINS 18
typedef struct RtDeviations {
    unsigned long long watchdog_paths; /* cut by the watchdog (max_depth 0): a deviation from the reference */
    unsigned long long cut_paths;      /* cut at the depth limit (watchdog or max_depth) */
    unsigned long long max_deep_depth; /* longest path that reached depth 64 */
    unsigned long long deep_paths;     /* paths that reached depth 64 (sum of deep_hist) */
    unsigned long long deep_hist[RT_DEV_HIST_BINS];
    /* the bounded traversal's run-time guard (RtOptions.check_interval): rays
     * re-traced by the plain KD traversal, results that differed (a deviation
     * from the reference; 0 expected), and the first such ray (o, d) */
    unsigned long long bounded_checked;
    unsigned long long bounded_mismatches;
    float mismatch_ray[6];
    /* the deep-path hand-off of the default render (ABI 7):
     * owed_pixels / owed_passes: pixels taken back from the long-path kernel
     * that chained calls (RtOptions.overlap) had skipped, and the passes they
     * owed (run by the taker, in the pixel's order; > 0 shows the chained-call
     * protocol fired).  Failure signals, 0 in a working render:
     * long_safety_quits: long-path waves that left by a safety net while
     * handed-over paths were still unclaimed; stranded_pixels: pixels still
     * handed over after a join's drain (the frame is incomplete: the join
     * returns RT_E_INCOMPLETE, and the pixels are released so later renders
     * run); check_dropped: rays the guard sampled past its per-call record
     * capacity (not re-traced).  linger_expiries: finisher waves that stopped
     * waiting (1 s) for pixels out in the long-path kernel, which then
     * finishes those pixels itself (a slow tail, not an error).
     * long_closed (ABI 8): long-path kernels that found their call's path
     * kernel not started within their bound (a profiler serialising
     * dispatches, a shared chip) and closed the hand-off until the next
     * unchained call: the path kernel then runs its deep paths itself
     * (identical results, a slower tail). */
    unsigned long long owed_pixels;
    unsigned long long owed_passes;
    unsigned long long long_safety_quits;
    unsigned long long stranded_pixels;
    unsigned long long check_dropped;
    unsigned long long linger_expiries;
    unsigned long long long_closed;
    /* wide_overflows (ABI 9): bounces of the long-path kernel whose wave-wide
     * bound query outgrew its on-chip lists and were traced by the wide KD
     * traversal instead (identical results, a slower bounce; 0 in the recorded
     * runs of the 2M-triangle bench scene: the lists are sized on its grazing
     * rays, csrc/wide_bvh_caps.h). */
    unsigned long long wide_overflows;
} RtDeviations;
int rt_deviation_stats(RtDeviations *out, int reset);
/* The T* certificate of the bounded traversal (added within ABI 12; counting
 * renders only: RtOptions.traversal = RT_TRAVERSAL_BOUNDED_COUNTED on the
 * wavefront kernel): of the rays that hit something, how many the
 * certificate covered (no KD descent) and how many a KD descent found
 * (rays it does not cover, and the few the bound does not apply to); their
 * sum is RT_CNT_HIT.  On this device since the last reset (rt_deviation_stats' reset
 * zeroes them too).  Either pointer may be NULL.  Joins like
 * rt_deviation_stats. */
#define RT_HAS_KD_CERT_STATS 1
int rt_kd_cert_stats(unsigned long long *certified, unsigned long long *fallback, int reset);

void rt_default_options(RtOptions *opt);
/* render(): if sample_count == 0 the frame's fb/sq/count are reset first
 * (reset_frame; RNG state is kept), then opt->passes passes run, each one
 * sample for every pixel that passes the adaptive test. */
int rt_render(rt_scene_t scene, G_Buffer g_buffer, Camera camera, int sample_count, const RtOptions *opt);

/* ---------------- ray queries and first-hit AOVs (ABI 10) ----------------
 * The renderer's closest-hit query for the caller's own rays: trace_ray
 * (rt/trace_ray.cuh:244-318) on n rays of 6 floats (origin, direction), and
 * the first-hit feature buffers of a camera (depth, normal, albedo, triangle
 * id) that denoisers and compositors take beside a low-spp frame.
 *
 * For every ray — any 6 floats whatever: directions are NOT normalised (the
 * reference's trace_ray does not normalise them either), NaN / Inf / zero
 * directions and far origins included — triangle, the barycentrics,
 * position, normal and tangent are bit-identical to the reference's
 * trace_ray, in either traversal mode.  RT_TRAVERSAL_BOUNDED applies the
 * conservative-BVH bound only where its exactness argument holds: rays with
 * 0.5 <= max(|d.x|, |d.y|, |d.z|) <= 2 (every unit direction) that do not lie
 * in a KD split plane; every other ray is traced by the plain KD traversal
 * (stats [2] counts them).  RT_TRAVERSAL_BOUNDED_COUNTED is taken as
 * RT_TRAVERSAL_BOUNDED.
 *
 * These calls read the prepared scene only: they neither read nor write a
 * G_Buffer, join no chain and touch no render workspace, so they may run
 * between chained rt_render calls.  They share one query workspace per
 * device (released by rt_shutdown): calls on different streams are ordered
 * among themselves on the device by an event. */
typedef struct RtRayHit { int32_t triangle; float bx, by, bz; } RtRayHit; /* 16 B; triangle -1 = miss, b* = 0 */
typedef struct RtRaySurface {          /* 80 B, 16-B aligned */
    float position[3]; float t;        /* t = magnitude(position - origin), sqrt((dx*dx + dy*dy) + dz*dz); miss: +inf */
    float normal[3];   float _pad0;    /* shading normal, flipped against the ray as trace_ray does */
    float tangent[3];  float _pad1;
    float albedo[3];   float _pad2;    /* material albedo * texel, as the renderer shades it */
    float emittance[3]; float _pad3;
} RtRaySurface;                        /* miss: all fields 0 except t */
typedef struct RtQueryOptions {
    int traversal;                     /* RT_TRAVERSAL_BOUNDED (default) or RT_TRAVERSAL_KD */
    void *stream;                      /* hipStream_t; NULL = synchronous on the null stream */
    unsigned long long *stats_device;  /* optional, 3 u64, adds: [0] rays, [1] hits, [2] rays traced by the
                                        * plain KD traversal */
} RtQueryOptions;
void rt_default_query_options(RtQueryOptions *opt);
/* rays_device: n x 6 floats (o.xyz d.xyz), 8-B aligned; hits_device: n RtRayHit, 16-B aligned; surface_device:
 * n RtRaySurface, 16-B aligned, or NULL.  Records at index n and beyond are never written.  n == 0: RT_OK
 * without a launch; n < 0, n > 2^31 - 1, a null or misaligned pointer: RT_E_INVALID before any GPU call.
 * opt NULL = the defaults. */
int rt_trace_rays(rt_scene_t scene, const float *rays_device, long long n, RtRayHit *hits_device,
                  RtRaySurface *surface_device, const RtQueryOptions *opt);
/* The pixel-centre rays of a width x height frame: the renderer's camera ray (rt/path_tracing.cuh:381-391)
 * with both jitter draws 0.5 and no aperture offset — the origin is the camera position bit for bit; no RNG
 * is consumed.  rays_device: width*height x 6 floats, 8-B aligned; ray y*width + x is pixel (x, y), row 0 =
 * bottom (the G_Buffer's orientation).  stream NULL = synchronous. */
int rt_camera_rays(Camera camera, int width, int height, float *rays_device, void *stream);
/* width*height entries each, pixel y*width + x, row 0 = bottom; any may be NULL.  depth: RtRaySurface.t
 * (+inf: miss); normal, albedo: 3 floats per pixel (0: miss); triangle: RtRayHit.triangle (-1: miss). */
typedef struct RtAovBuffers { float *depth; float *normal; float *albedo; int32_t *triangle; } RtAovBuffers;
/* rt_camera_rays followed by rt_trace_rays with a surface output, bit for bit, in one kernel that stores no
 * rays. */
int rt_render_aov(rt_scene_t scene, Camera camera, int width, int height, const RtAovBuffers *buffers,
                  const RtQueryOptions *opt);

/* ---------------- occlusion queries (ABI 12) ----------------
 * "Is anything in the way?" — shadow rays, point-to-point visibility, ambient occlusion, line of sight.
 * occluded_device[i] = 1 if the reference's trace_ray (rt/trace_ray.cuh:244-318) on ray i returns a hit
 * whose ray parameter s -- the *t of the winning intersect_triangle (rt/trace_ray.cuh:90-97), the value
 * trace_leaf_node's smallest_t ends on -- satisfies s < tmax_device[i] (a float32 compare); else 0.
 * tmax_device NULL = +inf for every ray (the result is then rt_trace_rays' hit flag).
 *
 * So for every ray and every tmax the answer is (rt_trace_rays hits) && (s < tmax), bit for bit, in either
 * traversal mode — the reference's first-leaf rule and its s >= 1e-5 rule included: a ray with
 * !(tmax > 1e-5f) (NaN, zero, negative, -inf, 1e-5f itself) is never occluded and is not traced, and no
 * self-intersection offset is needed beyond the reference's own 1e-5.
 *
 * rays_device: rt_trace_rays' layout and rules (n x 6 floats, 8-B aligned, used as given, never
 * normalised, any floats).  tmax_device: n floats, 4-B aligned, in units of the ray parameter: a distance
 * when the direction has unit length.  Prefer normalised directions with tmax = |q - p| for a segment
 * p -> q: d = q - p with tmax = 1 is answered too, but such a direction usually lies outside the bounded
 * traversal's domain (0.5 <= max|d_i| <= 2) and takes the plain KD traversal.  occluded_device: n bytes at
 * any alignment; no byte outside [0, n) is written.
 *
 * n == 0: RT_OK without a launch; a null scene, rays or output, a misaligned rays or tmax pointer, n < 0,
 * n > 2^31 - 1: RT_E_INVALID before any GPU call.  opt NULL = the defaults; traversal and stream as for
 * rt_trace_rays; stats_device adds [0] rays, [1] occluded rays, [2] rays that ran the plain KD traversal
 * (a ray rejected by the tmax rule counts in [0] only).  Ordering: as the other query calls (above). */
int rt_occluded(rt_scene_t scene, const float *rays_device, const float *tmax_device, long long n,
                uint8_t *occluded_device, const RtQueryOptions *opt);

/* ---------------- radiance queries (ABI 12, an addition) ----------------
 * "What light arrives along this ray?" — light and irradiance probes, lightmap and vertex baking, panoramic,
 * fisheye, orthographic or stereo cameras, radiance caches, re-rendering chosen pixels: the renderer's
 * trace_path (rt/path_tracing.cuh:268-325) for the caller's own rays.
 *
 * For ray i (o, d = its 6 floats, used as given, never normalised) with st = rng_device[i], `samples` times:
 *     (L, st) = trace_path(o, d, st)      started as the renderer starts a camera ray: ray type PRIMARY,
 *                                         inside_medium false, throughput 1 — so the first hit's emission
 *                                         counts, NEE follows diffuse events, the roulette is the reference's,
 *                                         and a miss ends the path without a roulette draw (a ray whose first
 *                                         trace_ray misses gives L = 0 and leaves st as it was);
 *     radiance[i] = radiance[i] + L       component-wise float adds, in sample order;
 *     sq[i] = sq[i] + luminance(L)^2      with the operations of rt/path_tracing.cuh:322-324;
 * then rng_device[i] = st.  With accumulate = 0 the sums start at +0.0f, with accumulate = 1 at the buffers'
 * contents (rt_render's frame_buffer / squared_luminance rule): k calls of 1 sample with accumulate = 1 after a
 * first call with 0 equal one call of k samples bit for bit, and for a ray list that is a frame's camera
 * samples the outputs are rt_render's frame_buffer, squared_luminance and random_numbers.  radiance is a SUM:
 * divide by the number of samples taken.  Every value is the reference's bit for bit, in either traversal
 * mode: for every ray whose direction has a magnitude within [2^-20, 2^20] (unnormalised, axis-parallel
 * directions and origins outside the scene included), and for every ray whose first trace_ray hits nothing —
 * among them every ray with a NaN or Inf component and every zero direction, which no intersect_triangle
 * test passes: L = 0, the RNG state untouched.  (A finite direction far outside that range that hits
 * something overflows in the reference's scatter arithmetic; its records then hold whatever that gives.)
 *
 * rays_device: n x 6 floats, 8-B aligned (rt_trace_rays' layout); rng_device: n uint32, read and written;
 * radiance_device: n x 3 floats; sq_luminance_device: n floats or NULL; all 4-B aligned.  Nothing at index n
 * or beyond is read or written.  n == 0: RT_OK without a launch; a null scene, rays, rng or radiance pointer, a
 * misaligned pointer, n < 0, n > 2^31 - 1, samples, max_depth or accumulate out of range: RT_E_INVALID before
 * any GPU call.  opt NULL = the defaults.
 *
 * Like the other queries it reads the prepared scene only — no G_Buffer, render workspace or chain, nothing
 * added to rt_deviation_stats (cuts and the longest path go to stats_device) — and shares their per-device
 * workspace and event ordering (released by rt_shutdown). */
#define RT_HAS_TRACE_PATHS 1
typedef struct RtPathOptions {
    int samples;      /* paths per ray; 0 = default 1; 1 .. 1<<20 */
    int max_depth;    /* as RtOptions.max_depth: 0 = unbounded (the 2^24-1 watchdog), else max extension rays */
    int accumulate;   /* 0: outputs are written as (+0 + the samples); 1: the samples are added to what the
                         output buffers hold (rt_render's fb/sq rule) */
    int traversal;    /* RT_TRAVERSAL_BOUNDED (default) / RT_TRAVERSAL_KD; _BOUNDED_COUNTED is taken as BOUNDED */
    void *stream;     /* hipStream_t; NULL = synchronous on the null stream */
    unsigned long long *stats_device; /* optional, 5 u64: adds [0] rays, [1] paths, [2] trace_ray calls
                         (extension + shadow rays, the oracle's RT_CNT_RAY meaning), [3] paths cut at the
                         depth limit; [4] longest path in extension rays (atomic max, not a sum) */
} RtPathOptions;
void rt_default_path_options(RtPathOptions *opt);
int rt_trace_paths(rt_scene_t scene, const float *rays_device, uint32_t *rng_device, long long n,
                   float *radiance_device, float *sq_luminance_device, const RtPathOptions *opt);

/* ---------------- radiance queries that make their own rays (within ABI 12, an addition) ----------------
 * rt_trace_paths for rays the library draws itself, on the device, from each element's own RNG state: a second
 * camera path beside rt_render (pinhole, equirectangular, fisheye, orthographic) and a probe / baking primitive
 * (cosine-weighted hemispheres over surface points).  No ray buffer exists: a lane draws its element's next ray
 * where it would otherwise re-read the caller's.
 *
 * A sampler maps (element e, RNG state st) to (origin o, direction d, new st).  Every operation is a correctly
 * rounded float32 one (+ - * / sqrtf, compares) or the library's sincos (rt_libm.h), unfused, in the order written;
 * draws are the renderer's get_random_unilateral, in the order written.  Element e of an image sampler is pixel
 * (x, y) = (e % width, e / width), row 0 = bottom (the G_Buffer's orientation); W, H = (float)width, height; R is
 * the camera's rotation (Camera::rotation(), a host-side frame constant) and R*v = (v.x*i + v.y*j) + v.z*k;
 * TAU = PI * 2 with the reference's PI = 3.1415926536f.
 *
 *   RT_SAMPLER_PINHOLE (4 draws)  the renderer's camera sample (rt/path_tracing.cuh:381-391, :327-336): draws rx,
 *       ry; dir = normalize(t*((float)x + rx - hw)/hw, t*((float)y + ry - hh)/hw, 1) with t = tanf(FOV / 2),
 *       hw = (float)(width / 2), hh = (float)(height / 2) (integer halves; hw divides on both axes); d = R*dir;
 *       theta = draw * TAU; r = sqrtf(draw) * aperture_radius; (s, c) = sincos(theta);
 *       o = (position + R*(r*c, 0, 0)) + R*(0, r*s, 0).
 *   RT_SAMPLER_EQUIRECT (2 draws: rx, ry)  lon = ((float)x + rx) / W * TAU - PI;
 *       lat = ((float)y + ry) / H * PI - PI * 0.5f; (sl, cl) = sincos(lon); (sa, ca) = sincos(lat);
 *       d = R*(ca*sl, sa, ca*cl); o = position.
 *   RT_SAMPLER_FISHEYE (2 draws: rx, ry)  equidistant, the image circle inscribed in the shorter side:
 *       rad = min(W, H) * 0.5f; u = (((float)x + rx) - W*0.5f) / rad; v = (((float)y + ry) - H*0.5f) / rad;
 *       r = sqrtf(u*u + v*v); if !(r <= 1): d = 0 (outside the circle; the 2 draws are taken all the same); else
 *       theta = r * (FOV * 0.5f); (s, c) = sincos(theta); k = r > 0 ? s / r : 0; d = R*(k*u, k*v, c).  o = position.
 *   RT_SAMPLER_ORTHO (2 draws: rx, ry)  u = (((float)x + rx) - W*0.5f) / (W*0.5f) * ortho_half_width;
 *       v = (((float)y + ry) - H*0.5f) / (W*0.5f) * ortho_half_width (square pixels);
 *       o = (position + R*(u, 0, 0)) + R*(0, v, 0); d = R*(0, 0, 1).
 *   RT_SAMPLER_HEMISPHERE (2 draws, diffuse_direction's order, rt/path_tracing.cuh:45-59)  element e reads 6 floats
 *       of points_device: position p, normal n (used as given).  (ds, dc) = sincos(draw * TAU); ru2 = draw;
 *       sq = sqrtf(ru2); d = sq*dc*t + sqrtf(1 - ru2)*n + sq*ds*b; o = p.  (t, b) is the branch-free frame of n
 *       (Duff et al. 2017): sg = copysignf(1, n.z); a = -1 / (sg + n.z); q = n.x*n.y*a;
 *       t = (1 + sg*n.x*n.x*a, sg*q, -sg*n.x); b = (q, sg + n.y*n.y*a, -n.y).  Cosine-weighted for a unit n: the
 *       mean of L times pi is the irradiance at p.
 *
 * Pixel list (image kinds): with pixels_device, element i is the pixel pixels_device[i]; an index outside
 * [0, width*height), compared unsigned, gives o = d = 0 and draws nothing — such a ray hits nothing: L = 0 and the
 * RNG state stays.  Centre ray (image kinds; rt_sampler_rays with rng NULL): both jitter draws are taken as 0.5,
 * there is no lens offset and nothing is drawn; for PINHOLE these are rt_camera_rays' rays bit for bit.
 * NaN or infinite camera fields are safe (no float is converted to an int, nothing is indexed by one): such rays
 * miss.
 *
 * THE CONTRACT.  rt_sample_paths with samples = k and accumulate = a gives the same radiance, sq_luminance and rng,
 * bit for bit, as k rounds of { rt_sampler_rays; rt_trace_paths(samples = 1, accumulate = a || round > 1) }, in
 * either traversal mode.  So a PINHOLE sampler with no pixel list run on a G_Buffer's random_numbers, frame_buffer,
 * squared_luminance and sample_count with accumulate = 0 is rt_render(sample_count = 0, passes = k, adaptive = 0) on
 * that G_Buffer, bit for bit in all four arrays — and a sampled image's outputs are a G_Buffer: rt_tonemap,
 * rt_save_render and rt_gbuffer_save read it as it is.
 *
 * RT_E_INVALID before any GPU call: what rt_trace_paths checks; a null sampler or a kind out of range; image kinds
 * with width or height < 1 or width*height > 2^31 - 1; no pixel list and n != width*height; FISHEYE with a FOV
 * that is not finite or outside (0, 2 pi]; ORTHO with an ortho_half_width that is not finite or <= 0; HEMISPHERE
 * with null or misaligned points; a misaligned pixels_device or sample_count_device; rt_sampler_rays(_host) with
 * null rays, or with rng NULL for HEMISPHERE.  n == 0: RT_OK without a launch.  Nothing at index n or beyond is
 * read or written.  Workspace, ordering and stats_device: rt_trace_paths' (no G_Buffer, chain or render workspace
 * is touched).
 *
 * AOVs, denoising and reprojection for every image kind are rt_sample_aov, rt_denoise_sampler and
 * rt_reproject_sampler ("frames of every camera model", below).  rt_sample_paths itself gives every element every
 * sample; the adaptive test is rt_sample_paths_adaptive's (below). */
#define RT_HAS_PATH_SAMPLERS 1
#define RT_SAMPLER_PINHOLE 0
#define RT_SAMPLER_EQUIRECT 1
#define RT_SAMPLER_FISHEYE 2
#define RT_SAMPLER_ORTHO 3
#define RT_SAMPLER_HEMISPHERE 4
/* (with ISAKLM_RT_CALLER_TYPES the caller's Camera is not complete here: the field then is these 28 bytes, the
 * layout ISAKLM_RT_CHECK_LAYOUT() asserts of Camera, and the caller copies its camera into them) */
#ifdef ISAKLM_RT_CALLER_TYPES
typedef struct RtSamplerCamera { float position[3]; float yaw, pitch, FOV, aperture_radius; } RtSamplerCamera;
#else
typedef Camera RtSamplerCamera;
#endif
typedef struct RtSampler {
    int kind;                       /* RT_SAMPLER_* */
    int width, height;              /* image kinds */
    RtSamplerCamera camera;               /* image kinds: position, yaw, pitch; FOV: PINHOLE as the renderer, FISHEYE the full
                                       angle across the image circle, (0, 2*pi]; aperture_radius: PINHOLE only */
    float ortho_half_width;         /* ORTHO: world units from the centre to the left / right edge, finite, > 0 */
    const int32_t *pixels_device;   /* image kinds, optional: n pixel indices; NULL: element i = pixel i and n == width*height */
    const float *points_device;     /* HEMISPHERE: n x 6 floats (position, normal), 8-B aligned */
} RtSampler;

/* per element, `samples` times: (o, d, st) = sampler(e, st); (L, st) = trace_path(o, d, st); sums as rt_trace_paths.
 * sample_count_device (optional, n ints): count = (accumulate ? count : 0) + samples. */
int rt_sample_paths(rt_scene_t scene, const RtSampler *sampler, uint32_t *rng_device, long long n,
                    float *radiance_device, float *sq_luminance_device, int *sample_count_device,
                    const RtPathOptions *opt);
/* one sample's rays, n x 6 floats, rt_trace_rays' layout; advances rng_device.  rng_device NULL: the centre rays
 * (image kinds; RT_E_INVALID for HEMISPHERE). */
int rt_sampler_rays(const RtSampler *sampler, uint32_t *rng_device, long long n, float *rays_device, void *stream);
/* the same arithmetic on host arrays (pixels / points / rng / rays are host pointers), bit for bit */
int rt_sampler_rays_host(const RtSampler *sampler, uint32_t *rng, long long n, float *rays);

/* ---------------- adaptive samplers (within ABI 12, an addition) ----------------
 * rt_sample_paths with the renderer's adaptive test (rt/path_tracing.cuh:352-376) in front of every sample:
 * panoramas, fisheye and orthographic frames and probe sets that stop sampling element by element, as rt_render's
 * pinhole frames do.  No existing struct grows; with adaptive NULL the call is rt_sample_paths.
 *
 * With adaptive given, element e starts from (sum, sum_sq, cnt) = the buffers' contents (accumulate = 1) or
 * (+0, +0, 0) (accumulate = 0) and runs `samples` passes:
 *
 *     if (!adaptive_run(sum, sum_sq, cnt))   the pass is used up: no ray is drawn, no RNG draw is taken
 *     else (o, d, st) = sampler(e, st); (L, st) = trace_path(o, d, st); sum += L; sum_sq += luminance(L)^2; cnt += 1
 *
 * adaptive_run is rt_render's test, operation for operation: cnt < min_samples -> run; else tl = luminance(sum),
 * mean = tl / cnt, var = (sum_sq - tl*tl / cnt) / (cnt - 1), iw = z * sqrtf(var / cnt) with
 * z = sqrtf(2) * erfinvf(1 - tolerance) computed on the host, run = iw > mean * tolerance — at min_samples 0 and 1
 * too, where the variance divides by cnt - 1 <= 0 (0 / 0 is a NaN, which fails the compare: the element stops).  A
 * skipped pass leaves the state as it was, so every later pass of the call skips too.  At the end radiance,
 * sq_luminance, sample_count = cnt and rng are written (with accumulate = 1 an element that took no sample is
 * not stored: the buffers hold those bits).
 *
 * THE CONTRACTS.  A PINHOLE sampler with no pixel list on a G_Buffer's four arrays is
 * rt_render(sample_count = accumulate ? 1 : 0, passes = samples, adaptive = 1, min_samples, tolerance) on that
 * G_Buffer, bit for bit in all four arrays, in either traversal mode.  For every kind (pixel lists and hemisphere
 * points included) samples = k equals k host-driven rounds of { the open set A of the current state
 * (rt_convergence_host); rt_sample_paths(samples = 1, accumulate = 1) on A's gathered rng, radiance, sq, count and
 * pixel indices or points; scatter back }, bit for bit.
 *
 * stats_device keeps RtPathOptions' five words: [1] (paths) is the number of samples actually taken, so
 * samples * n - paths passes were skipped; a call that adds 0 to [1] found every element converged and adds 0 to
 * [2] (no ray was traced).
 *
 * RT_E_INVALID before any GPU call: what rt_sample_paths checks, and with adaptive given a null
 * sq_luminance_device or sample_count_device, or min_samples < 0.  tolerance is taken unchecked, as rt_render's. */
#define RT_HAS_ADAPTIVE_SAMPLERS 1
typedef struct RtAdaptive { int min_samples; float tolerance; } RtAdaptive;   /* rt_render's MIN_SAMPLES / MAX_TOLERANCE */
int rt_sample_paths_adaptive(rt_scene_t scene, const RtSampler *sampler, uint32_t *rng_device, long long n,
                             float *radiance_device, float *sq_luminance_device, int *sample_count_device,
                             const RtPathOptions *opt, const RtAdaptive *adaptive);

/* ---------------- convergence (within ABI 12, an addition) ----------------
 * "Is this frame done?": the adaptive test asked of n elements' sums — a G_Buffer's frame_buffer,
 * squared_luminance and sample_count, or rt_sample_paths' outputs — without sampling anything.  Per element, with
 * adaptive_run's operations in their order (above):
 *   open       adaptive_run would run a sample on the next pass;
 *   stats      4 u64: [0] elements, [1] open elements, [2] elements with count < min_samples, [3] the sum of the
 *              counts (rt_convergence adds to stats_device, rt_convergence_host writes);
 *   rel_error  (optional, n floats) +inf for count < 2; 0 where !(iw > 0) (black elements, a variance that rounds
 *              negative); otherwise the one float division iw / mean.  A diagnostic: open is never derived from it.
 * rt_convergence (GPU) and rt_convergence_host (CPU) give the same bits.  rt_convergence reads what may be a frame:
 * like rt_tonemap and rt_denoise it first joins the renders (chained calls' deep-path tails included) on `stream`;
 * stream NULL = synchronous.  It keeps no workspace.  RT_E_INVALID before any GPU call: a null radiance,
 * sq_luminance or sample_count pointer, n < 0 or > 2^31 - 1, a misaligned pointer (4 B; stats 8 B),
 * min_samples < 0.  n == 0: RT_OK without a launch.  tolerance is taken unchecked. */
#define RT_HAS_CONVERGENCE 1
int rt_convergence(const float *radiance_device, const float *sq_luminance_device, const int *sample_count_device,
                   long long n, int min_samples, float tolerance, float *rel_error_device,
                   unsigned long long *stats_device, void *stream);
int rt_convergence_host(const float *radiance, const float *sq_luminance, const int *sample_count, long long n,
                        int min_samples, float tolerance, float *rel_error, unsigned long long stats[4]);

/* draw_frame's colour math (rt/render.cuh:37-59): correct_color(fb/count) ->
 * RGBA8 into a device buffer of width*height*4 bytes, row 0 = bottom. */
int rt_tonemap(G_Buffer g_buffer, uint8_t *rgba_device, int width, int height, void *stream);
/* save_render (rt/save_render.cuh:25-67): tonemap, flip vertically, write PNG */
int rt_save_render(G_Buffer g_buffer, int width, int height, const char *png_path);
/* the PNG encoder rt_save_render uses (replaces lodepng::encode,
 * rt/save_render.cuh:18-23): host RGBA8 rows top to bottom */
int rt_write_png(const char *png_path, const uint8_t *rgba_host, int width, int height);

/* ---------------- denoising (ABI 11) ----------------
 * A variance-guided edge-avoiding a-trous filter for low-spp frames: the
 * G_Buffer's mean radiance (frame_buffer / sample_count), smoothed over
 * `iterations` levels of a 5x5 B3-spline kernel with tap spacing 1, 2, 4, ...,
 * each tap weighted by edge stops on the first-hit normal and depth
 * (rt_render_aov's buffers) and on the luminance difference measured in
 * standard deviations of the pixel's mean (from squared_luminance, the
 * quantity the adaptive test uses).  Hits and misses never mix.  With
 * demodulation the filter runs on colour / albedo and the albedo is multiplied
 * back, so textures stay sharp.  DESIGN.md "Denoising" defines every operation:
 * all of them are correctly rounded float32 operations in a fixed order, and
 * rt_denoise (GPU) and rt_denoise_host (CPU) give the same bits.
 *
 * rt_denoise reads the frame: like rt_tonemap it first joins the renders
 * (chained calls' deep-path tails included) on `stream`.  It writes only
 * rgb_out_device.  It keeps one workspace per device (52 B per pixel of the
 * last frame, released by rt_shutdown); calls on different streams are
 * ordered on it by an event.  Errors before any GPU call (RT_E_INVALID): a
 * null required buffer, a bad size (width or height < 1, width * height >
 * 2^31 - 1), iterations or normal_log2 out of range, demodulate outside
 * {-1, 0, 1}, a negative or non-finite sigma. */
typedef struct RtDenoiseOptions {
    int   iterations;    /* a-trous levels, tap spacing 1,2,4,...; 0 = default 5; 1..8 */
    float sigma_lum;     /* 0 = default 4:   luminance edge stop, in standard deviations of the pixel's mean */
    float sigma_depth;   /* 0 = default 1:   depth edge stop, in local depth slopes */
    int   normal_log2;   /* 0 = default 7:   normal weight = max(0, n_p.n_q)^(2^k), by k squarings; 1..10 */
    int   demodulate;    /* 0 = default on (1): filter colour / albedo and multiply back; -1 = off */
    void *stream;        /* hipStream_t; NULL = synchronous */
} RtDenoiseOptions;
void rt_default_denoise_options(RtDenoiseOptions *opt);
/* rgb_out_device: width*height x 3 floats, mean radiance, row 0 = bottom (the G_Buffer's orientation).
 * aov: depth and normal required; albedo required unless demodulate = -1; triangle unused.
 * opt NULL = the defaults. */
int rt_denoise(G_Buffer g, const RtAovBuffers *aov, int width, int height, float *rgb_out_device,
               const RtDenoiseOptions *opt);
/* the same arithmetic on host arrays, same layouts (CPU tier, integrators without a GPU at hand);
 * opt->stream is ignored */
int rt_denoise_host(const float *fb, const float *sq, const int *count, const float *depth, const float *normal,
                    const float *albedo, int width, int height, float *rgb_out, const RtDenoiseOptions *opt);
/* rt_tonemap's colour math (correct_color -> RGBA8) for a float RGB mean-radiance buffer (width*height x 3
 * floats, e.g. rt_denoise's output) */
int rt_tonemap_rgb(const float *rgb_device, uint8_t *rgba_device, int width, int height, void *stream);

/* ---------------- temporal reprojection (ABI 12, an addition) ----------------
 * Carries a frame's samples over to a moved camera, where the reference's
 * main() calls reset_frame (rt/main.cu:114-155) and starts again at 0 spp.
 * The history needs no new type: a reprojected frame is another G_Buffer —
 * per-pixel sums frame_buffer and squared_luminance and a per-pixel
 * sample_count — which rt_render with sample_count != 0 adds passes to,
 * rt_denoise takes its variance from and rt_tonemap divides:
 *
 *     rt_render_aov(scene, cam_new, W, H, &aov_new, NULL);
 *     rt_reproject(g_old, &aov_old, cam_old, &aov_new, cam_new, W, H, g_new, NULL);   instead of a reset
 *     rt_render(scene, g_new, cam_new, 1, &opt);                                      adds passes to the carried sums
 *
 * For every pixel of the new frame that hit something, its first hit (the
 * pixel-centre ray times dst_aov->depth, kept relative to the old camera) is
 * projected into the old frame.  A projection within 1/64 pixel of a pixel
 * centre takes that pixel alone, any other the four bilinear taps around it.
 * A tap counts if it lies in the frame, has samples, hit something, and shows
 * the same surface: its depth within depth_tol (relative) of the point's
 * distance from the old camera, its normal within normal_min (a cosine) of
 * the new pixel's and, with match_triangle, the same triangle.  If the
 * counting taps hold at least 1/16 of the weight, the pixel gets their
 * weighted mean radiance and mean squared luminance times n, with
 * n = min(the counting taps' sample counts, max_history) as its sample_count;
 * a lone tap that keeps its whole count is copied bit for bit (an unmoved
 * camera returns the frame itself).  Every other pixel — a miss, a point
 * behind or outside the old frame, a disocclusion, a carried sum that is NaN
 * or infinite (it would spread with every later move) — is reset: sums 0, count 0,
 * which rt_render's adaptive test and rt_denoise take as "no samples yet".
 * DESIGN.md "Temporal reprojection" defines every operation: all are correctly
 * rounded float32 operations in a fixed order, and rt_reproject (GPU) and
 * rt_reproject_host (CPU) give the same bits.
 *
 * Writes dst.frame_buffer, dst.squared_luminance and dst.sample_count for all
 * width*height pixels and nothing else.  random_numbers is neither read nor
 * written in either G_Buffer: put the same RNG array in both and the per-pixel
 * streams simply continue.  dst's three written arrays must not overlap src's
 * three (the call is a gather).  AOVs: depth and normal are required on both
 * sides, triangle is optional on both, albedo is unused.
 *
 * rt_reproject reads a frame: like rt_tonemap and rt_denoise it first joins
 * the renders (chained calls' deep-path tails included) on `stream`.  It keeps
 * no per-device workspace, so calls are ordered by their streams alone.  A
 * following rt_render on dst is ordered behind it by the stream (or by the
 * NULL-stream call having been synchronous).
 * NaN and infinite depths, positions and angles are safe: they fail the
 * projection's compares and the pixel (for a camera whose yaw, pitch or FOV is
 * NaN, infinite or beyond +-2^19: every pixel) is reset.
 * Errors before any GPU call (RT_E_INVALID): a null required pointer, a bad
 * size (width or height < 1, width * height > 2^31 - 1; a 1-pixel-wide frame
 * has no camera — its half width is 0 — and resets every pixel), overlapping
 * src and dst arrays, max_history or match_triangle out of range, a negative,
 * NaN or infinite depth_tol, normal_min outside (-1, 1]. */
#define RT_HAS_REPROJECT 1
typedef struct RtReprojectOptions {
    int   max_history;    /* cap of the carried per-pixel sample count; 0 = default (64); 1 .. 1<<20 */
    float depth_tol;      /* 0 = default (0.02): a source tap is the same surface if |z_src - z_expected| <= depth_tol * z_expected */
    float normal_min;     /* 0 = default (0.95): ... and dot(n_new, n_src) >= normal_min;  (-1, 1] */
    int   match_triangle; /* 0 = default on (1) when both triangle buffers are given: ... and the triangle ids are equal; -1 = off */
    void *stream;         /* hipStream_t; NULL = synchronous */
    unsigned long long *stats_device; /* optional, 3 u64, adds: [0] pixels, [1] pixels that kept history (count_out > 0),
                                         [2] samples carried (sum of count_out) */
} RtReprojectOptions;
void rt_default_reproject_options(RtReprojectOptions *opt);
/* opt NULL = the defaults */
int rt_reproject(G_Buffer src, const RtAovBuffers *src_aov, Camera src_camera,
                 const RtAovBuffers *dst_aov, Camera dst_camera, int width, int height,
                 G_Buffer dst, const RtReprojectOptions *opt);
/* the same arithmetic on host arrays, same layouts (fb: 3 floats per pixel); the triangle arrays and stats may
 * be NULL; stats is written (not added to); opt->stream and opt->stats_device are ignored */
int rt_reproject_host(const float *src_fb, const float *src_sq, const int *src_count,
                      const float *src_depth, const float *src_normal, const int32_t *src_triangle, Camera src_camera,
                      const float *dst_depth, const float *dst_normal, const int32_t *dst_triangle, Camera dst_camera,
                      int width, int height, float *dst_fb, float *dst_sq, int *dst_count,
                      unsigned long long stats[3], const RtReprojectOptions *opt);

/* ---------------- frames of every camera model (within ABI 12, an addition) ----------------
 * The frame tools above for an RtSampler's image kinds: a sampled frame (rt_sample_paths on a G_Buffer's arrays) gets
 * its guides, its denoiser and its history whatever the camera model.  No existing struct grows, no existing call
 * changes; RT_HAS_SAMPLER_FRAMES is the feature test.
 *
 * rt_sample_aov: rt_render_aov for a sampler.  Element i is the sampler's centre ray (both jitter draws 0.5, no lens
 * offset, nothing drawn: rt_sampler_rays with rng NULL); pixel lists are allowed.  An out-of-frame entry, or a fisheye
 * pixel outside the image circle, has d = 0 and misses: depth +inf, normal and albedo 0, triangle -1; an ORTHO
 * pixel's depth is measured from its own origin on the camera plane.  One launch of the query kernel: no ray and no
 * record is stored.  THE CONTRACT: every buffer is, bit for bit, what rt_sampler_rays(rng = NULL) + rt_trace_rays
 * with a surface output give (t, normal, albedo, triangle), in either traversal mode, and a PINHOLE sampler without a
 * pixel list is rt_render_aov.  RT_E_INVALID before any GPU call: what rt_sampler_rays checks, a HEMISPHERE sampler,
 * null buffers, a misaligned buffer; n == 0 or nothing asked for: RT_OK without a launch.  Workspace, ordering and
 * stats_device: rt_render_aov's.
 *
 * rt_denoise_sampler / rt_denoise_sampler_host: rt_denoise on a sampler's width x height frame.  Only whole frames: a
 * pixel list or a HEMISPHERE sampler is RT_E_INVALID.  For every kind but EQUIRECT the result is rt_denoise's
 * (rt_denoise_host's), bit for bit.  For EQUIRECT the x axis is periodic — longitudes -pi and +pi are neighbours —
 * and every x neighbour is taken modulo width where rt_denoise clamps or drops it: the depth slope's x +- 1, the
 * 3x3 variance blur's columns, the 5x5 taps' x + step*dx.  Rows stay as they are (the poles are edges).  The tap
 * order stays dy, then dx, from -2 to 2; taps that alias one pixel (2*step >= width) are simply taken again.  So the
 * filter commutes with a roll of the frame's columns, bit for bit, and a panorama has no seam.  Join, workspace
 * (the same 52 B per pixel) and stream rules: rt_denoise's.
 *
 * rt_reproject_sampler / rt_reproject_sampler_host: rt_reproject for two samplers of one image kind, width and
 * height (whole frames; the camera fields, the FOV and ortho_half_width may differ).  Steps 1 and 4-7 are
 * rt_reproject's; for dst pixel p with z = dst_depth[p] < inf, in this order, every operation a correctly rounded
 * float32 one or the library's atan2 / sincos (rt_libm.h):
 *   2. (o_rel, d) = the dst sampler's centre ray for a camera at the origin (rt_sample_aov's d, bit for bit; the
 *      origin relative to the camera position): o_rel = +0, for ORTHO (0 + R*(u, 0, 0)) + R*(0, v, 0);
 *      v = (delta + o_rel) + d*z with delta = pos_dst - pos_src (never a world position);
 *      c = (v . Rs.i, v . Rs.j, v . Rs.k) with Rs the src camera's rotation; |v| = sqrtf((v.x^2 + v.y^2) + v.z^2).
 *   3. the continuous source pixel (u, w) and the depth z_exp the source AOV holds there; W, H = (float)width, height:
 *      PINHOLE   rt_reproject's text (the aperture is ignored): z_exp = |v|.
 *      ORTHO     z_exp = c.z;  u = (c.x / ohw * (W*0.5f) + W*0.5f) - 0.5f;  w = (c.y / ohw * (W*0.5f) + H*0.5f) - 0.5f
 *                (ohw = the src sampler's ortho_half_width).
 *      EQUIRECT  z_exp = |v|;  lon = atan2(c.x, c.z);  h = sqrtf(c.x^2 + c.z^2);  lat = atan2(c.y, h);
 *                u = (lon + PI) / TAU * W - 0.5f;  w = (lat + PI*0.5f) / PI * H - 0.5f.  Tap columns are taken modulo
 *                width (the snapped tap, x0 = -1, x0 + 1 = width); rows are not wrapped.
 *      FISHEYE   z_exp = |v|;  h = sqrtf(c.x^2 + c.y^2);  theta = atan2(h, c.z);  r = theta / (FOV_src * 0.5f), reset
 *                unless r <= 1;  s = h > 0 ? r / h : 0;  rad = min(W, H) * 0.5f;  u = ((s*c.x)*rad + W*0.5f) - 0.5f;
 *                w = ((s*c.y)*rad + H*0.5f) - 0.5f.
 *      Every model but PINHOLE resets unless 0 < z_exp < inf; then rt_reproject's frame test on (u, w).
 * THE CONTRACTS.  Two PINHOLE samplers give rt_reproject's output and stats bit for bit; GPU and host give the same
 * bits for every kind; an unmoved camera returns the frame itself, bit for bit, wherever the projection round-trips
 * within the 1/64-pixel snap — it does by a factor of ~50 in frames up to 257 x 129 (worst error 2.9e-4 pixel).  In
 * large frames float32 runs out near an equirectangular frame's poles: at 1920 x 960 the pole rows of a rotated
 * panorama are off by up to 0.017 pixel and may take four taps instead of a copy.  That is float32, not a defect.
 * NaN and infinite camera fields are safe as in rt_reproject: they fail the compares and every pixel resets; no
 * float that can be a NaN is converted to an int before a compare has passed it.  RT_E_INVALID before any GPU call:
 * the two samplers not of the same image kind, width and height, a pixel list on either, a HEMISPHERE sampler, what
 * rt_sampler_rays checks of each, and everything rt_reproject checks.  Writes, join and ordering: rt_reproject's. */
#define RT_HAS_SAMPLER_FRAMES 1
int rt_sample_aov(rt_scene_t scene, const RtSampler *sampler, long long n, const RtAovBuffers *buffers,
                  const RtQueryOptions *opt);
int rt_denoise_sampler(G_Buffer g, const RtAovBuffers *aov, const RtSampler *sampler, float *rgb_out_device,
                       const RtDenoiseOptions *opt);
int rt_denoise_sampler_host(const float *fb, const float *sq, const int *count, const float *depth,
                            const float *normal, const float *albedo, const RtSampler *sampler, float *rgb_out,
                            const RtDenoiseOptions *opt);
int rt_reproject_sampler(G_Buffer src, const RtAovBuffers *src_aov, const RtSampler *src_sampler,
                         const RtAovBuffers *dst_aov, const RtSampler *dst_sampler, G_Buffer dst,
                         const RtReprojectOptions *opt);
/* rt_reproject_host's arrays, the two samplers in place of the two cameras and the frame size */
int rt_reproject_sampler_host(const float *src_fb, const float *src_sq, const int *src_count,
                              const float *src_depth, const float *src_normal, const int32_t *src_triangle,
                              const RtSampler *src_sampler,
                              const float *dst_depth, const float *dst_normal, const int32_t *dst_triangle,
                              const RtSampler *dst_sampler,
                              float *dst_fb, float *dst_sq, int *dst_count,
                              unsigned long long stats[3], const RtReprojectOptions *opt);

/* ---------------- multi-GPU shards ----------------
 * One process per GPU.  Rank 0 makes an id (rt_comm_unique_id), ships its
 * RT_COMM_ID_BYTES to the other ranks out of band, every rank calls
 * rt_comm_create, renders its shard (spp slice: seeds skipped by g*W*H; or
 * rows: RtOptions.shard_id / num_shards), then rt_reduce_shards sums fb, sq
 * and count of every rank into `root` (one RCCL reduce per array, grouped;
 * stream NULL = synchronous). */
#define RT_COMM_ID_BYTES 128
typedef struct RtComm *rt_comm_t;
int rt_comm_unique_id(void *id_out);
int rt_comm_create(int nranks, int rank, const void *id, rt_comm_t *out);
int rt_comm_destroy(rt_comm_t comm);
int rt_reduce_shards(rt_comm_t comm, G_Buffer g_buffer, int width, int height, int root, void *stream);

/* self-test of the traversal's reciprocal-based division against IEEE '/'
 * on n random operand pairs (host); returns the number of mismatches */
unsigned long long rt_selftest_division(unsigned long long n, unsigned long long seed, unsigned long long *tested);

#ifdef __cplusplus
}
#endif
#endif /* ISAKLM_RT_H */
