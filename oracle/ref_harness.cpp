/*
 * ref_harness.cpp — TEST INFRASTRUCTURE ONLY.
 *
 * Driver of the reference's own source (INDA23PlusPlus/isaklm-raytracer): a C
 * interface shaped like rt_oracle.h over the reference's functions, compiled
 * by oracle/Makefile.ref from the reference's headers where they lie into
 * oracle/_ref/libref_rt.so.  oracle/reference.py wraps it; the tests compare
 * the oracle and the product with it, and tests/golden/reference/ holds its
 * recorded results.
 *
 * Nothing of the reference is copied here.  Every entry point marshals its
 * arguments, calls the reference's function and marshals the result; the file
 * holds no arithmetic of its own apart from erfinvf (not in the host libm) and
 * the colour-to-byte statement of ref_tonemap (see there).  The stand-in
 * headers are in ref_shim/; ref_shim/ref_preinclude.h routes the
 * transcendentals to csrc/rt_libm.h.
 *
 * SCREEN_W, SCREEN_H, MIN_SAMPLES and MAX_TOLERANCE are compile-time macros in
 * the reference.  macros.h is included first (it has #pragma once, so the
 * reference's later includes of it do nothing) and the four are then redefined
 * as variables: every use of them in the reference is a run-time expression.
 */
#include "macros.h"

#undef SCREEN_W
#undef SCREEN_H
#undef MIN_SAMPLES
#undef MAX_TOLERANCE
static int ref_screen_w = 3, ref_screen_h = 3, ref_min_samples = 100;
static float ref_max_tolerance = 0.05f;
#define SCREEN_W ref_screen_w
#define SCREEN_H ref_screen_h
#define MIN_SAMPLES ref_min_samples
#define MAX_TOLERANCE ref_max_tolerance

/* the reference's create_scene() calls create_models(), which lists the
 * reference's own meshes; its definition is renamed out of the way and
 * create_scene() finds ours, which lists the scene file's */
#define create_models ref_create_models_of_the_reference
#include "create_models.cuh"
#undef create_models
std::vector<Triangle> create_models();
#include "create_scene.cuh"
#include "path_tracing.cuh"

#include <unistd.h>

thread_local uint3 blockIdx, threadIdx;
thread_local dim3 blockDim, gridDim;

float erfinvf(float p)
{
    if (p == 0.95f) return 1.3859037160873413f;
    double y = (double)p, x = 0.0;
    for (int it = 0; it < 100; ++it) {
        double fx = erf(x) - y;
        double d = 1.1283791670955126 * exp(-x * x);
        double nx = x - fx / d;
        if (nx == x) break;
        x = nx;
    }
    return (float)x;
}

static_assert(sizeof(Triangle) == 152 && sizeof(KD_Tree_Node) == 20 && sizeof(Material) == 56, "reference layout");

/* ------------------------------------------------------------ scene file */
struct MeshLine {
    std::string obj, mat;
    float ox, oy, oz, yaw, pitch, scale;
    int smooth;
};
static std::vector<MeshLine> g_meshes; /* what create_models() lists */
static std::string g_error;

struct RefScene {
    Scene scene;
    int nodes, indices;
};

std::vector<Triangle> create_models()
{
    std::vector<Triangle> triangles(0);
    for (const MeshLine &m : g_meshes)
        load_mesh(m.obj, m.mat, triangles, {{m.ox, m.oy, m.oz}, rotation_matrix(m.yaw, m.pitch) * m.scale}, m.smooth != 0);
    return triangles;
}

static bool readable(const std::string &p)
{
    std::ifstream f(p);
    return f.good();
}

/* the number after `label` in what create_scene() printed */
static int printed_count(const std::string &text, const std::string &label)
{
    size_t k = text.find(label);
    return k == std::string::npos ? -1 : std::stoi(text.substr(k + label.size()));
}

extern "C" {

const char *ref_last_error(void) { return g_error.c_str(); }

/* scene text file (the project's: `mesh obj mat ox oy oz yaw pitch scale smooth`
 * and `camera x y z yaw pitch fov aperture` lines) -> the reference's Scene.
 * The reference opens texture paths as written in the .mat file, relative to
 * the working directory, so the scene is loaded from its own directory. */
RefScene *ref_scene_load(const char *scene_path, float camera_out[7])
{
    std::string path(scene_path);
    std::ifstream file(path);
    if (!file.good()) {
        g_error = "cannot open " + path;
        return nullptr;
    }
    size_t slash = path.rfind('/');
    std::string dir = slash == std::string::npos ? "." : path.substr(0, slash);
    char cwd[4096];
    if (!getcwd(cwd, sizeof cwd) || chdir(dir.c_str()) != 0) {
        g_error = "cannot enter " + dir;
        return nullptr;
    }
    g_meshes.clear();
    bool ok = true;
    std::string line;
    try {
        while (ok && getline(file, line)) {
            std::vector<std::string> s = split_string(line, ' ');
            if (s.size() == 0 || s[0][0] == '#') continue;
            if (s[0] == "mesh" && s.size() == 10) {
                g_meshes.push_back({s[1], s[2], std::stof(s[3]), std::stof(s[4]), std::stof(s[5]), std::stof(s[6]),
                                    std::stof(s[7]), std::stof(s[8]), std::stoi(s[9])});
                if (!readable(s[1]) || !readable(s[2])) {
                    g_error = "cannot open " + s[1] + " or " + s[2];
                    ok = false;
                }
            } else if (s[0] == "camera" && s.size() == 8) {
                for (int k = 0; k < 7; ++k) camera_out[k] = std::stof(s[k + 1]);
            } else {
                g_error = "bad scene line: " + line;
                ok = false;
            }
        }
    } catch (const std::exception &e) {
        g_error = "bad number in: " + line;
        ok = false;
    }
    if (ok && g_meshes.empty()) {
        g_error = "empty scene " + path;
        ok = false;
    }
    RefScene *out = nullptr;
    if (ok) {
        /* create_scene() and create_kd_tree() print their counts; the Scene
         * itself does not carry the node and index counts */
        std::ostringstream printed;
        std::streambuf *old = std::cout.rdbuf(printed.rdbuf());
        Scene scene = create_scene();
        std::cout.rdbuf(old);
        out = new RefScene{scene, printed_count(printed.str(), "node count: "),
                           printed_count(printed.str(), "triangle index count: ")};
        /* sample_direct_light reads light_indicies[light_count] when its draw
         * is 1.0 (one past the list: undefined in the reference).  The project
         * defines that entry as the last light; so does this list. */
        if (scene.light_count > 0) {
            int *padded;
            cudaMalloc(&padded, (scene.light_count + 1) * sizeof(int));
            cudaMemcpy(padded, scene.light_indicies, scene.light_count * sizeof(int), cudaMemcpyDeviceToDevice);
            padded[scene.light_count] = padded[scene.light_count - 1];
            cudaFree(scene.light_indicies);
            out->scene.light_indicies = padded;
        }
    }
    if (chdir(cwd) != 0) g_error = "cannot return to the working directory";
    return out;
}

void ref_scene_free(RefScene *s)
{
    if (!s) return;
    std::set<void *> texels;
    for (int i = 0; i < s->scene.triangle_count; ++i) texels.insert(s->scene.triangles[i].material.texture.buffer);
    for (void *p : texels) cudaFree(p);
    cudaFree(s->scene.triangles);
    cudaFree(s->scene.light_indicies);
    cudaFree(s->scene.kd_tree.nodes);
    cudaFree(s->scene.kd_tree.triangle_indicies);
    delete s;
}

int ref_scene_counts(const RefScene *s, int *triangles, int *nodes, int *indices, int *lights)
{
    *triangles = s->scene.triangle_count;
    *nodes = s->nodes;
    *indices = s->indices;
    *lights = s->scene.light_count;
    return 0;
}

/* the reference's bytes: 152 B triangles, 20 B nodes, indices, lights,
 * bounds[6]; padding bytes zeroed so that comparisons are byte-exact */
void ref_scene_copy(const RefScene *s, void *triangles152, void *nodes20, int *indices, int *lights, float bounds[6])
{
    const Scene &sc = s->scene;
    if (triangles152) {
        memcpy(triangles152, sc.triangles, (size_t)sc.triangle_count * sizeof(Triangle));
        const size_t pad = offsetof(Triangle, material) + offsetof(Material, transparent) + sizeof(bool);
        for (int i = 0; i < sc.triangle_count; ++i)
            memset((char *)triangles152 + (size_t)i * sizeof(Triangle) + pad, 0,
                   offsetof(Triangle, material) + offsetof(Material, texture) - pad);
    }
    if (nodes20) {
        memcpy(nodes20, sc.kd_tree.nodes, (size_t)s->nodes * sizeof(KD_Tree_Node));
        for (int i = 0; i < s->nodes; ++i) {
            char *n = (char *)nodes20 + (size_t)i * sizeof(KD_Tree_Node);
            const size_t axis_end = offsetof(KD_Tree_Node, plane_axis) + sizeof(uint8_t);
            const size_t leaf_end = offsetof(KD_Tree_Node, is_leaf_node) + sizeof(bool);
            memset(n + axis_end, 0, offsetof(KD_Tree_Node, plane_offset) - axis_end);
            memset(n + leaf_end, 0, sizeof(KD_Tree_Node) - leaf_end);
        }
    }
    if (indices) memcpy(indices, sc.kd_tree.triangle_indicies, (size_t)s->indices * sizeof(int));
    if (lights) memcpy(lights, sc.light_indicies, (size_t)sc.light_count * sizeof(int));
    if (bounds) {
        const Bounding_Box &b = sc.kd_tree.bounding_box;
        bounds[0] = b.min.x; bounds[1] = b.min.y; bounds[2] = b.min.z;
        bounds[3] = b.max.x; bounds[4] = b.max.y; bounds[5] = b.max.z;
    }
}

/* the G_Buffer constructor's seeds (screen.cuh) for a width x height frame */
void ref_seeds(int width, int height, uint32_t *out)
{
    ref_screen_w = width;
    ref_screen_h = height;
    G_Buffer g;
    memcpy(out, g.random_numbers, (size_t)width * height * sizeof(uint32_t));
    cudaFree(g.frame_buffer);
    cudaFree(g.squared_luminance);
    cudaFree(g.sample_count);
    cudaFree(g.random_numbers);
}

/* a G_Buffer over the caller's arrays (the type has no other constructor: one is made once and copied) */
static G_Buffer g_buffer_over(float *fb, float *sq, int *count, uint32_t *rng)
{
    static G_Buffer *made = nullptr;
    if (!made) {
        int w = ref_screen_w, h = ref_screen_h;
        ref_screen_w = ref_screen_h = 1;
        made = new G_Buffer();
        ref_screen_w = w;
        ref_screen_h = h;
    }
    G_Buffer g = *made;
    g.frame_buffer = (Vec3D *)fb;
    g.squared_luminance = sq;
    g.sample_count = count;
    g.random_numbers = rng;
    return g;
}

/* trace_ray for n rays (o.xyz, d.xyz); out per ray, as floats: hit, triangle_index, albedo3, emittance3,
 * roughness, refractive_index, extinction, transparent, position3, normal3, tangent3, bitangent3 (24);
 * a miss reports triangle -1 and the Sample as trace_ray left it (zeroed before the call) */
void ref_trace_rays(const RefScene *s, const float *rays6, int n, float *out24)
{
    for (int i = 0; i < n; ++i) {
        const float *r = rays6 + 6 * (size_t)i;
        Ray ray = {{r[0], r[1], r[2]}, {r[3], r[4], r[5]}};
        Sample sm;
        memset(&sm, 0, sizeof sm);
        bool hit = trace_ray(ray, s->scene, sm);
        float *o = out24 + 24 * (size_t)i;
        o[0] = hit;
        o[1] = hit ? sm.triangle_index : -1;
        o[2] = sm.albedo.x; o[3] = sm.albedo.y; o[4] = sm.albedo.z;
        o[5] = sm.emittance.x; o[6] = sm.emittance.y; o[7] = sm.emittance.z;
        o[8] = sm.roughness; o[9] = sm.refractive_index; o[10] = sm.extinction; o[11] = sm.transparent;
        o[12] = sm.position.x; o[13] = sm.position.y; o[14] = sm.position.z;
        o[15] = sm.normal.x; o[16] = sm.normal.y; o[17] = sm.normal.z;
        o[18] = sm.tangent.x; o[19] = sm.tangent.y; o[20] = sm.tangent.z;
        o[21] = sm.bitangent.x; o[22] = sm.bitangent.y; o[23] = sm.bitangent.z;
    }
}

/* get_scattered_light for n inputs, laid out as or_scatter's: ray_dir[3], sample[22], inside, rng;
 * out[9] = ray position3, direction3, weight3 */
void ref_scatter(const float *ray_dir3, const float *sample22, const int *inside, const uint32_t *rng, int n,
                 float *out9, uint32_t *rng_out, int *inside_out, int *type_out)
{
    for (int i = 0; i < n; ++i) {
        const float *d = ray_dir3 + 3 * (size_t)i, *v = sample22 + 22 * (size_t)i;
        Sample sm;
        memset(&sm, 0, sizeof sm);
        sm.albedo = {v[0], v[1], v[2]};
        sm.emittance = {v[3], v[4], v[5]};
        sm.roughness = v[6];
        sm.refractive_index = v[7];
        sm.extinction = v[8];
        sm.transparent = v[9] != 0.0f;
        sm.position = {v[10], v[11], v[12]};
        sm.normal = {v[13], v[14], v[15]};
        sm.tangent = {v[16], v[17], v[18]};
        sm.bitangent = {v[19], v[20], v[21]};
        bool in = inside[i] != 0;
        uint32_t state = rng[i];
        Scattering_Event e = get_scattered_light({d[0], d[1], d[2]}, in, g_buffer_over(nullptr, nullptr, nullptr, &state),
                                                 0, sm);
        float *o = out9 + 9 * (size_t)i;
        o[0] = e.ray.position.x; o[1] = e.ray.position.y; o[2] = e.ray.position.z;
        o[3] = e.ray.direction.x; o[4] = e.ray.direction.y; o[5] = e.ray.direction.z;
        o[6] = e.weight.x; o[7] = e.weight.y; o[8] = e.weight.z;
        rng_out[i] = state;
        inside_out[i] = in;
        type_out[i] = e.type;
    }
}

/* sample_direct_light at n shading points; out[3] radiance, rng advanced in place */
void ref_direct_light(const RefScene *s, const float *pos3, const float *normal3, uint32_t *rng, int n, float *out3)
{
    for (int i = 0; i < n; ++i) {
        const float *p = pos3 + 3 * (size_t)i, *nr = normal3 + 3 * (size_t)i;
        Vec3D r = sample_direct_light({p[0], p[1], p[2]}, {nr[0], nr[1], nr[2]}, s->scene,
                                      g_buffer_over(nullptr, nullptr, nullptr, rng + i), 0);
        out3[3 * (size_t)i] = r.x;
        out3[3 * (size_t)i + 1] = r.y;
        out3[3 * (size_t)i + 2] = r.z;
    }
}

/* path_tracing() over `passes` passes on the caller's G_Buffer arrays, one 3x3
 * cell per call as one CUDA thread runs it; sample_count_arg == 0 zeroes
 * frame_buffer, squared_luminance and sample_count first, as render() does
 * with reset_frame (render.cuh itself cannot be included: <<< >>> does not
 * parse).  width and height must be multiples of the cell: the kernel has no
 * bounds guard.  adaptive == 0 turns the adaptive test off with a MIN_SAMPLES
 * no pixel reaches. */
int ref_render(const RefScene *s, const float camera7[7], float *frame_buffer, float *squared_luminance,
               int *sample_count, uint32_t *random_numbers, int width, int height, int passes, int sample_count_arg,
               int adaptive, int min_samples, float tolerance)
{
    if (width <= 0 || height <= 0 || width % SCREEN_CELL_W || height % SCREEN_CELL_H) {
        g_error = "width and height must be multiples of the screen cell";
        return -1;
    }
    ref_screen_w = width;
    ref_screen_h = height;
    ref_min_samples = adaptive ? min_samples : INT32_MAX;
    ref_max_tolerance = tolerance;
    Camera camera = {{camera7[0], camera7[1], camera7[2]}, camera7[3], camera7[4], camera7[5], camera7[6]};
    G_Buffer g = g_buffer_over(frame_buffer, squared_luminance, sample_count, random_numbers);
    if (sample_count_arg == 0) {
        memset(frame_buffer, 0, (size_t)width * height * sizeof(Vec3D));
        memset(squared_luminance, 0, (size_t)width * height * sizeof(float));
        memset(sample_count, 0, (size_t)width * height * sizeof(int));
    }
    blockDim = dim3(1, 1, 1);
    gridDim = dim3(width / SCREEN_CELL_W, height / SCREEN_CELL_H, 1);
    threadIdx = {0, 0, 0};
    for (int p = 0; p < passes; ++p)
        for (unsigned by = 0; by < gridDim.y; ++by)
            for (unsigned bx = 0; bx < gridDim.x; ++bx) {
                blockIdx = {bx, by, 0};
                path_tracing(g, s->scene, camera);
            }
    return 0;
}

/* correct_color on n colours */
void ref_correct_color(const float *in3, int n, float *out3)
{
    for (int i = 0; i < n; ++i) {
        Vec3D c = correct_color({in3[3 * (size_t)i], in3[3 * (size_t)i + 1], in3[3 * (size_t)i + 2]});
        out3[3 * (size_t)i] = c.x;
        out3[3 * (size_t)i + 1] = c.y;
        out3[3 * (size_t)i + 2] = c.z;
    }
}

/* The pixel of draw_frame (render.cuh) and save_render (save_render.cuh) ->
 * RGBA8, rows as in the frame buffer (save_render writes them bottom up).
 * Neither file can be included (<<< >>>), so their one colour statement has to
 * stand here: the mean with the reference's Vec3D * float, the reference's
 * correct_color, and the float -> byte conversion that passing a float to
 * make_uchar4 performs. */
void ref_tonemap(const float *frame_buffer, const int *sample_count, int n, uint8_t *rgba)
{
    const Vec3D *fb = (const Vec3D *)frame_buffer;
    for (int i = 0; i < n; ++i) {
        Vec3D color = correct_color(fb[i] * (1.0f / sample_count[i]));
        uchar4 c = make_uchar4(color.x * MAX_COLOR_CHANNEL, color.y * MAX_COLOR_CHANNEL, color.z * MAX_COLOR_CHANNEL,
                               MAX_COLOR_CHANNEL);
        rgba[4 * (size_t)i] = c.x;
        rgba[4 * (size_t)i + 1] = c.y;
        rgba[4 * (size_t)i + 2] = c.z;
        rgba[4 * (size_t)i + 3] = c.w;
    }
}

/* which libm the library was built with: 1 = the project's rt_libm.h (the pinned build), 0 = the host's */
int ref_uses_rt_libm(void)
{
#ifdef REF_GLIBC_LIBM
    return 0;
#else
    return 1;
#endif
}
}
