// rt_render — the reference's main() (rt/main.cu:60-155) without the GLFW
// window: C++ host code over the C-ABI of include/isaklm_rt.h.
//
//   G_Buffer g_buffer = G_Buffer();            -> rt_gbuffer_create
//   Scene scene = create_scene();              -> rt_host_scene_load_file (create_models as data)
//                                                 + rt_create_scene + rt_scene_prepare
//   Camera camera = {...}                      -> the scene file's camera line (or the reference's)
//   call_render(...); ++sample_count;          -> rt_render with `passes` passes per call
//   if (sample_count >= MAX_SAMPLES) save_render(g_buffer)  -> rt_save_render
//
// usage: rt_render [--scene FILE | --generate NAME DIR] [--width W] [--height H]
//                  [--spp N] [--passes P] [--adaptive 0|1] [--min-samples N]
//                  [--tolerance T] [--max-depth D] [--kernel mega|wavefront]
//                  [--shard G N] [--device D] [--out PNG] [--quiet]
//                  [--checkpoint FILE] [--resume FILE] [--aov PREFIX] [--denoise]
//                  [--reproject-to "PX PY PZ YAW PITCH" [--spp2 N]]
//                  [--camera-model pinhole|equirect|fisheye|ortho] [--ortho-half-width X]
//                  [--until-converged] [--error-map PFM]
// --until-converged asks rt_convergence after every call and stops as soon as
// the adaptive test (--min-samples, --tolerance) would sample no pixel again —
// or at --spp, whichever comes first — where the reference's main() keeps
// launching passes that sample nothing until MAX_SAMPLES.  A converged frame
// takes no further sample, so the image is the one a full --adaptive 1 --spp N
// render writes.  It needs the adaptive test: --adaptive 0 with it is a usage
// error; with --camera-model the frame is rendered by rt_sample_paths_adaptive.
// It is a usage error with --reproject-to or --shard (a shard sees its rows only).
// --error-map writes rt_convergence's relative-error map of the shown frame
// (Pf, --aov's depth layout; inf = fewer than 2 samples).
// --camera-model renders the frame through rt_sample_paths instead of
// rt_render: each call draws --passes samples per pixel from the model's
// sampler (RT_SAMPLER_*; fisheye reads the camera's FOV as the angle across the
// image circle, ortho takes --ortho-half-width world units, default 2) into
// the G_Buffer's four arrays, so --checkpoint, --resume and --out work
// unchanged.  That path runs the adaptive test under --until-converged only and renders whole
// frames of one camera: with an explicit --adaptive 1, --shard or --reproject-to the
// flag is a usage error, and so is a model other than pinhole with --aov or
// --denoise (those buffers are the pinhole camera's).
// --reproject-to moves the camera after the --spp samples (FOV and aperture
// stay): instead of the reference's reset the frame is carried over to the new
// camera (rt_reproject, guided by rt_render_aov of both cameras) into a second
// G_Buffer that shares the first one's RNG array, --spp2 more samples are
// rendered on top, and --out (and --denoise's image) show that second frame.
// --aov writes the first-hit feature buffers of the pixel-centre rays
// (rt_render_aov) before the render loop: PREFIX.albedo.pfm and
// PREFIX.normal.pfm (PF, 3 floats per pixel) and PREFIX.depth.pfm (Pf; inf =
// no hit), little-endian, rows bottom to top (the G_Buffer's orientation).
// --denoise writes, beside the unchanged --out image, <out stem>.denoised.png:
// the frame through rt_denoise (guided by the same first-hit buffers; --aov's
// are reused) and rt_tonemap_rgb, flipped as save_render flips.
// --checkpoint writes the G_Buffer + sample count after every rt_render call
// (rt_gbuffer_save); --resume continues from such a file (rt_gbuffer_load),
// bit-identical to a render that never stopped.
// Defaults are the reference's macros (rt/macros.h): 1920x1080, MAX_SAMPLES
// 5000, MIN_SAMPLES 100, MAX_TOLERANCE 0.05, adaptive sampling on.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "isaklm_rt.h"

namespace {

int fail(const char *what)
{
    fprintf(stderr, "rt_render: %s: %s\n", what, rt_last_error());
    return 1;
}

void usage()
{
    fprintf(stderr,
            "usage: rt_render [--scene FILE | --generate NAME DIR] [--width W] [--height H] [--spp N]\n"
            "                 [--passes P] [--adaptive 0|1] [--min-samples N] [--tolerance T] [--max-depth D]\n"
            "                 [--kernel mega|wavefront] [--shard G N] [--device D] [--out PNG] [--quiet]\n"
            "                 [--checkpoint FILE] [--resume FILE] [--aov PREFIX] [--denoise]\n"
            "                 [--reproject-to \"PX PY PZ YAW PITCH\" [--spp2 N]]\n"
            "                 [--camera-model pinhole|equirect|fisheye|ortho] [--ortho-half-width X]\n"
            "                 [--until-converged] [--error-map PFM]\n");
}

// PFM: "PF" (3 channels) or "Pf" (1), width height, a negative scale = little-endian, rows bottom to top
bool write_pfm(const std::string &path, const float *data, int width, int height, int channels)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "%s\n%d %d\n-1.0\n", channels == 3 ? "PF" : "Pf", width, height);
    const size_t n = (size_t)width * height * channels;
    const bool ok = fwrite(data, sizeof(float), n, f) == n;
    return fclose(f) == 0 && ok;
}

// the first-hit feature buffers of the pixel-centre rays (rt_render_aov) in device memory
int render_aovs(rt_scene_t scene, Camera camera, int width, int height, RtAovBuffers *b)
{
    const size_t n = (size_t)width * height;
    if (rt_device_alloc((void **)&b->depth, n * 4) != RT_OK || rt_device_alloc((void **)&b->normal, n * 12) != RT_OK ||
        rt_device_alloc((void **)&b->albedo, n * 12) != RT_OK)
        return fail("aov buffers");
    if (rt_render_aov(scene, camera, width, height, b, nullptr) != RT_OK) return fail("render_aov");
    return 0;
}

void free_aovs(RtAovBuffers *b)
{
    if (b->depth) rt_free(b->depth);
    if (b->normal) rt_free(b->normal);
    if (b->albedo) rt_free(b->albedo);
    if (b->triangle) rt_free(b->triangle);
    b->depth = b->normal = b->albedo = nullptr;
    b->triangle = nullptr;
}

// render_aovs plus the triangle ids: rt_reproject's guides
int render_guides(rt_scene_t scene, Camera camera, int width, int height, RtAovBuffers *b)
{
    if (rt_device_alloc((void **)&b->triangle, (size_t)width * height * 4) != RT_OK) return fail("aov buffers");
    return render_aovs(scene, camera, width, height, b);
}

// --aov: the buffers downloaded and written as PFM files
int write_aovs(const RtAovBuffers &b, int width, int height, const std::string &prefix)
{
    const size_t n = (size_t)width * height;
    std::vector<float> host(n * 3);
    const struct { const char *name; const float *dev; int channels; } planes[3] = {
        {"albedo", b.albedo, 3}, {"normal", b.normal, 3}, {"depth", b.depth, 1}};
    for (const auto &pl : planes) {
        if (rt_download(host.data(), pl.dev, n * pl.channels * sizeof(float)) != RT_OK) return fail("aov download");
        const std::string path = prefix + "." + pl.name + ".pfm";
        if (!write_pfm(path, host.data(), width, height, pl.channels)) {
            fprintf(stderr, "rt_render: cannot write %s\n", path.c_str());
            return 1;
        }
    }
    return 0;
}

// "dir/x.png" -> "dir/x.denoised.png" (a name without an extension gets the suffix appended)
std::string denoised_path(const std::string &out)
{
    const size_t slash = out.find_last_of('/');
    const size_t dot = out.find_last_of('.');
    const bool has_ext = dot != std::string::npos && (slash == std::string::npos || dot > slash + 1);
    return (has_ext ? out.substr(0, dot) : out) + ".denoised.png";
}

// --denoise: rt_denoise -> rt_tonemap_rgb -> PNG with save_render's vertical flip (rt/save_render.cuh:55)
int write_denoised(G_Buffer g_buffer, const RtAovBuffers &b, int width, int height, const std::string &path)
{
    const size_t n = (size_t)width * height;
    float *rgb = nullptr;
    uint8_t *rgba = nullptr;
    if (rt_device_alloc((void **)&rgb, n * 12) != RT_OK || rt_device_alloc((void **)&rgba, n * 4) != RT_OK)
        return fail("denoise buffers");
    if (rt_denoise(g_buffer, &b, width, height, rgb, nullptr) != RT_OK) return fail("denoise");
    if (rt_tonemap_rgb(rgb, rgba, width, height, nullptr) != RT_OK) return fail("tonemap_rgb");
    std::vector<uint8_t> img(n * 4), flipped(n * 4);
    if (rt_download(img.data(), rgba, n * 4) != RT_OK) return fail("denoised download");
    rt_free(rgb);
    rt_free(rgba);
    for (int y = 0; y < height; ++y)
        memcpy(&flipped[(size_t)(height - y - 1) * width * 4], &img[(size_t)y * width * 4], (size_t)width * 4);
    if (rt_write_png(path.c_str(), flipped.data(), width, height) != RT_OK) return fail("write denoised png");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    std::string scene_path, gen_name, gen_dir, out = "render.png", checkpoint, resume, aov, reproject_to;
    int width = 1920, height = 1080, spp = 5000, passes = 64, adaptive = 1, min_samples = 100, max_depth = 0;
    int spp2 = 0;
    int device = 0, shard_id = 0, num_shards = 1, kernel = RT_KERNEL_WAVEFRONT;
    int camera_model = -1; // RT_SAMPLER_*; -1: rt_render
    float tolerance = 0.05f, ortho_half_width = 2.0f;
    bool quiet = false, denoise = false, adaptive_given = false, shard_given = false, until_converged = false;
    std::string error_map;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&](void) -> const char * {
            if (i + 1 >= argc) {
                usage();
                exit(2);
            }
            return argv[++i];
        };
        if (a == "--scene") scene_path = next();
        else if (a == "--generate") { gen_name = next(); gen_dir = next(); }
        else if (a == "--width") width = atoi(next());
        else if (a == "--height") height = atoi(next());
        else if (a == "--spp") spp = atoi(next());
        else if (a == "--passes") passes = atoi(next());
        else if (a == "--adaptive") { adaptive = atoi(next()); adaptive_given = true; }
        else if (a == "--min-samples") min_samples = atoi(next());
        else if (a == "--tolerance") tolerance = (float)atof(next());
        else if (a == "--max-depth") max_depth = atoi(next());
        else if (a == "--kernel") kernel = std::string(next()) == "mega" ? RT_KERNEL_MEGA : RT_KERNEL_WAVEFRONT;
        else if (a == "--shard") { shard_id = atoi(next()); num_shards = atoi(next()); shard_given = true; }
        else if (a == "--device") device = atoi(next());
        else if (a == "--out") out = next();
        else if (a == "--quiet") quiet = true;
        else if (a == "--checkpoint") checkpoint = next();
        else if (a == "--resume") resume = next();
        else if (a == "--aov") aov = next();
        else if (a == "--denoise") denoise = true;
        else if (a == "--reproject-to") reproject_to = next();
        else if (a == "--spp2") spp2 = atoi(next());
        else if (a == "--camera-model") {
            const std::string m = next();
            camera_model = m == "pinhole" ? RT_SAMPLER_PINHOLE : m == "equirect" ? RT_SAMPLER_EQUIRECT
                           : m == "fisheye" ? RT_SAMPLER_FISHEYE : m == "ortho" ? RT_SAMPLER_ORTHO : -2;
        }
        else if (a == "--ortho-half-width") ortho_half_width = (float)atof(next());
        else if (a == "--until-converged") until_converged = true;
        else if (a == "--error-map") error_map = next();
        else {
            usage();
            return 2;
        }
    }
    if (scene_path.empty() == gen_name.empty() || width <= 0 || height <= 0 || spp <= 0 || passes <= 0 || spp2 < 0 ||
        (spp2 > 0 && reproject_to.empty())) {
        usage();
        return 2;
    }
    // the sampled path: whole frames of one camera, every pixel every sample; first-hit buffers are the pinhole's
    if (camera_model == -2 ||
        (camera_model >= 0 && ((adaptive_given && adaptive != 0) || shard_given || !reproject_to.empty())) ||
        (camera_model > RT_SAMPLER_PINHOLE && (!aov.empty() || denoise))) {
        usage();
        return 2;
    }
    // "is the frame done" is the adaptive test's question, asked of a whole frame of one camera
    if (until_converged && ((camera_model < 0 && adaptive == 0) || shard_given || !reproject_to.empty() || min_samples < 0)) {
        usage();
        return 2;
    }
    if (!error_map.empty() && min_samples < 0) {
        usage();
        return 2;
    }
    if (!gen_name.empty()) {
        char buf[4096];
        if (rt_generate_scene(gen_name.c_str(), gen_dir.c_str(), buf, sizeof buf) != RT_OK) return fail("generate");
        scene_path = buf;
    }
    if (rt_set_device(device) != RT_OK) return fail("set_device");

    // G_Buffer() (rt/screen.cuh:22-46); a row shard keeps the single-stream seeds
    G_Buffer g_buffer;
    if (rt_gbuffer_create(width, height, 0, &g_buffer) != RT_OK) return fail("G_Buffer");

    // create_scene() (rt/create_scene.cuh:18): create_models, create_kd_tree, upload
    const auto t0 = std::chrono::steady_clock::now();
    RtHostScene *host = nullptr;
    if (rt_host_scene_create(&host) != RT_OK) return fail("host scene");
    Camera camera = {{-2.1f, 1.7f, -1.2f}, 0.975f, 0.3f, 1.57079632679f, 0.002f}; // rt/main.cu:101-104
    if (rt_host_scene_load_file(host, scene_path.c_str(), &camera) != RT_OK) return fail("create_models");
    Scene scene;
    if (rt_create_scene(host, &scene, nullptr, nullptr) != RT_OK) return fail("create_scene");
    rt_scene_t prepared = nullptr;
    if (rt_scene_prepare(&scene, &prepared) != RT_OK) return fail("prepare"); // counts derived from the tree
    rt_host_scene_destroy(host);
    const double setup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    RtAovBuffers aov_buffers = {nullptr, nullptr, nullptr, nullptr};
    if (!aov.empty()) {
        if (render_aovs(prepared, camera, width, height, &aov_buffers) != 0) return 1;
        if (write_aovs(aov_buffers, width, height, aov) != 0) return 1;
        if (!denoise) free_aovs(&aov_buffers);
    }

    RtOptions opt;
    rt_default_options(&opt);
    opt.width = width;
    opt.height = height;
    opt.adaptive = adaptive;
    opt.min_samples = min_samples;
    opt.tolerance = tolerance;
    opt.max_depth = max_depth;
    opt.kernel = kernel;
    opt.shard_id = shard_id;
    opt.num_shards = num_shards;

    // the frame loop (rt/main.cu:114-155): call_render, ++sample_count, save at MAX_SAMPLES
    const auto t1 = std::chrono::steady_clock::now();
    int sample_count = 0;
    if (!resume.empty()) {
        if (rt_gbuffer_load(resume.c_str(), g_buffer, width, height, &sample_count) != RT_OK) return fail("resume");
        if (!quiet) printf("resumed at %d samples per pixel\n", sample_count);
    }
    const long long n_pixels = (long long)width * height;
    unsigned long long *conv_stats = nullptr; // --until-converged: rt_convergence's four words
    unsigned long long conv[4] = {0, 0, 0, 0};
    bool converged = false;
    if (until_converged && rt_device_alloc((void **)&conv_stats, sizeof conv) != RT_OK) return fail("convergence stats");
    const RtAdaptive adaptive_test = {min_samples, tolerance};
    while (sample_count < spp && !converged) {
        opt.passes = passes < spp - sample_count ? passes : spp - sample_count;
        if (camera_model >= 0) {
            const RtSampler sampler = {camera_model, width, height, camera, ortho_half_width, nullptr, nullptr};
            RtPathOptions po;
            rt_default_path_options(&po);
            po.samples = opt.passes;
            po.max_depth = max_depth;
            po.accumulate = sample_count > 0;
            if (rt_sample_paths_adaptive(prepared, &sampler, g_buffer.random_numbers, n_pixels,
                                         (float *)g_buffer.frame_buffer, g_buffer.squared_luminance,
                                         g_buffer.sample_count, &po, until_converged ? &adaptive_test : nullptr) != RT_OK)
                return fail("sample_paths");
        } else if (rt_render(prepared, g_buffer, camera, sample_count, &opt) != RT_OK) return fail("render");
        sample_count += opt.passes;
        if (!checkpoint.empty() && rt_gbuffer_save(g_buffer, width, height, sample_count, checkpoint.c_str()) != RT_OK)
            return fail("checkpoint");
        if (!quiet) printf("samples per pixel: %d\n", sample_count);
        if (until_converged) { // (rt_convergence joins the renders first)
            if (rt_memset(conv_stats, 0, sizeof conv) != RT_OK ||
                rt_convergence((const float *)g_buffer.frame_buffer, g_buffer.squared_luminance, g_buffer.sample_count,
                               n_pixels, min_samples, tolerance, nullptr, conv_stats, nullptr) != RT_OK ||
                rt_download(conv, conv_stats, sizeof conv) != RT_OK)
                return fail("convergence");
            converged = conv[1] == 0;
        }
    }
    if (rt_synchronize() != RT_OK) return fail("synchronize");
    const double render_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    // the samples the rate line counts: the ones actually taken where the driver knows them
    double samples_taken = (double)n_pixels * spp;
    if (until_converged && conv[0]) { // (no call ran if --resume already was at --spp: nothing to report then)
        samples_taken = (double)conv[3];
        if (converged)
            printf("converged after %d passes: %llu samples (mean %.2f per pixel)\n", sample_count, conv[3],
                   (double)conv[3] / (double)n_pixels);
        else
            printf("not converged: %llu pixels open\n", conv[1]);
    }
    if (conv_stats) rt_free(conv_stats);

    // --reproject-to: the camera moves; where main() resets (rt/main.cu:114-155) the frame is carried over
    G_Buffer moved = {nullptr, nullptr, nullptr, nullptr};
    if (!reproject_to.empty()) {
        Camera camera2 = camera;
        if (sscanf(reproject_to.c_str(), "%f %f %f %f %f", &camera2.position.x, &camera2.position.y,
                   &camera2.position.z, &camera2.yaw, &camera2.pitch) != 5) {
            usage();
            return 2;
        }
        const size_t n = (size_t)width * height;
        RtAovBuffers old_aov = {nullptr, nullptr, nullptr, nullptr};
        free_aovs(&aov_buffers); // (the first camera's: the denoised frame is the second camera's)
        if (render_guides(prepared, camera, width, height, &old_aov) != 0) return 1;
        if (render_guides(prepared, camera2, width, height, &aov_buffers) != 0) return 1;
        if (rt_device_alloc((void **)&moved.frame_buffer, n * 12) != RT_OK ||
            rt_device_alloc((void **)&moved.squared_luminance, n * 4) != RT_OK ||
            rt_device_alloc((void **)&moved.sample_count, n * 4) != RT_OK)
            return fail("reprojected G_Buffer");
        moved.random_numbers = g_buffer.random_numbers; // the per-pixel streams continue
        if (rt_reproject(g_buffer, &old_aov, camera, &aov_buffers, camera2, width, height, moved, nullptr) != RT_OK)
            return fail("reproject");
        free_aovs(&old_aov);
        for (int done = 0; done < spp2;) {
            opt.passes = passes < spp2 - done ? passes : spp2 - done;
            if (rt_render(prepared, moved, camera2, 1, &opt) != RT_OK) return fail("render after reprojection");
            done += opt.passes;
            if (!quiet) printf("samples per pixel after the move: +%d\n", done);
        }
        if (rt_synchronize() != RT_OK) return fail("synchronize");
        camera = camera2;
    }
    const G_Buffer shown = moved.frame_buffer ? moved : g_buffer;
    if (rt_save_render(shown, width, height, out.c_str()) != RT_OK) return fail("save_render");
    if (until_converged)
        printf("rendered %dx%d x %d passes in %.3f s (%.2f Msamples/s taken; scene setup %.2f s) -> %s\n", width, height,
               sample_count, render_s, samples_taken / render_s / 1e6, setup_s, out.c_str());
    else
        printf("rendered %dx%d x %d spp in %.3f s (%.2f Msamples/s nominal; scene setup %.2f s) -> %s\n", width,
               height, spp, render_s, samples_taken / render_s / 1e6, setup_s, out.c_str());
    if (!error_map.empty()) {
        float *err = nullptr;
        std::vector<float> host((size_t)n_pixels);
        if (rt_device_alloc((void **)&err, (size_t)n_pixels * 4) != RT_OK) return fail("error map");
        if (rt_convergence((const float *)shown.frame_buffer, shown.squared_luminance, shown.sample_count, n_pixels,
                           min_samples, tolerance, err, nullptr, nullptr) != RT_OK ||
            rt_download(host.data(), err, (size_t)n_pixels * 4) != RT_OK)
            return fail("error map");
        rt_free(err);
        if (!write_pfm(error_map, host.data(), width, height, 1)) {
            fprintf(stderr, "rt_render: cannot write %s\n", error_map.c_str());
            return 1;
        }
    }
    if (denoise) {
        if (!aov_buffers.depth && render_aovs(prepared, camera, width, height, &aov_buffers) != 0) return 1;
        const std::string path = denoised_path(out);
        if (write_denoised(shown, aov_buffers, width, height, path) != 0) return 1;
        if (!quiet) printf("denoised -> %s\n", path.c_str());
    }
    free_aovs(&aov_buffers);
    if (moved.frame_buffer) {
        rt_free(moved.frame_buffer);
        rt_free(moved.squared_luminance);
        rt_free(moved.sample_count);
    }

    rt_scene_release(prepared);
    rt_destroy_scene(&scene);
    rt_gbuffer_destroy(&g_buffer);
    return 0;
}
