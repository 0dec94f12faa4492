// rt_launch.h — the host entry points that cross the library's HIP files:
// abi.hip calls them, the file named above each group defines them and
// includes this header too, so a signature that drifts is a compile error.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_device.h"

struct RtDnParams; // denoise_math.h
struct RtRpFrame;  // reproject_math.h
struct RtRpParams;
struct RtRpLens;
struct RtDevSampler; // sampler_math.h
struct RtCvParams;   // convergence_math.h

// path_kernel.hip: the megakernel and rt_tonemap
int rt_launch_path(const RtDevScene &sc, const RtDevFrame &fr, const RtDevCamera &cam, int stack_depth,
                   hipStream_t stream, int traversal);
int rt_launch_tonemap(const Vec3D *fb, const int *count, RtUChar4 *out, int n, hipStream_t stream);
void rt_path_shutdown();

// wavefront.hip: rt_render's wavefront kernels (o.kernel 1..3) on o.stream; it reads the options' wf_*, traversal,
// profile, overlap, check_interval, coalesce_passes and debug fields and applies their defaults itself
int rt_launch_wavefront(const RtDevScene &sc, const RtDevFrame &fr, const RtDevCamera &cam, const RtOptions &o);
int rt_wavefront_device_init();
int rt_wavefront_join(void *stream, int consume); // 0, -1 (a HIP failure) or RT_WAVEFRONT_INCOMPLETE
const char *rt_wavefront_incomplete_msg();
void rt_wavefront_shutdown();

// query.hip
int rt_launch_trace_rays(const RtDevScene &sc, const float *rays, long long n, void *hits, void *surface, int traversal,
                         unsigned long long *stats, hipStream_t stream);
int rt_launch_render_aov(const RtDevScene &sc, const RtDevCamera &cam, int width, int height, float *depth,
                         float *normal, float *albedo, int *triangle, int traversal, unsigned long long *stats,
                         hipStream_t stream);
int rt_launch_camera_rays(const RtDevCamera &cam, int width, int height, float *rays, hipStream_t stream);
int rt_launch_occluded(const RtDevScene &sc, const float *rays, const float *tmax, long long n, uint8_t *occluded,
                       int traversal, unsigned long long *stats, hipStream_t stream);
int rt_launch_trace_paths(const RtDevScene &sc, const float *rays, uint32_t *rng, long long n, float *radiance, float *sq,
                          int samples, int max_depth, int accumulate, int traversal, unsigned long long *stats,
                          hipStream_t stream);
// (adaptive: NULL = every element takes every sample; else rt_sample_paths_adaptive's test, sq and count given)
int rt_launch_sample_paths(const RtDevScene &sc, const RtDevSampler &smp, uint32_t *rng, long long n, float *radiance,
                           float *sq, int *count, int samples, int max_depth, int accumulate, int traversal,
                           unsigned long long *stats, hipStream_t stream, const RtCvParams *adaptive);
int rt_launch_sampler_rays(const RtDevSampler &smp, uint32_t *rng, long long n, float *rays, hipStream_t stream);
void rt_query_shutdown();

// denoise.hip (wrap_x: the x axis is periodic — rt_denoise_sampler's EQUIRECT frames)
int rt_launch_denoise(const Vec3D *fb, const float *sq, const int *count, const float *depth, const float *normal,
                      const float *albedo, int width, int height, float *rgb_out, const RtDnParams &prm,
                      hipStream_t stream, int wrap_x);
int rt_launch_tonemap_rgb(const float *rgb, RtUChar4 *out, int n, hipStream_t stream);
void rt_denoise_shutdown();

// reproject.hip (model: RT_SAMPLER_PINHOLE .. RT_SAMPLER_ORTHO, the two cameras' model; lens: what the models
// beside the pinhole read of the samplers)
int rt_launch_reproject(const RtRpFrame &src, const RtDevCamera &src_cam, const float *dst_depth,
                        const float *dst_normal, const int *dst_triangle, const RtDevCamera &dst_cam, int width,
                        int height, const RtRpParams &prm, Vec3D *fb_out, float *sq_out, int *count_out,
                        unsigned long long *stats, hipStream_t stream, int model, const RtRpLens &lens);
// query.hip: rt_sample_aov — the sampler's centre rays into the AOV buffers
int rt_launch_sample_aov(const RtDevScene &sc, const RtDevSampler &smp, long long n, float *depth, float *normal,
                         float *albedo, int *triangle, int traversal, unsigned long long *stats, hipStream_t stream);

// convergence.hip
int rt_launch_convergence(const float *radiance, const float *sq, const int *count, long long n, const RtCvParams &prm,
                          float *rel_error, unsigned long long *stats, hipStream_t stream);

// abi.hip: rt_shutdown at exit, before the HIP runtime's finalisers
void rt_register_shutdown();
