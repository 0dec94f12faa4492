// rt_launch.h — the render path's host entry points that cross its HIP files
// (abi.hip, path_kernel.hip, wavefront.hip): declared once, here.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_device.h"

// path_kernel.hip: the megakernel
int rt_launch_path(const RtDevScene &sc, const RtDevFrame &fr, const RtDevCamera &cam, int stack_depth,
                   hipStream_t stream, int traversal);

// wavefront.hip: rt_render's wavefront kernels (o.kernel 1..3) on o.stream; it reads the options' wf_*, traversal,
// profile, overlap, check_interval, coalesce_passes and debug fields and applies their defaults itself
int rt_launch_wavefront(const RtDevScene &sc, const RtDevFrame &fr, const RtDevCamera &cam, const RtOptions &o);
int rt_wavefront_device_init();
int rt_wavefront_join(void *stream, int consume); // 0, -1 (a HIP failure) or RT_WAVEFRONT_INCOMPLETE
const char *rt_wavefront_incomplete_msg();
void rt_wavefront_shutdown();

// abi.hip: rt_shutdown at exit, before the HIP runtime's finalisers
void rt_register_shutdown();
