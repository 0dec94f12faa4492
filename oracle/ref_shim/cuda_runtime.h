/*
 * TEST INFRASTRUCTURE ONLY — stand-in for <cuda_runtime.h>, so that the
 * reference's own headers compile as plain host C++ (oracle/Makefile.ref).
 * Only declarations of ours: the few names the reference's render path uses.
 * "Device" memory is host memory.
 */
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>

#define __host__
#define __device__
#define __global__

struct uchar4 { unsigned char x, y, z, w; };
struct uint3 { unsigned int x, y, z; };
struct uint4 { unsigned int x, y, z, w; };
struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};

static inline uchar4 make_uchar4(unsigned char x, unsigned char y, unsigned char z, unsigned char w)
{
    return uchar4{x, y, z, w};
}
static inline uint4 make_uint4(unsigned int x, unsigned int y, unsigned int z, unsigned int w)
{
    return uint4{x, y, z, w};
}

/* the launch coordinates a kernel reads; the harness sets them per cell */
extern thread_local uint3 blockIdx, threadIdx;
extern thread_local dim3 blockDim, gridDim;

typedef int cudaError_t;
typedef unsigned long long cudaSurfaceObject_t;
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };

/* The reference reads one element past two of its buffers: texel index
 * width * height (+ width) when mod(uv, 1) returns 1.0 (trace_ray.cuh
 * sample_texture) and light_indicies[light_count] when the light pick draws
 * 1.0 (path_tracing.cuh sample_direct_light).  What a CUDA allocation holds
 * there is undefined; every allocation here is zero-filled and carries zeroed
 * slack, so those reads stay inside it.  Zero texels are the project's
 * convention for the first read; the harness states the second one itself. */
#define REF_SHIM_SLACK (64 * 1024)

template <typename T> static inline cudaError_t cudaMalloc(T **p, size_t bytes)
{
    /* cudaMalloc(0) gives NULL: a texture file that stbi_load cannot open leaves its material untextured */
    *p = bytes ? (T *)calloc(1, bytes + REF_SHIM_SLACK) : nullptr;
    return (*p || !bytes) ? 0 : 2;
}
static inline cudaError_t cudaMemcpy(void *dst, const void *src, size_t bytes, cudaMemcpyKind)
{
    if (bytes) memcpy(dst, src, bytes);
    return 0;
}
static inline cudaError_t cudaFree(void *p)
{
    free(p);
    return 0;
}

/* erfinvf (libdevice's in the reference): path_tracing() calls it with
 * 1 - MAX_TOLERANCE only.  The same values as rt_adaptive_z (rt_libm.h): the
 * correctly rounded erfinvf(0.95f), otherwise Newton steps on erf in double. */
float erfinvf(float p);
