// camera_math.h — the camera's frame constants and its pixel-centre ray, one
// text for the host (abi.hip, host/reproject_host.cpp) and the gfx950 kernels
// (query.hip, reproject.hip).  Every includer is built with -ffp-contract=off.
#pragma once

#include "rt_device.h"
#include "rt_vecmath.h"

// Camera::rotation() and tanf(FOV / 2) are frame constants (rt/camera.cuh:22-25, :381).  Host only: the
// trigonometry never runs on the device.
inline RtDevCamera rt_device_camera(const Camera &cam)
{
    RtDevCamera dc;
    RtM3 R = rt_rotation_matrix(cam.yaw, cam.pitch);
    dc.R[0] = R.i.x; dc.R[1] = R.i.y; dc.R[2] = R.i.z;
    dc.R[3] = R.j.x; dc.R[4] = R.j.y; dc.R[5] = R.j.z;
    dc.R[6] = R.k.x; dc.R[7] = R.k.y; dc.R[8] = R.k.z;
    dc.pos[0] = cam.position.x; dc.pos[1] = cam.position.y; dc.pos[2] = cam.position.z;
    dc.tan_half_fov = rt_tanf(cam.FOV / 2);
    dc.aperture = cam.aperture_radius;
    return dc;
}

// rt_device_camera for a camera that may hold any floats.  The library's trigonometry reduces its argument through
// an int (rt_libm.h rt_reduce_pio2: angles of a few radians): a NaN, infinite or absurd angle never reaches it — such
// a camera gets NaN constants, which fail every compare made on them.
#define RT_CAMERA_MAX_ANGLE 524288.0f // 2^19
inline RtDevCamera rt_device_camera_checked(const Camera &cam)
{
    if (fabsf(cam.yaw) <= RT_CAMERA_MAX_ANGLE && fabsf(cam.pitch) <= RT_CAMERA_MAX_ANGLE &&
        fabsf(cam.FOV) <= RT_CAMERA_MAX_ANGLE)
        return rt_device_camera(cam);
    RtDevCamera dc;
    for (int k = 0; k < 9; ++k) dc.R[k] = NAN;
    dc.pos[0] = cam.position.x; dc.pos[1] = cam.position.y; dc.pos[2] = cam.position.z;
    dc.tan_half_fov = NAN;
    dc.aperture = cam.aperture_radius;
    return dc;
}

RT_HD RtM3 rt_camera_rotation(const RtDevCamera &cam)
{
    RtM3 m = {rt_v3(cam.R[0], cam.R[1], cam.R[2]), rt_v3(cam.R[3], cam.R[4], cam.R[5]),
              rt_v3(cam.R[6], cam.R[7], cam.R[8])};
    return m;
}

// camera_ray (rt_kernels.h; rt/path_tracing.cuh:381-391) with both jitter
// draws 0.5 and no aperture offset: the direction through the centre of pixel
// (x, y).  Draws nothing from the pixel's RNG.
RT_HD Vec3D rt_camera_centre_dir(const RtDevCamera &cam, int half_w, int half_h, int x, int y)
{
    const Vec3D dir = rt_normalize(rt_v3(cam.tan_half_fov * ((float)x + 0.5f - (float)half_w) / (float)half_w,
                                         cam.tan_half_fov * ((float)y + 0.5f - (float)half_h) / (float)half_w, 1.0f));
    return rt_camera_rotation(cam) * dir;
}
