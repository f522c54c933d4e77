// lens.h -- the camera ray of a path: KIRK's pinhole ray (Camera::getRayFromPixel,
// Common/Camera.cpp:59-66) and, behind khp_set_lens, the thin-lens ray of
// Camera::transformToDof (Camera.cpp:39-51), which only KIRK's Whitted tracer calls.
// Plain float32 functions compiled by g++ (lens_host.cpp: khp_camera_rays_host) and by
// hipcc (render.hip: camera_path, the one place the kernels make camera rays), both with
// -ffp-contract=off: the same bits on host and device.  Every step is one float32
// operation in the order written.
#pragma once

#include <stdint.h>

#include "../../include/kirk_hip.h"
#include "kmath.h"

namespace khp {

// pi/4 and pi/2 rounded to float32 (0x3F490FDB, 0x3FC90FDB)
constexpr float LENS_PI_4 = 0.785398185253143310546875f;
constexpr float LENS_PI_2 = 1.57079637050628662109375f;

// Why khp_set_lens refuses *l, or null (the text khp_last_error gives).
inline const char* lens_error(const khp_lens* l) {
    if (!l) return "null argument";
    if (!(l->radius >= 0.0f) || l->radius == k_inf()) return "radius must be finite and >= 0";
    if (!(l->focus_distance > 0.0f) || l->focus_distance == k_inf()) return "focus_distance must be finite and > 0";
    if (l->focus != KHP_LENS_FOCUS_KIRK && l->focus != KHP_LENS_FOCUS_PLANE)
        return "focus must be KHP_LENS_FOCUS_KIRK or KHP_LENS_FOCUS_PLANE";
    if (l->reserved != 0u) return "reserved must be 0";
    return nullptr;
}

// The argument checks khp_camera_rays_host and khp_debug_camera_rays share (lens_host.cpp).
const char* camera_rays_error(const khp_lens* lens, uint32_t width, uint32_t n, const void* pixels,
                              const void* samples, const void* orig, const void* dir);

// Shirley and Chiu's concentric map of the unit square onto the unit disk (area
// preserving).  KIRK draws glm::diskRand(m_aperture * 3) by rejection from rand(); this
// is the same distribution, uniform over the disk, as a function of the path's key.
KHD void concentric_disk(float u, float v, float& x, float& y) {
    const float a = 2.0f * u - 1.0f, b = 2.0f * v - 1.0f;
    if (a == 0.0f && b == 0.0f) {
        x = 0.0f;
        y = 0.0f;
        return;
    }
    float r, phi;
    if (k_fabs(a) > k_fabs(b)) {
        r = a;
        const float q = b / a;
        phi = LENS_PI_4 * q;
    } else {
        r = b;
        const float q = a / b;
        const float t = LENS_PI_4 * q;
        phi = LENS_PI_2 - t;
    }
    x = r * k_cosf(phi);
    y = r * k_sinf(phi);
}

// The lens ray through the focus point of the pinhole ray (p, d), d normalised.
KHD void lens_ray(const khp_camera& cam, const khp_lens& lens, uint32_t key, v3 p, v3 d, v3& o, v3& dir) {
    const float u = draw_u01(key, dim_of(0, P_LENS_U)), v = draw_u01(key, dim_of(0, P_LENS_V));
    float dx, dy;
    concentric_disk(u, v, dx, dy);
    const float lx = lens.radius * dx, ly = lens.radius * dy;
    const v3 ax = ld3(cam.axis_x), ay = ld3(cam.axis_y);
    float ft = lens.focus_distance;
    if (lens.focus == KHP_LENS_FOCUS_PLANE) {
        const v3 fwd = normalize(cross(ay, ax));   // the camera normal (img_sensor's)
        const float c = dot(d, fwd);
        if (c > 0.0f) ft = lens.focus_distance / c;
    }
    const v3 f = p + d * ft;
    const v3 start = (p + ax * lx) + ay * ly;
    o = start;
    dir = normalize(f - start);   // the Ray constructor normalises (Common/Ray.cpp:11-15)
}

// The pinhole ray of the path with key `key` through pixel (x, y) (Camera::getRayFromPixel,
// Camera.cpp:59-66; the Ray constructor normalises).
KHD void pinhole_ray(const khp_camera& cam, uint32_t x, uint32_t y, uint32_t key, v3& o, v3& dir) {
    const float u1 = draw_u01(key, dim_of(0, P_CAM_X)), u2 = draw_u01(key, dim_of(0, P_CAM_Y));
    const float s1 = ((float)x + u1) * cam.pixel_size, s2 = ((float)y + u2) * cam.pixel_size;
    const v3 to = ((ld3(cam.bottom_left) + ld3(cam.axis_x) * s1) + ld3(cam.axis_y) * s2) - ld3(cam.position);
    o = ld3(cam.position);
    dir = normalize(to);
}

// The camera ray of that path: the pinhole ray with lens.radius == 0 (no lens draw), else
// the lens ray through its focus point.  The kernels choose between the two at compile
// time (camera_path<LENS>, instances picked by the plan); this is the same choice at run time.
KHD void camera_ray(const khp_camera& cam, const khp_lens& lens, uint32_t x, uint32_t y, uint32_t key, v3& o,
                    v3& dir) {
    pinhole_ray(cam, x, y, key, o, dir);
    if (lens.radius > 0.0f) lens_ray(cam, lens, key, o, dir, o, dir);
}

}  // namespace khp
