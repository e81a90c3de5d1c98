// Range pixel -> point of the LiDAR frame, shared by projection.hip (section 11 of include/nvsf_hip.h) and object_masks.hip (section 12).
#pragma once
#include "common.h"
#include <math.h>

// convert.pano_to_lidar (nvsf/lib/convert.py:221-291) for pixel `pix` (row-major) of an Hl x Wl range image whose range is r: numpy on
// fp32 arrays, every operation rounded to fp32 by itself, true divisions.
//   beta = -(i - Wl / 2) / Wl * fov_hoz / 180 * pi, alpha = (fov_up - j / Hl * fov) / 180 * pi, point = (ca cb, ca sb, sa) * r
__device__ __forceinline__ void pano_point(uint32_t pix, uint32_t Hl, uint32_t Wl, float fov_up, float fov, float fov_hoz, float r, float& x,
                                           float& y, float& z) {
    const float i = (float)(pix % Wl), j = (float)(pix / Wl);
    const float kPi = 3.14159265358979323846f;
    const float beta = (-(i - (float)Wl / 2.0f)) / (float)Wl * fov_hoz / 180.0f * kPi;
    const float alpha = (fov_up - j / (float)Hl * fov) / 180.0f * kPi;
    const float ca = cosf(alpha), sa = sinf(alpha), cb = cosf(beta), sb = sinf(beta);
    x = (ca * cb) * r;
    y = (ca * sb) * r;
    z = sa * r;
}
