// LiDAR-projected camera depth maps for gfx950 (include/nvsf_hip.h section 11).
//
// The reference gives every frame a pseudo ground-truth camera depth image (nvsf/nerf/dataset/base_dataset.py:153-157): the range
// image becomes a point cloud (convert.pano_to_lidar, nvsf/lib/convert.py:221-291), the cloud is taken into the camera and through the
// pinhole (dataset_utils.lidar2points2d, :17-32), and a z-buffer keeps the nearest point of every pixel
// (dataset_utils.get_lidar_depth_image, :69-96 -- a Python loop over the points).  Here one thread = one range pixel (or one point of a
// raw cloud) and the whole split goes through in one call.
//
// Arithmetic, in the reference's dtypes:
//   fp32  beta = -(i - W/2) / W * fov_hoz / 180 * pi, alpha = (fov_up - j / H * fov) / 180 * pi   (numpy on fp32 arrays: every
//         operation rounded to fp32, true divisions), dir = (cos a cos b, cos a sin b, sin a), point = dir * range
//   fp64  c = [x, y, z, 1] @ lidar2cam^T (the fp32 matrix widened), q = c @ K^T, z = clip(q2, 1e-5, 99999), u = q0 / z, v = q1 / z,
//         inside iff 0 <= u < W and 0 <= v < H (a NaN is never inside), pixel (int(v), int(u)), value z rounded to fp32.
// Rounding to fp32 is monotonic, so the nearest point of a pixel is the smallest BIT PATTERN of the positive fp32 depths that land in
// it: an integer minimum, whose result does not depend on the order the points arrive in.  Two runs give the same bits.  0 has to mean
// "empty" in the finished image, so the minimum is taken by a compare-and-swap that treats 0 as the identity: a memset and one
// kernel, no pass that rewrites a sentinel afterwards.  At ~1 % occupied pixels the swap almost never repeats.
#include "common.h"
#include "pano_device.h"
#include <math.h>

namespace {
constexpr int kBlock = 256;

struct Pinhole { double k[9]; };    // K, row-major
struct Extrinsic { double m[12]; };  // rows 0..2 of lidar2cam, widened from fp32

// steps 2-3 of the header's description for one point
__device__ __forceinline__ void splat(float x, float y, float z, const double* __restrict__ m, const double* __restrict__ k, uint32_t H,
                                      uint32_t W, uint32_t* __restrict__ out) {
    const double px = (double)x, py = (double)y, pz = (double)z;
    double c[3], q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) c[r] = ((px * m[4 * r] + py * m[4 * r + 1]) + pz * m[4 * r + 2]) + m[4 * r + 3];
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = (c[0] * k[3 * r] + c[1] * k[3 * r + 1]) + c[2] * k[3 * r + 2];
    double d = q[2];
    d = d < 1e-5 ? 1e-5 : d;  // np.clip: NaN fails both tests and passes through
    d = d > 99999.0 ? 99999.0 : d;
    const double u = q[0] / d, v = q[1] / d;
    if (!(u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H)) return;
    const uint32_t bits = __float_as_uint((float)d);  // d in [1e-5, 99999]: a positive, finite, non-zero fp32
    uint32_t* cell = out + (size_t)(uint32_t)v * W + (uint32_t)u;
    uint32_t old = __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // other threads swap this word meanwhile
    while (old == 0u || old > bits) {
        const uint32_t seen = atomicCAS(cell, old, bits);
        if (seen == old) break;
        old = seen;
    }
}

__global__ __launch_bounds__(kBlock) void k_lidar_depth_images(const float* __restrict__ range_m, uint32_t Hl, uint32_t Wl, uint32_t per_frame,
                                                               uint32_t total, float fov_up, float fov, float fov_hoz,
                                                               const float* __restrict__ lidar2cam, Pinhole cam, uint32_t H, uint32_t W,
                                                               uint32_t* __restrict__ out) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= total) return;
    const float r = range_m[n];
    if (r == 0.0f) return;  // np.where(pano != 0.0): a NaN range goes on and lands nowhere
    const uint32_t f = n / per_frame, pix = n - f * per_frame;
    double m[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) m[e] = (double)lidar2cam[16 * (size_t)f + e];
    float x, y, z;
    pano_point(pix, Hl, Wl, fov_up, fov, fov_hoz, r, x, y, z);  // step 1 (pano_device.h)
    splat(x, y, z, m, cam.k, H, W, out + (size_t)f * H * W);
}

__global__ __launch_bounds__(kBlock) void k_points_depth_image(const float* __restrict__ points, uint32_t P, Extrinsic ext, Pinhole cam, uint32_t H, uint32_t W,
                                                               uint32_t* __restrict__ out) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= P) return;
    splat(points[3 * (size_t)n], points[3 * (size_t)n + 1], points[3 * (size_t)n + 2], ext.m, cam.k, H, W, out);
}

constexpr uint64_t kMaxImage = 1ull << 31;  // elements of the output and of the input: 32-bit thread indices
}  // namespace

NVSF_API int nvsf_lidar_depth_images(const float* range_m, uint32_t F, uint32_t Hl, uint32_t Wl, float fov_up, float fov, float fov_hoz,
                                     const float* lidar2cam, const double* K, uint32_t H, uint32_t W, float* out, hipStream_t stream) {
    REQUIRE(range_m && lidar2cam && K && out && F >= 1 && Hl >= 1 && Wl >= 1 && H >= 1 && W >= 1);
    REQUIRE(fov > 0.0f && fov_hoz > 0.0f && fov_up == fov_up && fov < INFINITY && fov_hoz < INFINITY);
    REQUIRE((uint64_t)F * Hl * Wl < kMaxImage && (uint64_t)F * H * W < kMaxImage);
    Pinhole cam;
    for (int e = 0; e < 9; ++e) cam.k[e] = K[e];
    if (hipMemsetAsync(out, 0, (size_t)F * H * W * sizeof(float), stream) != hipSuccess) return (int)hipGetLastError();
    const uint32_t per_frame = Hl * Wl, total = F * per_frame;
    hipLaunchKernelGGL(k_lidar_depth_images, dim3(cdiv(total, kBlock)), dim3(kBlock), 0, stream, range_m, Hl, Wl, per_frame, total, fov_up, fov,
                       fov_hoz, lidar2cam, cam, H, W, reinterpret_cast<uint32_t*>(out));
    return nvsf_launch_status();
}

NVSF_API int nvsf_points_depth_image(const float* points, uint32_t P, const float* lidar2cam, const double* K, uint32_t H, uint32_t W,
                                     float* out, hipStream_t stream) {
    REQUIRE(lidar2cam && K && out && H >= 1 && W >= 1 && (uint64_t)H * W < kMaxImage && (P == 0 || points) && P < kMaxImage);
    Pinhole cam;
    Extrinsic ext;
    for (int e = 0; e < 12; ++e) ext.m[e] = (double)lidar2cam[e];
    for (int e = 0; e < 9; ++e) cam.k[e] = K[e];
    if (hipMemsetAsync(out, 0, (size_t)H * W * sizeof(float), stream) != hipSuccess) return (int)hipGetLastError();
    if (P == 0) return NVSF_OK;
    hipLaunchKernelGGL(k_points_depth_image, dim3(cdiv(P, kBlock)), dim3(kBlock), 0, stream, points, P, ext, cam, H, W, reinterpret_cast<uint32_t*>(out));
    return nvsf_launch_status();
}
