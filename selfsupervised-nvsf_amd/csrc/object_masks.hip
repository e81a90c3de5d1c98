// Static / dynamic object masks and the range-image z-buffer for gfx950 (include/nvsf_hip.h section 12).
//
// The reference splits its evaluation table by the annotated moving objects (trainer.py:1545-1626).  utils.compute_object_masks
// (nvsf/nerf/utils.py:750-807) turns a range image into a cloud, asks scipy's Delaunay triangulation of every annotated box which
// points it holds (lib/tools.py:138-160) and projects the cloud back into a range image with that bit as payload
// (lib/convert.py::lidar_to_pano_with_intensities, :105-181 -- a Python loop over the points, also the routine that makes the range
// images of the data set, preprocess/generate_rangeview.py:185-258); utils.compute_object_masks_img (:810-873) fills the projected
// boxes of the camera image with a double Python loop.  Here: one thread per point / range pixel / camera pixel.
//
// Membership: a convex hull is the intersection of its supporting half-spaces, n.p + d <= 0 in fp64, planes staged in LDS once per
// workgroup.  Z-buffer: a 64-bit integer atomicMin on (bits(dist) << 32) | index into a workspace filled with ones, then a resolve
// pass.  A positive fp32 orders as its bits do and among equal dists the lowest index wins -- the reference's strict `>` in arrival
// order -- so the image does not depend on scheduling and two runs give the same bits.
#include "common.h"
#include "pano_device.h"
#include <math.h>

namespace {
constexpr int kBlock = 256;
constexpr uint32_t kMaxPlanes = 768;    // B * KMAX of one launch: 768 planes x 32 B = 24 KiB of LDS (64 boxes of 12 planes)
constexpr uint32_t kBoxChunk = 1024;    // image boxes staged per pass: 16 KiB of LDS
constexpr uint64_t kMaxImage = 1ull << 31;
constexpr uint64_t kEmpty = ~0ull;

// What lidar_to_pano_with_intensities computes from its Python floats before the loop, each formed in double and rounded to fp32 once
// (numpy 2: a Python float beside an fp32 value is cast to fp32).
struct PanoGeom {
    float az0;        // fov_hoz_up * pi / 180
    float step_h;     // (fov_hoz * pi / 180) / W
    float el0;        // (fov - fov_up) / 180 * pi
    float step_v;     // fov / 180 * pi / H
    float max_depth;
    float Hf, Wf;
    uint32_t W;
};

__device__ __forceinline__ void stage_planes(const double* __restrict__ planes, const uint32_t* __restrict__ counts, uint32_t B, uint32_t KMAX,
                                             double* s_planes, uint32_t* s_counts) {
    for (uint32_t e = threadIdx.x; e < B * KMAX * 4; e += kBlock) s_planes[e] = planes[e];
    for (uint32_t b = threadIdx.x; b < B; b += kBlock) s_counts[b] = min(counts[b], KMAX);
    __syncthreads();
}

// 1 iff some box holds the point: every one of its half-spaces has n.p + d <= 0, the sum left to right in fp64.  A box without planes
// holds nothing; a NaN coordinate is in no box.
__device__ __forceinline__ uint32_t in_hulls(float x, float y, float z, const double* s_planes, const uint32_t* s_counts, uint32_t B,
                                             uint32_t KMAX) {
    const double px = (double)x, py = (double)y, pz = (double)z;
    for (uint32_t b = 0; b < B; ++b) {
        const uint32_t K = s_counts[b];
        const double* q = s_planes + (size_t)b * KMAX * 4;
        uint32_t k = 0;
        for (; k < K; ++k, q += 4)
            if (!(((px * q[0] + py * q[1]) + pz * q[2]) + q[3] <= 0.0)) break;
        if (k == K && K > 0) return 1u;
    }
    return 0u;
}

// convert.py:128-176 for one point; `tag` is the low word of the z-buffer key (the point's index, or twice the index plus a payload bit)
__device__ __forceinline__ void zbuffer_enter(float x, float y, float z, uint32_t tag, const PanoGeom& g, unsigned long long* __restrict__ ws) {
    const float xx = __fmul_rn(x, x), yy = __fmul_rn(y, y);
    const float dist = sqrtf(__fadd_rn(__fadd_rn(xx, yy), __fmul_rn(z, z)));  // np.linalg.norm of an fp32 row
    if (!(dist < g.max_depth) || dist == 0.0f) return;                       // `dist >= max_depth`; NaN and 0: header
    const float beta = g.az0 - atan2f(y, x);
    const float alpha = atan2f(z, sqrtf(__fadd_rn(xx, yy))) + g.el0;
    const float c = rintf(beta / g.step_h), r = rintf(g.Hf - alpha / g.step_v);  // Python's round: half to even
    if (!(r >= 0.0f && r < g.Hf && c >= 0.0f && c < g.Wf)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(dist) << 32) | tag;
    atomicMin(ws + (size_t)(uint32_t)r * g.W + (uint32_t)c, key);
}

__global__ __launch_bounds__(kBlock) void k_points_in_hulls(const float* __restrict__ points, uint32_t P, const double* __restrict__ planes,
                                                            const uint32_t* __restrict__ counts, uint32_t B, uint32_t KMAX,
                                                            uint8_t* __restrict__ mask) {
    __shared__ double s_planes[kMaxPlanes * 4];
    __shared__ uint32_t s_counts[kMaxPlanes];
    stage_planes(planes, counts, B, KMAX, s_planes, s_counts);
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= P) return;
    mask[n] = (uint8_t)in_hulls(points[3 * (size_t)n], points[3 * (size_t)n + 1], points[3 * (size_t)n + 2], s_planes, s_counts, B, KMAX);
}

__global__ __launch_bounds__(kBlock) void k_points_to_pano(const float* __restrict__ points, uint32_t P, PanoGeom g,
                                                           unsigned long long* __restrict__ ws) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= P) return;
    zbuffer_enter(points[3 * (size_t)n], points[3 * (size_t)n + 1], points[3 * (size_t)n + 2], n, g, ws);
}

// the whole of compute_object_masks for one range pixel: point (section 11 step 1), membership, back into the z-buffer
__global__ __launch_bounds__(kBlock) void k_range_pixels_to_pano(const float* __restrict__ range_m, uint32_t H, uint32_t W, float fov_up, float fov,
                                                                 float fov_hoz, PanoGeom g, const double* __restrict__ planes,
                                                                 const uint32_t* __restrict__ counts, uint32_t B, uint32_t KMAX,
                                                                 unsigned long long* __restrict__ ws) {
    __shared__ double s_planes[kMaxPlanes * 4];
    __shared__ uint32_t s_counts[kMaxPlanes];
    stage_planes(planes, counts, B, KMAX, s_planes, s_counts);
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= H * W) return;
    const float r = range_m[n];
    if (r == 0.0f) return;  // np.where(pano != 0.0)
    float x, y, z;
    pano_point(n, H, W, fov_up, fov, fov_hoz, r, x, y, z);
    // cloud order is pixel order, so 2 n + bit orders equal dists as the cloud index does
    zbuffer_enter(x, y, z, 2u * n + in_hulls(x, y, z, s_planes, s_counts, B, KMAX), g, ws);
}

// kMode 0: payload_img = payload[index]; 1: payload_img = the key's low bit
template <int kMode>
__global__ __launch_bounds__(kBlock) void k_resolve(const unsigned long long* __restrict__ ws, uint32_t n_pix, const float* __restrict__ payload,
                                                    float* __restrict__ pano, float* __restrict__ payload_img) {
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= n_pix) return;
    const unsigned long long key = ws[n];
    const bool hit = key != kEmpty;
    if (pano) pano[n] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
    if (payload_img) {
        const uint32_t tag = (uint32_t)key;
        payload_img[n] = !hit ? 0.0f : kMode == 0 ? payload[tag] : (float)(tag & 1u);
    }
}

__global__ __launch_bounds__(kBlock) void k_box_mask_image(const int32_t* __restrict__ boxes, uint32_t B, uint32_t W, uint32_t n_pix,
                                                           uint8_t* __restrict__ mask) {
    __shared__ int32_t s_box[kBoxChunk * 4];
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    const int32_t x = (int32_t)(n % W), y = (int32_t)(n / W);
    bool hit = false;
    for (uint32_t base = 0; base < B; base += kBoxChunk) {
        const uint32_t nb = min(B - base, kBoxChunk);
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < nb * 4; e += kBlock) s_box[e] = boxes[(size_t)base * 4 + e];
        __syncthreads();
        for (uint32_t b = 0; b < nb && !hit; ++b)  // an inverted box fails one of the two-sided tests for every pixel
            hit = x >= s_box[4 * b] && x <= s_box[4 * b + 2] && y >= s_box[4 * b + 1] && y <= s_box[4 * b + 3];
    }
    if (n < n_pix) mask[n] = hit ? 1 : 0;
}

// geom: HOST pointer to (fov_up, fov, fov_hoz_up, fov_hoz, max_depth) in double
bool pano_geom(const double* geom, uint32_t H, uint32_t W, PanoGeom* g) {
    const double fov_up = geom[0], fov = geom[1], fov_hoz_up = geom[2], fov_hoz = geom[3], max_depth = geom[4];
    if (!(fov > 0.0 && fov < INFINITY && fov_hoz > 0.0 && fov_hoz < INFINITY && fov_up == fov_up && fov_hoz_up == fov_hoz_up && max_depth > 0.0))
        return false;
    const double pi = 3.141592653589793;  // np.pi
    g->az0 = (float)(fov_hoz_up * pi / 180);
    g->step_h = (float)((fov_hoz * pi / 180) / W);
    g->el0 = (float)((fov - fov_up) / 180 * pi);
    g->step_v = (float)(fov / 180 * pi / H);
    g->max_depth = (float)max_depth;
    g->Hf = (float)H;
    g->Wf = (float)W;
    g->W = W;
    return g->step_h > 0.0f && g->step_v > 0.0f;
}

bool hulls_ok(const double* planes, const uint32_t* counts, uint32_t B, uint32_t KMAX) {
    return B == 0 || (planes && counts && KMAX >= 1 && (uint64_t)B * KMAX <= kMaxPlanes);
}
}  // namespace

NVSF_API int nvsf_points_in_hulls(const float* points, uint32_t P, const double* planes, const uint32_t* plane_counts, uint32_t B, uint32_t KMAX,
                                  uint8_t* mask, hipStream_t stream) {
    REQUIRE((P == 0 || (points && mask)) && P < kMaxImage && hulls_ok(planes, plane_counts, B, KMAX));
    if (P == 0) return NVSF_OK;
    if (B == 0) return hipMemsetAsync(mask, 0, P, stream) == hipSuccess ? NVSF_OK : (int)hipGetLastError();
    hipLaunchKernelGGL(k_points_in_hulls, dim3(cdiv(P, kBlock)), dim3(kBlock), 0, stream, points, P, planes, plane_counts, B, KMAX, mask);
    return nvsf_launch_status();
}

NVSF_API int nvsf_lidar_to_pano(const float* points, const float* payload, uint32_t P, uint32_t H, uint32_t W, const double* geom, void* workspace,
                                size_t ws_bytes, float* pano, float* payload_img, hipStream_t stream) {
    REQUIRE(geom && workspace && pano && H >= 1 && W >= 1 && (uint64_t)H * W < kMaxImage && (P == 0 || points));
    REQUIRE(!payload_img || payload || P == 0);
    REQUIRE(((uintptr_t)workspace & 7) == 0 && ws_bytes >= (size_t)H * W * sizeof(uint64_t));
    PanoGeom g;
    REQUIRE(pano_geom(geom, H, W, &g));
    const uint32_t n_pix = H * W;
    unsigned long long* ws = static_cast<unsigned long long*>(workspace);
    if (hipMemsetAsync(ws, 0xFF, (size_t)n_pix * sizeof(uint64_t), stream) != hipSuccess) return (int)hipGetLastError();
    if (P) hipLaunchKernelGGL(k_points_to_pano, dim3(cdiv(P, kBlock)), dim3(kBlock), 0, stream, points, P, g, ws);
    hipLaunchKernelGGL(k_resolve<0>, dim3(cdiv(n_pix, kBlock)), dim3(kBlock), 0, stream, ws, n_pix, payload, pano, payload_img);
    return nvsf_launch_status();
}

NVSF_API int nvsf_range_image_object_mask(const float* range_m, uint32_t H, uint32_t W, const double* geom, const double* planes,
                                          const uint32_t* plane_counts, uint32_t B, uint32_t KMAX, void* workspace, size_t ws_bytes,
                                          float* dyn_mask, hipStream_t stream) {
    REQUIRE(range_m && geom && workspace && dyn_mask && H >= 1 && W >= 1 && (uint64_t)H * W < (kMaxImage >> 1));
    REQUIRE(hulls_ok(planes, plane_counts, B, KMAX));
    REQUIRE(((uintptr_t)workspace & 7) == 0 && ws_bytes >= (size_t)H * W * sizeof(uint64_t));
    PanoGeom g;
    REQUIRE(pano_geom(geom, H, W, &g));
    const uint32_t n_pix = H * W;
    if (B == 0)  // no box: nothing is dynamic, whatever the z-buffer would keep
        return hipMemsetAsync(dyn_mask, 0, (size_t)n_pix * sizeof(float), stream) == hipSuccess ? NVSF_OK : (int)hipGetLastError();
    unsigned long long* ws = static_cast<unsigned long long*>(workspace);
    if (hipMemsetAsync(ws, 0xFF, (size_t)n_pix * sizeof(uint64_t), stream) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(k_range_pixels_to_pano, dim3(cdiv(n_pix, kBlock)), dim3(kBlock), 0, stream, range_m, H, W, (float)geom[0], (float)geom[1],
                       (float)geom[3], g, planes, plane_counts, B, KMAX, ws);
    hipLaunchKernelGGL(k_resolve<1>, dim3(cdiv(n_pix, kBlock)), dim3(kBlock), 0, stream, ws, n_pix, (const float*)nullptr, (float*)nullptr, dyn_mask);
    return nvsf_launch_status();
}

NVSF_API int nvsf_box_mask_image(const int32_t* boxes, uint32_t B, uint32_t H, uint32_t W, uint8_t* dyn_mask, hipStream_t stream) {
    REQUIRE(dyn_mask && H >= 1 && W >= 1 && (uint64_t)H * W < kMaxImage && (B == 0 || boxes) && B <= (1u << 20));
    const uint32_t n_pix = H * W;
    if (B == 0) return hipMemsetAsync(dyn_mask, 0, n_pix, stream) == hipSuccess ? NVSF_OK : (int)hipGetLastError();
    hipLaunchKernelGGL(k_box_mask_image, dim3(cdiv(n_pix, kBlock)), dim3(kBlock), 0, stream, boxes, B, W, n_pix, dyn_mask);
    return nvsf_launch_status();
}
