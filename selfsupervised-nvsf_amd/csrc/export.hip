// Prediction export, gfx950 (section 14 of include/nvsf_hip.h): a rendered range image -> the point cloud of the sweep in the LiDAR
// frame and in the world frame, and float planes -> the uint8 planes the image files hold.  Reference: Trainer.test / test_step
// (nvsf/nerf/trainer.py:817-903, 1109-1283) with utils.get_pcd_bound_to_world (nvsf/nerf/utils.py:444-474) over
// convert.pano_to_lidar_with_intensities (nvsf/lib/convert.py:221-268).
//
// The cloud is an ORDERED stream compaction: point k is the k-th pixel, row-major, whose range is not 0 -- numpy's
// `cloud[np.where(pano != 0.0)]`.  Three launches and no waiting between workgroups (no look-back, no flags, no atomics):
//   k_count  a workgroup owns kPixels consecutive pixels, as kChunks chunks of kBlock; a wave's ballot + popcount counts the kept ones;
//            one count per workgroup goes to the workspace.
//   k_scan   ONE workgroup turns the counts into exclusive prefixes in place, kBlock at a time with a running carry, and writes the total.
//   k_place  the same ballots again; rank = workgroup prefix + kept pixels of the earlier (chunk, wave) pairs + kept lanes below.
// The placement recomputes the ballots instead of storing them: the range image is read twice (272 KiB at 66 x 1030), which costs less
// than a third array.  Two runs give the same bits.
#include "pano_device.h"

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kChunks = 4;
constexpr uint32_t kPixels = kBlock * kChunks;   // pixels per workgroup; nvsf/nerf/export.py: PIXELS_PER_WORKGROUP
constexpr uint32_t kMaxPixels = 1u << 24;

struct Affine { double m[12]; };  // rows 0..2 of lidar2world

__device__ __forceinline__ bool kept(const float* __restrict__ range, uint32_t pix, uint32_t n) {
    return pix < n && range[pix] != 0.0f;  // -0.0 is dropped, NaN and negative ranges are kept: np.where(pano != 0.0)
}

__global__ __launch_bounds__(kBlock) void k_count(const float* __restrict__ range, uint32_t n, uint32_t* __restrict__ counts) {
    __shared__ uint32_t per_wave[kWaves];
    const uint32_t base = blockIdx.x * kPixels;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < kChunks; ++k) c += (uint32_t)__popcll(__ballot(kept(range, base + k * kBlock + threadIdx.x, n)));
    if (lane_id() == 0) per_wave[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += per_wave[w];
        counts[blockIdx.x] = s;
    }
}

// counts [G] -> exclusive prefixes in place; total[0] = their sum.  One workgroup: G <= 2^24 / kPixels = 16384, 64 rounds at most.
__global__ __launch_bounds__(kBlock) void k_scan(uint32_t* __restrict__ counts, uint32_t G, uint32_t* __restrict__ total) {
    __shared__ uint32_t wave_sum_lds[kWaves];
    const int wave = (int)(threadIdx.x >> 6);
    uint32_t carry = 0;
    for (uint32_t g0 = 0; g0 < G; g0 += kBlock) {  // workgroup-uniform trip count
        const uint32_t g = g0 + threadIdx.x;
        const uint32_t v = g < G ? counts[g] : 0u;
        const uint32_t incl = wave_scan_add_u32(v);
        __syncthreads();  // the previous round's reads of wave_sum_lds are done
        if (lane_id() == kWave - 1) wave_sum_lds[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint32_t s = wave_sum_lds[w];
            before += w < wave ? s : 0u;
            all += s;
        }
        if (g < G) counts[g] = carry + before + incl - v;
        carry += all;
    }
    if (threadIdx.x == 0) total[0] = carry;
}

template <bool kWorld>
__global__ __launch_bounds__(kBlock) void k_place(const float* __restrict__ range, const float* __restrict__ payload, uint32_t n, uint32_t H,
                                                  uint32_t W, float fov_up, float fov, float fov_hoz, float scale, Affine T,
                                                  const uint32_t* __restrict__ prefix, float4* __restrict__ cloud_lidar,
                                                  double* __restrict__ cloud_world, uint32_t capacity) {
    __shared__ uint32_t per_pair[kChunks * kWaves];  // kept pixels of (chunk, wave), in pixel order
    const uint32_t base = blockIdx.x * kPixels;
    const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
    unsigned long long mask[kChunks];
#pragma unroll
    for (int k = 0; k < kChunks; ++k) {
        mask[k] = __ballot(kept(range, base + k * kBlock + threadIdx.x, n));
        if (lane == 0) per_pair[k * kWaves + wave] = (uint32_t)__popcll(mask[k]);
    }
    __syncthreads();
    const uint32_t first = prefix[blockIdx.x];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < kChunks; ++k) {
        if (!((mask[k] >> lane) & 1ull)) continue;
        uint32_t rank = first + (uint32_t)__popcll(mask[k] & below);
        for (int e = 0; e < k * kWaves + wave; ++e) rank += per_pair[e];
        if (rank >= capacity) continue;  // the total still counts the point; its row is not written
        const uint32_t pix = base + k * kBlock + threadIdx.x;
        float x, y, z;
        pano_point(pix, H, W, fov_up, fov, fov_hoz, range[pix], x, y, z);
        x = x / scale; y = y / scale; z = z / scale;  // true fp32 divisions (utils.py:463), not a product by the reciprocal
        const float p = payload ? payload[pix] : 0.0f;
        cloud_lidar[rank] = make_float4(x, y, z, p);
        if (kWorld) {  // float64 affine of the fp32 point, left to right (utils.py:470-472: np.ones promotes the cloud to float64)
            const double xd = x, yd = y, zd = z;
            double* o = cloud_world + (size_t)rank * 4;
            o[0] = ((T.m[0] * xd + T.m[1] * yd) + T.m[2] * zd) + T.m[3];
            o[1] = ((T.m[4] * xd + T.m[5] * yd) + T.m[6] * zd) + T.m[7];
            o[2] = ((T.m[8] * xd + T.m[9] * yd) + T.m[10] * zd) + T.m[11];
            o[3] = (double)p;
        }
    }
}

// utils.linear_to_srgb (utils.py:31-36) on an fp32 tensor: where(x < 0.0031308, 12.92 x, 1.055 x^0.41666 - 0.055), the scalars rounded
// to fp32 and every operation rounded to fp32.  The power is formed in fp64 and rounded once, so it is the correctly rounded fp32 power
// (the reference's vectorised powf is within 1 ulp of it).  NaN passes through; a negative x takes the linear branch.
__device__ __forceinline__ float linear_to_srgb(float x) {
    if (x < 0.0031308f) return 12.92f * x;
    const float pw = (float)pow((double)x, (double)0.41666f);
    return 1.055f * pw - 0.055f;
}

// (uint8)(x * 255.0f): fp32 product, truncation toward zero.  Outside numpy's defined range: NaN -> 0, product <= -1 -> 0, >= 256 -> 255.
__device__ __forceinline__ uint8_t quantize(float x) {
    const float p = x * 255.0f;
    if (!(p > 0.0f)) return 0;  // NaN, zero, negative ((-1, 0) truncates to 0 anyway)
    return p >= 255.0f ? (uint8_t)255 : (uint8_t)(int)p;
}

__global__ __launch_bounds__(kBlock) void k_quantize(const float* __restrict__ x, uint32_t n, int srgb, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    out[i] = quantize(srgb ? linear_to_srgb(v) : v);
}

__global__ __launch_bounds__(kBlock) void k_linear_to_srgb(const float* __restrict__ x, uint32_t n, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = linear_to_srgb(x[i]);
}
}  // namespace

NVSF_API int nvsf_pano_to_cloud_sizes(uint32_t H, uint32_t W, uint64_t* sizes, hipStream_t) {
    REQUIRE(sizes && H >= 1 && W >= 1 && (uint64_t)H * W <= kMaxPixels);
    sizes[0] = (uint64_t)cdiv(H * W, kPixels) * sizeof(uint32_t);
    sizes[1] = kPixels;
    return NVSF_OK;
}

NVSF_API int nvsf_pano_to_cloud(const float* range, const float* payload, uint32_t H, uint32_t W, const double* geom, const double* lidar2world,
                                void* workspace, size_t ws_bytes, float* cloud_lidar, double* cloud_world, uint32_t capacity, uint32_t* count,
                                hipStream_t stream) {
    REQUIRE(H >= 1 && W >= 1 && (uint64_t)H * W <= kMaxPixels);
    REQUIRE(range && geom && workspace && count && (cloud_lidar || capacity == 0));
    REQUIRE(!cloud_world || lidar2world);
    REQUIRE(geom[1] > 0.0 && geom[2] > 0.0 && geom[3] > 0.0);
    const uint32_t n = H * W, G = cdiv(n, kPixels);
    REQUIRE(ws_bytes >= (size_t)G * sizeof(uint32_t));
    REQUIRE(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)cloud_lidar & 15) == 0 && ((uintptr_t)cloud_world & 7) == 0);
    uint32_t* counts = (uint32_t*)workspace;
    Affine T = {};
    if (cloud_world)
        for (int e = 0; e < 12; ++e) T.m[e] = lidar2world[e];
    hipLaunchKernelGGL(k_count, dim3(G), dim3(kBlock), 0, stream, range, n, counts);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(kBlock), 0, stream, counts, G, count);
    if (capacity > 0) {
        const float fov_up = (float)geom[0], fov = (float)geom[1], fov_hoz = (float)geom[2], scale = (float)geom[3];
        if (cloud_world)
            hipLaunchKernelGGL(k_place<true>, dim3(G), dim3(kBlock), 0, stream, range, payload, n, H, W, fov_up, fov, fov_hoz, scale, T, counts,
                               (float4*)cloud_lidar, cloud_world, capacity);
        else
            hipLaunchKernelGGL(k_place<false>, dim3(G), dim3(kBlock), 0, stream, range, payload, n, H, W, fov_up, fov, fov_hoz, scale, T, counts,
                               (float4*)cloud_lidar, cloud_world, capacity);
    }
    return nvsf_launch_status();
}

NVSF_API int nvsf_quantize_u8(const float* x, uint32_t n, int srgb, uint8_t* out, hipStream_t stream) {
    REQUIRE(n <= (1u << 30));
    if (n == 0) return NVSF_OK;
    REQUIRE(x && out);
    hipLaunchKernelGGL(k_quantize, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, stream, x, n, srgb, out);
    return nvsf_launch_status();
}

NVSF_API int nvsf_linear_to_srgb(const float* x, uint32_t n, float* out, hipStream_t stream) {
    REQUIRE(n <= (1u << 30));
    if (n == 0) return NVSF_OK;
    REQUIRE(x && out);
    hipLaunchKernelGGL(k_linear_to_srgb, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, stream, x, n, out);
    return nvsf_launch_status();
}
