// LiDAR cloud cleaning for the scene-flow loss, gfx950: the k-nearest-neighbour statistic of the statistical outlier filter and the
// inlier tests of the RANSAC ground fit.  Reference: point_removal, nvsf/nerf/utils.py:151-268 (Open3D's
// remove_statistical_outlier + my_ransac), called once per frame by Trainer.process_pointcloud, trainer.py:1848-1912.
//
// k_knn_mean (the hot path: N^2 distance evaluations, N ~ 55 k): a workgroup of 4 waves streams the whole cloud through a 1024-point
// LDS tile, as k_chamfer_scan does; every wave owns kQ = 4 queries and keeps, per query, the 64 smallest squared distances seen so
// far ONE PER LANE, ascending (k <= 64 = the wave size).  An iteration gives every lane one candidate, read from LDS once and tested
// against the kQ queries; __ballot collects the lanes whose candidate beats the query's current k-th distance and only those are
// inserted, one by one: the list shifts one lane up past the insertion point (a DPP wave shift, no LDS traffic).  After the first
// tiles an insertion is rare (about k ln(N / k) per query in all), so the loop is the distance evaluation.  Squared distances are
// formed from coordinate differences; ties with the k-th distance are not inserted, which leaves the multiset of the k smallest --
// and so the mean -- unchanged.  The mean is a fixed butterfly over the lanes: two runs give the same bits.
#include "common.h"
#include <math.h>

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kQ = 4;             // queries per wave
constexpr int kTile = 1024;       // points per LDS tile (12 KiB)
constexpr int kMaxPlanes = 256;   // plane hypotheses per LDS chunk of k_plane_count

// lane l <- v of lane l - 1, lane 0 <- first (DPP wave_shr:1)
__device__ __forceinline__ float wave_shift_up(float v, float first) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(first), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float read_lane(float v, int lane) {  // lane: wave-uniform
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

__global__ __launch_bounds__(kBlock) void k_knn_mean(const float* __restrict__ pts, uint32_t n, uint32_t kk, float* __restrict__ out) {
    __shared__ float tile[kTile * 3];
    const int lane = lane_id();
    const uint32_t q0 = (blockIdx.x * kWaves + (threadIdx.x >> 6)) * kQ;  // wave-uniform
    float qx[kQ], qy[kQ], qz[kQ], best[kQ], kth[kQ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
        const uint32_t qi = min(q0 + q, n - 1);  // a query past the end repeats the last point and is not written
        qx[q] = pts[(size_t)qi * 3]; qy[q] = pts[(size_t)qi * 3 + 1]; qz[q] = pts[(size_t)qi * 3 + 2];
        best[q] = INFINITY; kth[q] = INFINITY;
    }
    // Tiles are visited outwards from the workgroup's own: a sensor writes its cloud ring by ring, so neighbours in memory are neighbours
    // in space, the k-th distance is near its final value after the first tile and the later ones insert next to nothing.  (Visited
    // in index order, every ring on the way to the query kept beating the bar: 3.2 ms instead of the figure in DESIGN.md 9c.)
    const uint32_t tiles = (n + kTile - 1) / kTile, own = min(blockIdx.x * (kWaves * kQ) / kTile, tiles - 1);
    for (uint32_t step = 0; step < 2 * tiles; ++step) {
        const uint32_t off = (step + 1) / 2;
        if ((step & 1) ? own + off >= tiles : off > own) continue;  // workgroup-uniform: that side has run out of tiles
        const uint32_t t0 = ((step & 1) ? own + off : own - off) * kTile;
        const uint32_t cnt = min((uint32_t)kTile, n - t0);
        __syncthreads();
        const uint32_t padded = (cnt + kWave - 1) / kWave * kWave;  // <= kTile; the last rows lie at infinity: never a neighbour
        for (uint32_t e = threadIdx.x; e < padded * 3; e += kBlock) tile[e] = e < cnt * 3 ? pts[(size_t)t0 * 3 + e] : INFINITY;
        __syncthreads();
        for (uint32_t j0 = 0; j0 < cnt; j0 += kWave) {
            const uint32_t j = j0 + lane;
            const float tx = tile[3 * j], ty = tile[3 * j + 1], tz = tile[3 * j + 2];
#pragma unroll
            for (int q = 0; q < kQ; ++q) {
                const float dx = tx - qx[q], dy = ty - qy[q], dz = tz - qz[q];
                const float d = dx * dx + dy * dy + dz * dz;
                unsigned long long m = __ballot(d < kth[q]);
                while (m) {  // wave-uniform: insert the candidates that beat the k-th distance, lowest lane first
                    const int src = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const float dc = read_lane(d, src);
                    if (dc < kth[q]) {  // an earlier insertion of this round may have lowered the bar
                        const float below = wave_shift_up(best[q], dc);
                        best[q] = best[q] > dc ? fmaxf(below, dc) : best[q];
                        kth[q] = read_lane(best[q], (int)kk - 1);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
        float s = (uint32_t)lane < kk ? sqrtf(best[q]) : 0.0f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0 && q0 + q < n) out[q0 + q] = s / (float)kk;
    }
}

// Signed plane distance in fp64: 3 N K multiply-adds are nothing next to the neighbour search, and the inlier sets then do not depend
// on fp32 rounding of terms two orders of magnitude above the threshold.
__device__ __forceinline__ bool near_plane(double x, double y, double z, const float* p, double thr) {
    return fabs((double)p[0] * x + (double)p[1] * y + (double)p[2] * z + (double)p[3]) < thr;
}

// one point per lane, hypotheses from LDS (wave-uniform reads); per hypothesis one __ballot + popcount per wave into an LDS counter,
// then one global integer atomic per (workgroup, hypothesis): the counts do not depend on the order of anything.
__global__ __launch_bounds__(kBlock) void k_plane_count(const float* __restrict__ pts, uint32_t n, const float* __restrict__ planes,
                                                        uint32_t K, float threshold, int* __restrict__ counts) {
    __shared__ float pl[kMaxPlanes * 4];
    __shared__ int cnt[kMaxPlanes];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    const uint32_t ii = live ? i : 0;
    const double x = pts[(size_t)ii * 3], y = pts[(size_t)ii * 3 + 1], z = pts[(size_t)ii * 3 + 2];
    const double thr = (double)threshold;
    for (uint32_t k0 = 0; k0 < K; k0 += kMaxPlanes) {
        const uint32_t kc = min((uint32_t)kMaxPlanes, K - k0);
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < kc * 4; e += kBlock) pl[e] = planes[(size_t)k0 * 4 + e];
        for (uint32_t e = threadIdx.x; e < kc; e += kBlock) cnt[e] = 0;
        __syncthreads();
        for (uint32_t k = 0; k < kc; ++k) {
            const unsigned long long m = __ballot(live && near_plane(x, y, z, pl + 4 * k, thr));
            if (lane_id() == 0 && m) atomicAdd(&cnt[k], __popcll(m));
        }
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < kc; e += kBlock)
            if (cnt[e]) atomicAdd(counts + k0 + e, cnt[e]);
    }
}

__global__ __launch_bounds__(kBlock) void k_plane_mask(const float* __restrict__ pts, uint32_t n, const float* __restrict__ planes,
                                                       uint32_t R, float threshold, float z_max, uint8_t* __restrict__ mask) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float zf = pts[(size_t)i * 3 + 2];
    const double x = pts[(size_t)i * 3], y = pts[(size_t)i * 3 + 1], z = zf;
    bool hit = false;
    for (uint32_t r = 0; r < R; ++r) hit = hit || near_plane(x, y, z, planes + 4 * (size_t)r, (double)threshold);
    mask[i] = (hit && zf < z_max) ? 1 : 0;
}
}  // namespace

constexpr uint32_t kMaxPoints = 1u << 28;  // 3 n and the grid sizes stay far inside 32 bits

NVSF_API int nvsf_knn_mean_distance(const float* points, uint32_t n, uint32_t k, float* out_mean, hipStream_t stream) {
    REQUIRE(k >= 1 && k <= (uint32_t)kWave && n <= kMaxPoints);
    if (n == 0) return NVSF_OK;
    REQUIRE(points && out_mean);
    hipLaunchKernelGGL(k_knn_mean, dim3(cdiv(n, kWaves * kQ)), dim3(kBlock), 0, stream, points, n, k < n ? k : n, out_mean);
    return nvsf_launch_status();
}

NVSF_API int nvsf_plane_inlier_count(const float* points, uint32_t n, const float* planes, uint32_t K, float threshold, int32_t* counts,
                                     hipStream_t stream) {
    REQUIRE(n <= kMaxPoints && K <= (1u << 20) && threshold >= 0.0f);
    if (n == 0 || K == 0) return NVSF_OK;
    REQUIRE(points && planes && counts);
    hipLaunchKernelGGL(k_plane_count, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, stream, points, n, planes, K, threshold, counts);
    return nvsf_launch_status();
}

NVSF_API int nvsf_plane_inlier_mask(const float* points, uint32_t n, const float* planes, uint32_t R, float threshold, float z_max,
                                    uint8_t* mask, hipStream_t stream) {
    REQUIRE(n <= kMaxPoints && R <= (1u << 20) && threshold >= 0.0f);
    if (n == 0) return NVSF_OK;
    REQUIRE(points && mask && (planes || R == 0));
    hipLaunchKernelGGL(k_plane_mask, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, stream, points, n, planes, R, threshold, z_max, mask);
    return nvsf_launch_status();
}
