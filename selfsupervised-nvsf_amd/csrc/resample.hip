// Hierarchical importance resampling of the uniform ray render (include/nvsf_hip.h section 15): the inverse-CDF sampler of
// /root/reference/nvsf/nerf/models/renderer_dynamic.py:8-52, the per-ray merge of the coarse and the resampled depths, and the row
// merge / split that carries the field outputs (and their gradients) into the merged order.
//
// One 64-lane wave owns one ray, four rays per workgroup.  The ray's float64 cdf, its coarse depths and its new depths live in LDS
// (T = 1024, U = 256: 13 KB per wave).  The cdf is a cross-lane float64 scan carried from one 64-sample round to the next; every lane
// then inverts it for its own draws by binary search; the new depths are sorted by a bitonic network in LDS; the merge goes by rank
// (two binary searches per element, no serial walk of the row).  A wave shares its LDS slice with no other, so the phases are
// separated by wave-level barriers only: the four rays of a workgroup never wait for each other, and a wave past the last ray leaves
// at once.
#include "common.h"
#include <float.h>
#include <math.h>

namespace {
constexpr int kBlock = 256;
constexpr int kRaysPerBlock = kBlock / kWave;
constexpr uint32_t kMaxBins = 1024;   // nb of nvsf_sample_pdf; nvsf_resample_merge has nb = T - 1 and T <= 1024
constexpr uint32_t kMaxCoarse = 1024;
constexpr uint32_t kMaxFine = 256;
constexpr uint32_t kMaxDraws = 1u << 16;  // U of nvsf_sample_pdf (the draws are not staged)

// Orders this wave's LDS writes before its later LDS reads of other lanes' slots (no other wave touches the slice).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double wave_scan_add_f64(double v) {
    const int l = lane_id();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_up(v, o, 64);
        if (l >= o) v += u;
    }
    return v;
}

// cdf[0 .. nw] of the nw weights `weight_at(i)` (fp32, the 1e-5 already added): sum, pdf and running sum in float64, leading 0.
template <typename W>
__device__ __forceinline__ void build_cdf(W weight_at, uint32_t nw, double* cdf, int lane) {
    double part = 0.0;
    for (uint32_t i = lane; i < nw; i += 64) part += (double)weight_at(i);
    const double total = wave_sum(part);
    double carry = 0.0;
    if (lane == 0) cdf[0] = 0.0;
    for (uint32_t base = 0; base < nw; base += 64) {
        const uint32_t i = base + lane;
        const double p = i < nw ? (double)weight_at(i) / total : 0.0;
        const double incl = wave_scan_add_f64(p);
        if (i < nw) cdf[1 + i] = carry + incl;
        carry += __shfl(incl, 63, 64);
    }
}

// One draw through the inverse cdf (renderer_dynamic.py:38-50): cdf [nb] in LDS, bins `bin_at(k)`, k < nb.  Every index is clamped,
// whatever the cdf holds.
template <typename B>
__device__ __forceinline__ float invert_cdf(const double* cdf, uint32_t nb, B bin_at, float uf) {
    const double u = (double)uf;
    uint32_t lo = 0, hi = nb;  // searchsorted(cdf, u, right=True): the number of entries <= u
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cdf[mid] <= u) lo = mid + 1; else hi = mid;
    }
    const uint32_t below = lo > 0 ? lo - 1 : 0, above = lo < nb - 1 ? lo : nb - 1;
    const double c0 = cdf[below];
    double denom = cdf[above] - c0;
    if (denom < (double)1e-5f) denom = 1.0;
    const double b0 = (double)bin_at(below), b1 = (double)bin_at(above);
    const double t = (u - c0) / denom;
    return (float)(b0 + t * (b1 - b0));
}

__global__ __launch_bounds__(kBlock) void k_sample_pdf(const float* __restrict__ bins, const float* __restrict__ weights,
                                                       const float* __restrict__ u, uint32_t u_per_ray, uint32_t B, uint32_t nb, uint32_t U,
                                                       float* __restrict__ samples) {
    extern __shared__ double lds[];
    const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
    const uint32_t ray = blockIdx.x * kRaysPerBlock + wave;
    if (ray >= B) return;
    const size_t n = ray;
    double* cdf = lds + (size_t)wave * (nb + (nb + 1) / 2);
    float* bs = (float*)(cdf + nb);
    for (uint32_t i = lane; i < nb; i += 64) bs[i] = bins[n * nb + i];
    const float* w = weights + n * (nb - 1);
    build_cdf([&](uint32_t i) { return w[i] + 1e-5f; }, nb - 1, cdf, lane);
    wave_lds_sync();
    const float* ur = u + (u_per_ray ? n * U : 0);
    for (uint32_t j = lane; j < U; j += 64) {
        const float s = invert_cdf(cdf, nb, [&](uint32_t k) { return bs[k]; }, ur[j]);
        samples[n * U + j] = s;
    }
}

// steps 2-4 of DESIGN.md section 9j.  P = U rounded up to a power of two (the sorting network's length).
__global__ __launch_bounds__(kBlock) void k_resample_merge(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                           const float* __restrict__ aabb, const float* __restrict__ z_vals,
                                                           const float* __restrict__ weights, const float* __restrict__ u, uint32_t u_per_ray,
                                                           uint32_t N, uint32_t T, uint32_t U, uint32_t P, float* __restrict__ z_new,
                                                           float* __restrict__ xyz_new, float* __restrict__ z_merged, int32_t* __restrict__ src) {
    extern __shared__ double lds[];
    const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
    const uint32_t ray = blockIdx.x * kRaysPerBlock + wave;
    if (ray >= N) return;
    const size_t n = ray;
    double* cdf = lds + (size_t)wave * (T + (T + P + 1) / 2);
    float* zs = (float*)(cdf + T);
    float* fs = zs + T;
    const uint32_t nb = T - 1;
    for (uint32_t i = lane; i < T; i += 64) zs[i] = z_vals[n * T + i];
    const float* w = weights + n * T + 1;  // the pdf weights are weights[:, 1 : T-1]
    build_cdf([&](uint32_t i) {
        const float v = w[i];
        return ((v >= 0.0f && v <= FLT_MAX) ? v : 0.0f) + 1e-5f;  // non-finite or negative: 0, for the sampling only
    }, nb - 1, cdf, lane);
    wave_lds_sync();
    const float* ur = u + (u_per_ray ? n * U : 0);
    for (uint32_t j = lane; j < P; j += 64)
        fs[j] = j < U ? invert_cdf(cdf, nb, [&](uint32_t k) { const float a = zs[k]; return a + 0.5f * (zs[k + 1] - a); }, ur[j]) : INFINITY;
    wave_lds_sync();
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane; t < P / 2; t += 64) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                const bool up = (i & k) == 0;
                const float a = fs[i], b = fs[l];
                if ((a > b) == up && a != b) { fs[i] = b; fs[l] = a; }
            }
            wave_lds_sync();
        }
    }
    const size_t TU = (size_t)T + U;
    float o[3], d[3], lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = rays_o[3 * n + k]; d[k] = rays_d[3 * n + k]; lo[k] = aabb[k]; hi[k] = aabb[3 + k]; }
    for (uint32_t j = lane; j < U; j += 64) {
        const float f = fs[j];
        z_new[n * U + j] = f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float p = o[k] + d[k] * f;
            xyz_new[3 * (n * U + j) + k] = fminf(fmaxf(p, lo[k]), hi[k]);
        }
        uint32_t a = 0, b = T;  // coarse values <= f come first
        while (a < b) {
            const uint32_t m = (a + b) >> 1;
            if (zs[m] <= f) a = m + 1; else b = m;
        }
        z_merged[n * TU + j + a] = f;
        src[n * TU + j + a] = (int32_t)(T + j);
    }
    for (uint32_t i = lane; i < T; i += 64) {
        const float z = zs[i];
        uint32_t a = 0, b = U;  // fine values strictly smaller come first
        while (a < b) {
            const uint32_t m = (a + b) >> 1;
            if (fs[m] < z) a = m + 1; else b = m;
        }
        z_merged[n * TU + i + a] = z;
        src[n * TU + i + a] = (int32_t)i;
    }
}

// out[n, s] = cat(a[n], b[n])[src[n, s]] in units of V (kSplit: the reverse copy, out is read).  An index outside [0, T + U) moves nothing.
template <typename V, bool kSplit>
__global__ __launch_bounds__(kBlock) void k_move_rows(V* __restrict__ a, V* __restrict__ b, const int32_t* __restrict__ src, size_t total,
                                                      uint32_t T, uint32_t U, uint32_t units, V* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= total) return;
    const size_t row = idx / units;
    const uint32_t k = (uint32_t)(idx - row * units);
    const size_t n = row / ((size_t)T + U);
    const uint32_t s = (uint32_t)src[row];
    if (s >= T + U) return;
    V* p = s < T ? a + (n * T + s) * units + k : b + (n * U + (s - T)) * units + k;
    if (kSplit) *p = out[idx]; else out[idx] = *p;
}

template <bool kSplit>
int move_rows(void* a, void* b, const int32_t* src, uint32_t N, uint32_t T, uint32_t U, uint32_t row_bytes, void* out, hipStream_t stream) {
    if (N == 0) return NVSF_OK;
    REQUIRE(a && b && src && out && T > 0 && U > 0 && row_bytes > 0);
    const unsigned long long rows = (unsigned long long)N * ((unsigned long long)T + U);
    REQUIRE(rows < (1ull << 31) && rows * row_bytes < (1ull << 40));
    const uintptr_t align = (uintptr_t)a | (uintptr_t)b | (uintptr_t)out | row_bytes;
#define NVSF_MOVE(V)                                                                                                                   \
    {                                                                                                                                  \
        const uint32_t units = row_bytes / (uint32_t)sizeof(V);                                                                        \
        const size_t total = (size_t)rows * units;                                                                                     \
        hipLaunchKernelGGL((k_move_rows<V, kSplit>), dim3(cdiv(total, kBlock)), dim3(kBlock), 0, stream, (V*)a, (V*)b, src, total, T, U, \
                           units, (V*)out);                                                                                            \
    }
    if (align % 16 == 0) NVSF_MOVE(uint4)
    else if (align % 4 == 0) NVSF_MOVE(uint32_t)
    else if (align % 2 == 0) NVSF_MOVE(uint16_t)
    else NVSF_MOVE(uint8_t)
#undef NVSF_MOVE
    return nvsf_launch_status();
}

uint32_t pow2_at_least(uint32_t v) {
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}
}  // namespace

NVSF_API int nvsf_sample_pdf(const float* bins, const float* weights, const float* u, uint32_t u_per_ray, uint32_t B, uint32_t nb, uint32_t U,
                             float* samples, hipStream_t stream) {
    if (B == 0) return NVSF_OK;
    REQUIRE(bins && weights && u && samples && nb >= 2 && U >= 1);
    if (nb > kMaxBins || U > kMaxDraws) return NVSF_ERR_UNSUPPORTED;
    const size_t lds_bytes = (size_t)kRaysPerBlock * (nb + (nb + 1) / 2) * sizeof(double);
    hipLaunchKernelGGL(k_sample_pdf, dim3(cdiv(B, kRaysPerBlock)), dim3(kBlock), lds_bytes, stream, bins, weights, u, u_per_ray, B, nb, U, samples);
    return nvsf_launch_status();
}

NVSF_API int nvsf_resample_merge(const float* rays_o, const float* rays_d, const float* aabb, const float* z_vals, const float* weights,
                                 const float* u, uint32_t u_per_ray, uint32_t N, uint32_t T, uint32_t U, float* z_new, float* xyz_new,
                                 float* z_merged, int32_t* src, hipStream_t stream) {
    if (N == 0) return NVSF_OK;
    REQUIRE(rays_o && rays_d && aabb && z_vals && weights && u && z_new && xyz_new && z_merged && src && T >= 3 && U >= 1);
    if (T > kMaxCoarse || U > kMaxFine) return NVSF_ERR_UNSUPPORTED;
    REQUIRE((unsigned long long)N * ((unsigned long long)T + U) < (1ull << 31));
    const uint32_t P = pow2_at_least(U);
    const size_t lds_bytes = (size_t)kRaysPerBlock * (T + (T + P + 1) / 2) * sizeof(double);  // at most 53 248 bytes
    hipLaunchKernelGGL(k_resample_merge, dim3(cdiv(N, kRaysPerBlock)), dim3(kBlock), lds_bytes, stream, rays_o, rays_d, aabb, z_vals, weights,
                       u, u_per_ray, N, T, U, P, z_new, xyz_new, z_merged, src);
    return nvsf_launch_status();
}

NVSF_API int nvsf_merge_rows(const void* a, const void* b, const int32_t* src, uint32_t N, uint32_t T, uint32_t U, uint32_t row_bytes, void* out,
                             hipStream_t stream) {
    return move_rows<false>(const_cast<void*>(a), const_cast<void*>(b), src, N, T, U, row_bytes, out, stream);
}

NVSF_API int nvsf_split_rows(const void* merged, const int32_t* src, uint32_t N, uint32_t T, uint32_t U, uint32_t row_bytes, void* a, void* b,
                             hipStream_t stream) {
    return move_rows<true>(a, b, src, N, T, U, row_bytes, const_cast<void*>(merged), stream);
}
