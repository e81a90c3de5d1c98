// Evaluation meters on the device, gfx950: the arithmetic of the reference's meter classes (nvsf/lib/error_matrices.py:28-157 PSNR / RMSE /
// MAE, :159-297 the LiDAR range and intensity tables, :359-413 ray-drop, :415-470 SSIM) over whole rendered frames that already live in
// device memory.  Four entry points (include/nvsf_hip.h section 10); each leaves its statistics in a caller-supplied device buffer, so a
// frame's table costs no device -> host copy until the meter is read.
//
// Determinism: no floating-point atomic anywhere.  Every sum is fp64: a thread adds its elements in index order, a wave folds its lanes
// in a fixed butterfly, a workgroup its waves in wave order, and the per-workgroup partials go to the workspace, where ONE workgroup
// folds them in a fixed order.  The only atomics are the integer ones of the median's histograms, whose result does not depend on the
// order they land in.  Two runs give the same bits.
//
// k_ssim_tiles: a workgroup owns a 32 x 16 tile of window positions.  It stages the (16 + size - 1) x (32 + size - 1) pixels under them,
// both images and all channels, in LDS (fp32, de-interleaved: 26 KiB at size 11), then per channel filters the five moments
// p, t, pp, tt, pt along the rows into an fp64 LDS image (33 KiB) and along the columns into registers: the window is separable.  A wave
// reads 32 consecutive floats of two tile rows (row pass) or 32 consecutive doubles of two image rows (column pass): no bank conflict
// under either banking rule.  59.5 KiB of LDS: two workgroups per CU.
#include "common.h"
#include <math.h>

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr uint32_t kMaxPartials = 2048;  // workgroups of a streaming reduction = rows of its workspace
constexpr uint32_t kMaxElems = 1u << 30;
constexpr int kStatCols = 8;             // sum d^2, sum |d|, min t, max t, min p, max p, NaN seen in t, NaN seen in p

// the reference's `x[x < lo] = lo; x[x > hi] = hi` (error_matrices.py:266-269): NaN fails both tests and passes through
__device__ __forceinline__ float clamp_ref(float x, float lo, float hi) {
    x = x < lo ? lo : x;
    return x > hi ? hi : x;
}

struct Sum { __device__ static double op(double a, double b) { return a + b; } };
struct Min { __device__ static double op(double a, double b) { return fmin(a, b); } };
struct Max { __device__ static double op(double a, double b) { return fmax(a, b); } };

// fixed-order workgroup fold; the result is valid in thread 0.  `sh`: kWaves doubles of LDS owned by this call.
template <typename Op>
__device__ __forceinline__ double block_fold(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = Op::op(v, __shfl_xor(v, o, 64));
    if (lane_id() == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sh[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) r = Op::op(r, sh[w]);
    return r;
}

// ---- image_error_stats ---------------------------------------------------------------------------------------------------------
// kWide: d = t - p formed in fp64 (numpy, once one operand of the difference is a float64 array: RMSEMeter's camera-depth form)
template <bool kWide>
__global__ __launch_bounds__(kBlock) void k_error_stats(const float* __restrict__ pred, const float* __restrict__ truth, uint32_t n, float lo,
                                                        float hi, double* __restrict__ partial) {
    __shared__ double sh[kStatCols][kWaves];
    double s2 = 0.0, s1 = 0.0, tmin = INFINITY, tmax = -INFINITY, pmin = INFINITY, pmax = -INFINITY, nt = 0.0, np_ = 0.0;
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const float p = clamp_ref(pred[i], lo, hi), t = clamp_ref(truth[i], lo, hi);
        const double d = kWide ? (double)t - (double)p : (double)(t - p);  // fp32 difference: as numpy forms it on the reference's fp32 arrays
        s2 += d * d;
        s1 += fabs(d);
        tmin = fmin(tmin, (double)t); tmax = fmax(tmax, (double)t);
        pmin = fmin(pmin, (double)p); pmax = fmax(pmax, (double)p);
        nt += t != t ? 1.0 : 0.0;
        np_ += p != p ? 1.0 : 0.0;
    }
    double r[kStatCols];
    r[0] = block_fold<Sum>(s2, sh[0]);   r[1] = block_fold<Sum>(s1, sh[1]);
    r[2] = block_fold<Min>(tmin, sh[2]); r[3] = block_fold<Max>(tmax, sh[3]);
    r[4] = block_fold<Min>(pmin, sh[4]); r[5] = block_fold<Max>(pmax, sh[5]);
    r[6] = block_fold<Sum>(nt, sh[6]);   r[7] = block_fold<Sum>(np_, sh[7]);
    if (threadIdx.x == 0)
        for (int c = 0; c < kStatCols; ++c) partial[(size_t)blockIdx.x * kStatCols + c] = r[c];
}

__global__ __launch_bounds__(kBlock) void k_error_stats_fold(const double* __restrict__ partial, uint32_t rows, double* __restrict__ out) {
    __shared__ double sh[kStatCols][kWaves];
    double a[kStatCols] = {0.0, 0.0, INFINITY, -INFINITY, INFINITY, -INFINITY, 0.0, 0.0};
    for (uint32_t r = threadIdx.x; r < rows; r += kBlock) {
        const double* q = partial + (size_t)r * kStatCols;
        a[0] += q[0]; a[1] += q[1]; a[2] = fmin(a[2], q[2]); a[3] = fmax(a[3], q[3]); a[4] = fmin(a[4], q[4]); a[5] = fmax(a[5], q[5]);
        a[6] += q[6]; a[7] += q[7];
    }
    double r[kStatCols];
    r[0] = block_fold<Sum>(a[0], sh[0]); r[1] = block_fold<Sum>(a[1], sh[1]);
    r[2] = block_fold<Min>(a[2], sh[2]); r[3] = block_fold<Max>(a[3], sh[3]);
    r[4] = block_fold<Min>(a[4], sh[4]); r[5] = block_fold<Max>(a[5], sh[5]);
    r[6] = block_fold<Sum>(a[6], sh[6]); r[7] = block_fold<Sum>(a[7], sh[7]);
    if (threadIdx.x == 0) {
        out[0] = r[0]; out[1] = r[1];
        // numpy's min / max return NaN as soon as one element is NaN; fmin / fmax skip it
        out[2] = r[6] > 0.0 ? (double)NAN : r[2]; out[3] = r[6] > 0.0 ? (double)NAN : r[3];
        out[4] = r[7] > 0.0 ? (double)NAN : r[4]; out[5] = r[7] > 0.0 ? (double)NAN : r[5];
    }
}

// ---- raydrop_confusion ---------------------------------------------------------------------------------------------------------
constexpr int kDropCols = 6;  // TP, FP, TN, FN, equal (uint64) and sum d^2 (fp64)

__global__ __launch_bounds__(kBlock) void k_raydrop(const float* __restrict__ pred, const float* __restrict__ truth, uint32_t n, float ratio,
                                                    uint64_t* __restrict__ partial) {
    __shared__ uint32_t shc[5][kWaves];
    __shared__ double shd[kWaves];
    uint32_t c[5] = {0, 0, 0, 0, 0};
    double s2 = 0.0;
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const float p = pred[i], t = truth[i];
        const bool on = p > ratio;  // np.where(preds > ratio, 1, 0): NaN -> 0
        c[0] += (t == 1.0f && on);
        c[1] += (t == 0.0f && on);
        c[2] += (t == 0.0f && !on);
        c[3] += (t == 1.0f && !on);
        c[4] += (t == (on ? 1.0f : 0.0f));
        const float d = t - p;
        s2 += (double)d * (double)d;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint32_t w = wave_sum(c[k]);
        if (lane_id() == 0) shc[k][threadIdx.x >> 6] = w;
    }
    const double s = block_fold<Sum>(s2, shd);  // its barrier also publishes shc
    if (threadIdx.x == 0) {
        uint64_t* row = partial + (size_t)blockIdx.x * kDropCols;
        for (int k = 0; k < 5; ++k) {
            uint64_t tot = 0;
            for (int w = 0; w < kWaves; ++w) tot += shc[k][w];
            row[k] = tot;
        }
        row[5] = (uint64_t)__double_as_longlong(s);
    }
}

__global__ __launch_bounds__(kBlock) void k_raydrop_fold(const uint64_t* __restrict__ partial, uint32_t rows, uint64_t* __restrict__ out) {
    __shared__ unsigned long long shc[5][kWaves];
    __shared__ double shd[kWaves];
    unsigned long long c[5] = {0, 0, 0, 0, 0};
    double s2 = 0.0;
    for (uint32_t r = threadIdx.x; r < rows; r += kBlock) {
        const uint64_t* q = partial + (size_t)r * kDropCols;
        for (int k = 0; k < 5; ++k) c[k] += q[k];
        s2 += __longlong_as_double((long long)q[5]);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const unsigned long long w = wave_sum(c[k]);
        if (lane_id() == 0) shc[k][threadIdx.x >> 6] = w;
    }
    const double s = block_fold<Sum>(s2, shd);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 5; ++k) {
            uint64_t tot = 0;
            for (int w = 0; w < kWaves; ++w) tot += shc[k][w];
            out[k] = tot;
        }
        out[5] = (uint64_t)__double_as_longlong(s);
    }
}

// ---- median_abs_error: radix select over the bit patterns of |t - p| -------------------------------------------------------------
// A non-negative fp32 orders as its bit pattern does (+inf above every finite value, NaNs above +inf).  Three passes over the data pick
// 11, 10 and 10 bits of the two middle order statistics (ranks (n - 1) / 2 and n / 2): a pass histograms the digit of every element
// that matches the prefix found so far, one workgroup then walks the histogram to the bin that holds the rank.
constexpr int kMedState = 16;      // uint32: prefix A, prefix B, rank A, rank B, NaN count
constexpr int kMedBins = 2048;
constexpr size_t kMedWsBytes = (size_t)(kMedState + 2 * kMedBins) * sizeof(uint32_t);

__global__ __launch_bounds__(kBlock) void k_median_init(uint32_t* __restrict__ ws, uint32_t n) {
    for (uint32_t e = threadIdx.x; e < kMedState + 2 * kMedBins; e += kBlock) ws[e] = e == 2 ? (n - 1) / 2 : e == 3 ? n / 2 : 0u;
}

// one LDS atomic per lane, except that the lanes sharing the first active lane's bin go in as one add: a frame's abs errors hold long
// runs of one value (exact zeros where both rays are dropped), which would otherwise queue up on one LDS address
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t bin, bool active) {
    const unsigned long long live = __ballot(active);
    if (!live) return;
    const int first = __ffsll((long long)live) - 1;
    const uint32_t lead = (uint32_t)__builtin_amdgcn_readlane((int)bin, first);
    const unsigned long long same = __ballot(active && bin == lead);
    if (active) {
        if (bin != lead) atomicAdd(&hist[bin], 1u);
        else if (lane_id() == first) atomicAdd(&hist[lead], (uint32_t)__popcll(same));
    }
}

__global__ __launch_bounds__(kBlock) void k_median_hist(const float* __restrict__ pred, const float* __restrict__ truth, uint32_t n, float lo,
                                                        float hi, uint32_t* __restrict__ ws, uint32_t shift, uint32_t nbits, int first_pass) {
    __shared__ uint32_t hist[2][kMedBins];
    const uint32_t bins = 1u << nbits, top = shift + nbits;  // top <= 31
    const uint32_t pa = ws[0] >> top, pb = ws[1] >> top;
    const bool two = pa != pb;  // workgroup-uniform
    for (uint32_t e = threadIdx.x; e < 2 * kMedBins; e += kBlock) (&hist[0][0])[e] = 0;
    __syncthreads();
    uint32_t nans = 0;
    const uint32_t stride = gridDim.x * kBlock;
    const uint32_t rounds = (n + stride - 1) / stride;  // every lane runs every round: hist_add votes across the wave
    for (uint32_t k = 0; k < rounds; ++k) {
        const uint32_t i = k * stride + blockIdx.x * kBlock + threadIdx.x;
        const bool live = i < n;
        uint32_t key = 0;
        if (live) key = __float_as_uint(fabsf(clamp_ref(truth[i], lo, hi) - clamp_ref(pred[i], lo, hi)));
        nans += (live && key > 0x7f800000u);
        const uint32_t bin = (key >> shift) & (bins - 1), pre = key >> top;
        hist_add(hist[0], bin, live && pre == pa);
        if (two) hist_add(hist[1], bin, live && pre == pb);
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < bins; e += kBlock) {
        if (hist[0][e]) atomicAdd(ws + kMedState + e, hist[0][e]);
        if (two && hist[1][e]) atomicAdd(ws + kMedState + kMedBins + e, hist[1][e]);
    }
    if (first_pass) {
        nans = wave_sum(nans);
        if (lane_id() == 0 && nans) atomicAdd(ws + 4, nans);
    }
}

__global__ __launch_bounds__(kBlock) void k_median_select(uint32_t* __restrict__ ws, uint32_t shift, uint32_t nbits, uint32_t n, int last,
                                                          double* __restrict__ out) {
    __shared__ uint32_t h[2][kMedBins];
    __shared__ uint32_t wtot[2][kWaves];
    __shared__ uint32_t found[2][2];  // new prefix, new rank
    const uint32_t bins = 1u << nbits, top = shift + nbits, per = bins / kBlock;
    const uint32_t prefix[2] = {ws[0], ws[1]}, rank[2] = {ws[2], ws[3]};
    const bool two = (prefix[0] >> top) != (prefix[1] >> top);
    for (uint32_t e = threadIdx.x; e < bins; e += kBlock) {
        h[0][e] = ws[kMedState + e];
        h[1][e] = two ? ws[kMedState + kMedBins + e] : h[0][e];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    for (int s = 0; s < 2; ++s) {
        uint32_t c = 0;
        for (uint32_t j = 0; j < per; ++j) c += h[s][threadIdx.x * per + j];
        const uint32_t inc = wave_scan_add_u32(c);
        if (lane_id() == 63) wtot[s][wave] = inc;
        __syncthreads();
        uint32_t before = inc - c;
        for (int w = 0; w < wave; ++w) before += wtot[s][w];
        if (rank[s] >= before && rank[s] - before < c) {  // exactly one thread: the counts of a pass add up to more than the rank
            uint32_t j = 0;
            while (rank[s] - before >= h[s][threadIdx.x * per + j]) before += h[s][threadIdx.x * per + j++];
            found[s][0] = prefix[s] | ((threadIdx.x * per + j) << shift);
            found[s][1] = rank[s] - before;
        }
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < 2 * kMedBins; e += kBlock) ws[kMedState + e] = 0;  // the next pass adds into zeros
    if (threadIdx.x == 0) {
        ws[0] = found[0][0]; ws[1] = found[1][0]; ws[2] = found[0][1]; ws[3] = found[1][1];
        if (last) {
            const float a = __uint_as_float(found[0][0]), b = __uint_as_float(found[1][0]);
            // np.median of a float32 array: the middle value, or the float32 mean of the two middle values; NaN if any element is
            const float m = ws[4] ? NAN : (n & 1u) ? a : (a + b) / 2.0f;
            out[0] = (double)m;
        }
    }
}

// ---- ssim_mean -----------------------------------------------------------------------------------------------------------------
constexpr int kTW = 32, kTH = 16, kMaxWin = 11, kInW = kTW + kMaxWin - 1, kInH = kTH + kMaxWin - 1, kMaxC = 3;
struct SsimWindow { double w[kMaxWin]; };

template <bool kUniform>
__device__ __forceinline__ void tap(double& acc, double v, double w) {
    if (kUniform) acc += v; else acc += w * v;
}

template <bool kUniform>
__global__ __launch_bounds__(kBlock) void k_ssim_tiles(const float* __restrict__ pred, const float* __restrict__ truth, uint32_t H, uint32_t W,
                                                       uint32_t C, uint32_t size, SsimWindow win, double cov_norm,
                                                       const double* __restrict__ range_ptr, double* __restrict__ partial) {
    __shared__ float tp[kMaxC][kInH][kInW], tt[kMaxC][kInH][kInW];
    __shared__ double rows[5][kInH][kTW];
    __shared__ double red[kWaves];
    const uint32_t OH = H - size + 1, OW = W - size + 1;
    const uint32_t ox0 = blockIdx.x * kTW, oy0 = blockIdx.y * kTH;
    const uint32_t inh = kTH + size - 1, inw = kTW + size - 1;  // <= kInH, kInW
    // stage: consecutive threads read consecutive floats of an image row; pixels past the image are zero and feed only window
    // positions that are not counted
    for (uint32_t e = threadIdx.x; e < inh * inw * C; e += kBlock) {
        const uint32_t r = e / (inw * C), rem = e - r * (inw * C), col = rem / C, ch = rem - col * C;
        const uint32_t y = oy0 + r, x = ox0 + col;
        const bool in = y < H && x < W;
        const size_t g = ((size_t)y * W + x) * C + ch;
        tp[ch][r][col] = in ? pred[g] : 0.0f;
        tt[ch][r][col] = in ? truth[g] : 0.0f;
    }
    const double R = range_ptr[0];
    const double c1 = (0.01 * R) * (0.01 * R), c2 = (0.03 * R) * (0.03 * R);
    const double inv = (double)size;
    double acc = 0.0;
    for (uint32_t ch = 0; ch < C; ++ch) {
        __syncthreads();  // the tile is staged / the previous channel's columns are done with `rows`
        for (uint32_t it = threadIdx.x; it < inh * kTW; it += kBlock) {
            const uint32_t r = it / kTW, x = it % kTW;
            double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            for (uint32_t k = 0; k < size; ++k) {
                const double a = (double)tp[ch][r][x + k], b = (double)tt[ch][r][x + k], w = win.w[k];
                tap<kUniform>(m[0], a, w); tap<kUniform>(m[1], b, w); tap<kUniform>(m[2], a * a, w); tap<kUniform>(m[3], b * b, w);
                tap<kUniform>(m[4], a * b, w);
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) rows[q][r][x] = kUniform ? m[q] / inv : m[q];
        }
        __syncthreads();
        for (uint32_t o = threadIdx.x; o < kTH * kTW; o += kBlock) {
            const uint32_t y = o / kTW, x = o % kTW;
            double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            for (uint32_t k = 0; k < size; ++k) {
                const double w = win.w[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) tap<kUniform>(m[q], rows[q][y + k][x], w);
            }
            if (kUniform) {
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] /= inv;  // sum, then divide: a constant window gives its value back exactly
            }
            const double vp = cov_norm * (m[2] - m[0] * m[0]), vt = cov_norm * (m[3] - m[1] * m[1]), vpt = cov_norm * (m[4] - m[0] * m[1]);
            const double s = ((2.0 * m[0] * m[1] + c1) * (2.0 * vpt + c2)) / ((m[0] * m[0] + m[1] * m[1] + c1) * (vp + vt + c2));
            if (oy0 + y < OH && ox0 + x < OW) acc += s;
        }
    }
    const double tot = block_fold<Sum>(acc, red);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

__global__ __launch_bounds__(kBlock) void k_mean_fold(const double* __restrict__ partial, uint32_t rows, double count, double* __restrict__ out) {
    __shared__ double red[kWaves];
    double a = 0.0;
    for (uint32_t r = threadIdx.x; r < rows; r += kBlock) a += partial[r];
    const double tot = block_fold<Sum>(a, red);
    if (threadIdx.x == 0) out[0] = tot / count;
}

static inline uint32_t host_streaming_grid(uint32_t n) {
    const uint32_t g = cdiv(n, kBlock * 4);
    return g < kMaxPartials ? g : kMaxPartials;
}
}  // namespace

NVSF_API int nvsf_image_error_stats(const float* pred, const float* truth, uint32_t n, float lo, float hi, void* workspace, size_t ws_bytes,
                                    double* out, hipStream_t stream) {
    REQUIRE(pred && truth && workspace && out && n >= 1 && n <= kMaxElems && !(lo > hi));
    const uint32_t grid = host_streaming_grid(n);
    REQUIRE(ws_bytes >= (size_t)grid * kStatCols * sizeof(double) && ((uintptr_t)workspace & 7) == 0);
    hipLaunchKernelGGL(k_error_stats<false>, dim3(grid), dim3(kBlock), 0, stream, pred, truth, n, lo, hi, (double*)workspace);
    hipLaunchKernelGGL(k_error_stats_fold, dim3(1), dim3(kBlock), 0, stream, (const double*)workspace, grid, out);
    return nvsf_launch_status();
}

NVSF_API int nvsf_image_error_stats_wide(const float* pred, const float* truth, uint32_t n, float lo, float hi, void* workspace, size_t ws_bytes,
                                         double* out, hipStream_t stream) {
    REQUIRE(pred && truth && workspace && out && n >= 1 && n <= kMaxElems && !(lo > hi));
    const uint32_t grid = host_streaming_grid(n);
    REQUIRE(ws_bytes >= (size_t)grid * kStatCols * sizeof(double) && ((uintptr_t)workspace & 7) == 0);
    hipLaunchKernelGGL(k_error_stats<true>, dim3(grid), dim3(kBlock), 0, stream, pred, truth, n, lo, hi, (double*)workspace);
    hipLaunchKernelGGL(k_error_stats_fold, dim3(1), dim3(kBlock), 0, stream, (const double*)workspace, grid, out);
    return nvsf_launch_status();
}

NVSF_API int nvsf_raydrop_confusion(const float* pred, const float* truth, uint32_t n, float ratio, void* workspace, size_t ws_bytes,
                                    uint64_t* out, hipStream_t stream) {
    REQUIRE(pred && truth && workspace && out && n >= 1 && n <= kMaxElems);
    const uint32_t grid = host_streaming_grid(n);
    REQUIRE(ws_bytes >= (size_t)grid * kDropCols * sizeof(uint64_t) && ((uintptr_t)workspace & 7) == 0);
    hipLaunchKernelGGL(k_raydrop, dim3(grid), dim3(kBlock), 0, stream, pred, truth, n, ratio, (uint64_t*)workspace);
    hipLaunchKernelGGL(k_raydrop_fold, dim3(1), dim3(kBlock), 0, stream, (const uint64_t*)workspace, grid, out);
    return nvsf_launch_status();
}

NVSF_API int nvsf_median_abs_error(const float* pred, const float* truth, uint32_t n, float lo, float hi, void* workspace, size_t ws_bytes,
                                   double* out, hipStream_t stream) {
    REQUIRE(pred && truth && workspace && out && n >= 1 && n <= kMaxElems && !(lo > hi));
    REQUIRE(ws_bytes >= kMedWsBytes && ((uintptr_t)workspace & 3) == 0);
    uint32_t* ws = (uint32_t*)workspace;
    const uint32_t grid = host_streaming_grid(n);
    hipLaunchKernelGGL(k_median_init, dim3(1), dim3(kBlock), 0, stream, ws, n);
    const uint32_t shifts[3] = {20, 10, 0}, nbits[3] = {11, 10, 10};
    for (int p = 0; p < 3; ++p) {
        hipLaunchKernelGGL(k_median_hist, dim3(grid), dim3(kBlock), 0, stream, pred, truth, n, lo, hi, ws, shifts[p], nbits[p], p == 0);
        hipLaunchKernelGGL(k_median_select, dim3(1), dim3(kBlock), 0, stream, ws, shifts[p], nbits[p], n, p == 2, out);
    }
    return nvsf_launch_status();
}

NVSF_API int nvsf_ssim_mean(const float* pred, const float* truth, uint32_t H, uint32_t W, uint32_t C, int window, uint32_t size, float sigma,
                            int sample_cov, const double* range_ptr, void* workspace, size_t ws_bytes, double* out, hipStream_t stream) {
    REQUIRE(pred && truth && range_ptr && workspace && out);
    REQUIRE((C == 1 || C == 3) && (window == 0 || window == 1) && (sample_cov == 0 || sample_cov == 1));
    REQUIRE(size >= 3 && size <= (uint32_t)kMaxWin && (size & 1u) == 1u && H >= size && W >= size && H <= (1u << 15) && W <= (1u << 15));
    REQUIRE(window == 0 || (sigma > 0.0f && sigma < INFINITY));
    const uint32_t OH = H - size + 1, OW = W - size + 1;
    const dim3 grid(cdiv(OW, kTW), cdiv(OH, kTH));
    const uint32_t tiles = grid.x * grid.y;
    REQUIRE(ws_bytes >= (size_t)tiles * sizeof(double) && ((uintptr_t)workspace & 7) == 0);
    SsimWindow win;
    double total = 0.0;
    for (uint32_t k = 0; k < (uint32_t)kMaxWin; ++k) {
        const double d = ((double)k - (double)(size - 1) / 2.0) / (double)sigma;
        win.w[k] = k < size ? (window == 1 ? exp(-0.5 * d * d) : 1.0) : 0.0;
        total += win.w[k];
    }
    for (uint32_t k = 0; k < (uint32_t)kMaxWin; ++k) win.w[k] /= total;
    const double np = (double)size * (double)size;
    const double cov_norm = sample_cov ? np / (np - 1.0) : 1.0;
    if (window == 0)
        hipLaunchKernelGGL(k_ssim_tiles<true>, grid, dim3(kBlock), 0, stream, pred, truth, H, W, C, size, win, cov_norm, range_ptr, (double*)workspace);
    else
        hipLaunchKernelGGL(k_ssim_tiles<false>, grid, dim3(kBlock), 0, stream, pred, truth, H, W, C, size, win, cov_norm, range_ptr, (double*)workspace);
    hipLaunchKernelGGL(k_mean_fold, dim3(1), dim3(kBlock), 0, stream, (const double*)workspace, tiles, (double)OH * (double)OW * (double)C, out);
    return nvsf_launch_status();
}
