// Order statistics of a ray's termination distribution (include/nvsf_hip.h section 16): quantile ranges, the
// strongest return and the spread of weights / z_vals [N, T], and the gradient of the quantile ranges with respect to the weights.
//
// Per ray, with the compositor's intervals (uniform.hip: delta_i = z_{i+1} - z_i, delta_{T-1} = (far - near) / T), the inclusive prefix
// sums C_i of w (C_{-1} = 0, W = C_{T-1}) and sample i's mass spread uniformly over [z_i, z_i + delta_i]:
//   quantile  t_q = z_i + delta_i (tau - C_{i-1}) / w_i at the first i with C_i >= tau;  tau = q W (normalised) or q (absolute)
//   mode      z_i of the first i that attains max w
//   std       sqrt(sum_i w_i (z_i - mu)^2 / W),  mu = sum_i w_i z_i / W
// A row with W = 0 gives 0 everywhere; in the absolute form a row with W < q gives a zero quantile ("no return").
//
// One wave per ray, four rays per workgroup, lane = sample in chunks of 64 (4-byte loads, any alignment), every sum and the scan in fp64
// from the fp32 inputs, one rounding on store.  tau = q W needs the row total before the first crossing can be told, so the row is
// walked twice: the first walk leaves W and sum w z, the second finds the crossings, the arg-max and the central second moment.  W is
// NOT taken from the compositor's fp32 `weights_sum`: the crossing test C_i >= q W has to see the very total its own scan ends in
// (q = 1 must cross in the last positive sample, not past the row), so both walks scan with the same instructions and the same carry.
// The second walk reads a row the first left in the cache (3 KB a row at T = 768).
// Wave-uniform control flow throughout (the DPP scan needs every lane), vector stores, no LDS, no atomics.
#include "common.h"

#include <math.h>

namespace {
constexpr int kStatBlock = 256, kStatRays = kStatBlock / kWave, kStatMaxQ = 4;
struct StatLevels { double q[kStatMaxQ]; };

__device__ __forceinline__ double wave_bcast_f64(double v, int lane) { return __shfl(v, lane, 64); }

// one chunk of a row: this lane's weight, depth and interval (zero past T) and the row's prefix sums of w before / up to the lane
struct StatTile { double w, z, delta, c_lt, c_le; bool valid; };
__device__ __forceinline__ StatTile stat_tile(const float* __restrict__ w, const float* __restrict__ z, uint32_t base, uint32_t T,
                                              double last, double& run) {
    const uint32_t i = base + (uint32_t)lane_id();
    StatTile t;
    t.valid = i < T;
    t.w = t.z = t.delta = 0.0;
    if (t.valid) {
        t.w = (double)w[i];
        t.z = (double)z[i];
        t.delta = i + 1 < T ? (double)z[i + 1] - t.z : last;
    }
    const double s = wave_scan_add_f64(t.w);
    double e = __shfl_up(s, 1, 64);
    if (lane_id() == 0) e = 0.0;
    t.c_lt = run + e;
    t.c_le = run + s;
    run += wave_last_f64(s);
    return t;
}

// the row total exactly as stat_tile's carry ends, and sum w z
__device__ __forceinline__ void stat_totals(const float* __restrict__ w, const float* __restrict__ z, uint32_t T, double& W, double& M) {
    double run = 0.0, m = 0.0;
    for (uint32_t base = 0; base < T; base += kWave) {
        const uint32_t i = base + (uint32_t)lane_id();
        const double wi = i < T ? (double)w[i] : 0.0, zi = i < T ? (double)z[i] : 0.0;
        run += wave_last_f64(wave_scan_add_f64(wi));
        m += wi * zi;
    }
    W = run;
    M = wave_sum(m);
}

__global__ __launch_bounds__(kStatBlock) void k_ray_depth_stats_fwd(const float* __restrict__ weights, const float* __restrict__ z_vals,
                                                                    const float* __restrict__ nears, const float* __restrict__ fars,
                                                                    uint32_t N, uint32_t T, StatLevels lv, uint32_t Q, int normalize,
                                                                    float* __restrict__ quantiles, float* __restrict__ mode,
                                                                    float* __restrict__ std_out, double* __restrict__ state) {
    const uint32_t n = blockIdx.x * kStatRays + (threadIdx.x >> 6);
    if (n >= N) return;  // whole waves: n is wave-uniform
    const int lane = lane_id();
    const float* w = weights + (size_t)n * T;
    const float* z = z_vals + (size_t)n * T;
    const double last = ((double)fars[n] - (double)nears[n]) / (double)T;
    double W, M;
    stat_totals(w, z, T, W, M);
    double tau[kStatMaxQ], t_q[kStatMaxQ], a_q[kStatMaxQ];
    int idx[kStatMaxQ];
    uint32_t open = 0;  // levels whose crossing is still to be found
#pragma unroll
    for (int l = 0; l < kStatMaxQ; ++l) {
        tau[l] = normalize ? lv.q[l] * W : lv.q[l];
        t_q[l] = a_q[l] = 0.0;
        idx[l] = -1;
        if ((uint32_t)l < Q && W > 0.0 && W >= tau[l]) open |= 1u << l;
    }
    double mode_z = 0.0, sd = 0.0;
    if (W > 0.0) {
        const double mu = M / W;
        double run = 0.0, var = 0.0;
        float best_w = -1.0f;
        uint32_t best_i = 0, last_pos = 0;  // last_pos: 1 + the last index with a positive weight
        for (uint32_t base = 0; base < T; base += kWave) {
            const StatTile t = stat_tile(w, z, base, T, last, run);
            const uint32_t i = base + (uint32_t)lane;
#pragma unroll
            for (int l = 0; l < kStatMaxQ; ++l) {
                if (!(open >> l & 1u)) continue;
                // a zero weight never crosses: its two prefix sums come from different scan trees and may differ in the last bit
                const uint64_t hit = __ballot(t.valid && t.w > 0.0 && t.c_le >= tau[l]);
                if (hit == 0) continue;
                const int src = __ffsll((long long)hit) - 1;
                const double wi = wave_bcast_f64(t.w, src), zi = wave_bcast_f64(t.z, src), di = wave_bcast_f64(t.delta, src);
                const double a = fmin(fmax(tau[l] - wave_bcast_f64(t.c_lt, src), 0.0), wi);
                idx[l] = (int)(base + (uint32_t)src);
                a_q[l] = a;
                t_q[l] = zi + di * a / wi;
                open &= ~(1u << l);
            }
            if (t.valid) {
                const double d = t.z - mu;
                var += t.w * d * d;
                const float wf = (float)t.w;  // exact: the input is fp32
                if (wf > best_w) { best_w = wf; best_i = i; }
                if (wf > 0.0f) last_pos = i + 1;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {  // arg-max on (w, -i): the first index among equal weights
            const float ow = __shfl_xor(best_w, o, 64);
            const uint32_t oi = __shfl_xor(best_i, o, 64), ol = __shfl_xor(last_pos, o, 64);
            if (ow > best_w || (ow == best_w && oi < best_i)) { best_w = ow; best_i = oi; }
            last_pos = ol > last_pos ? ol : last_pos;
        }
        mode_z = (double)z[best_i];
        sd = sqrt(wave_sum(var) / W);
        // tau within a rounding of the row total and zero weights behind the last positive one: the crossing is that sample's end
        if (open != 0 && last_pos > 0) {
            const uint32_t i = last_pos - 1;
            const double wi = (double)w[i], zi = (double)z[i], di = i + 1 < T ? (double)z[i + 1] - zi : last;
#pragma unroll
            for (int l = 0; l < kStatMaxQ; ++l)
                if (open >> l & 1u) { idx[l] = (int)i; a_q[l] = wi; t_q[l] = zi + di; }
        }
    }
    if (lane == 0) {
        if (mode) mode[n] = (float)mode_z;
        if (std_out) std_out[n] = (float)sd;
    }
    if (lane < (int)Q) {
        double t = 0.0, a = 0.0, k = -1.0;
#pragma unroll
        for (int l = 0; l < kStatMaxQ; ++l)
            if (l == lane) { t = t_q[l]; a = a_q[l]; k = (double)idx[l]; }
        if (quantiles) quantiles[(size_t)n * Q + lane] = (float)t;
        if (state) {
            state[2 * ((size_t)n * Q + lane)] = k;
            state[2 * ((size_t)n * Q + lane) + 1] = a;
        }
    }
}

// grad_weights[n][j] = sum_l g_l (r_l (q_l [normalised] - [j < i_l]) - [j == i_l] delta_l a_l / w_l^2), r_l = delta_l / w_l, over the levels
// with a crossing i_l (state: i_l or -1, a_l = tau_l - C_{i_l - 1}): no scan, every entry of the row written once
__global__ __launch_bounds__(kStatBlock) void k_ray_depth_quantile_bwd(const float* __restrict__ weights, const float* __restrict__ z_vals,
                                                                       const float* __restrict__ nears, const float* __restrict__ fars,
                                                                       uint32_t N, uint32_t T, StatLevels lv, uint32_t Q, int normalize,
                                                                       const double* __restrict__ state, const float* __restrict__ grad_q,
                                                                       float* __restrict__ grad_w) {
    const uint32_t n = blockIdx.x * kStatRays + (threadIdx.x >> 6);
    if (n >= N) return;
    const float* w = weights + (size_t)n * T;
    const float* z = z_vals + (size_t)n * T;
    float* out = grad_w + (size_t)n * T;
    const double last = ((double)fars[n] - (double)nears[n]) / (double)T;
    double gr[kStatMaxQ], self[kStatMaxQ], all = 0.0;  // g r, g delta a / w^2, sum of g r q
    uint32_t at[kStatMaxQ];
#pragma unroll
    for (int l = 0; l < kStatMaxQ; ++l) {
        gr[l] = self[l] = 0.0;
        at[l] = 0;
        if ((uint32_t)l >= Q) continue;
        const double k = state[2 * ((size_t)n * Q + l)];
        if (k < 0.0) continue;
        const uint32_t i = (uint32_t)k;
        const double wi = (double)w[i], zi = (double)z[i], di = i + 1 < T ? (double)z[i + 1] - zi : last;
        const double g = (double)grad_q[(size_t)n * Q + l];
        at[l] = i;
        gr[l] = g * di / wi;
        self[l] = g * di * state[2 * ((size_t)n * Q + l) + 1] / (wi * wi);
        if (normalize) all += gr[l] * lv.q[l];
    }
    for (uint32_t j = (uint32_t)lane_id(); j < T; j += kWave) {
        double g = all;
#pragma unroll
        for (int l = 0; l < kStatMaxQ; ++l) {
            if (j < at[l]) g -= gr[l];
            if (j == at[l]) g -= self[l];
        }
        out[j] = (float)g;
    }
}

static inline bool levels_ok(const double* q, uint32_t Q, StatLevels& lv) {
    if (!q || Q < 1 || Q > (uint32_t)kStatMaxQ) return false;
    for (uint32_t l = 0; l < (uint32_t)kStatMaxQ; ++l) {
        lv.q[l] = l < Q ? q[l] : 1.0;
        if (!(lv.q[l] > 0.0 && lv.q[l] <= 1.0)) return false;  // refuses NaN as well
    }
    return true;
}
}  // namespace

NVSF_API int nvsf_ray_depth_stats_fwd(const float* weights, const float* z_vals, const float* nears, const float* fars, uint32_t N, uint32_t T,
                                      const double* q_levels, uint32_t Q, int normalize, float* quantiles, float* mode, float* std_dev,
                                      double* state, hipStream_t stream) {
    StatLevels lv;
    REQUIRE(T >= 1 && (uint64_t)N * T <= (1ull << 31) && levels_ok(q_levels, Q, lv));
    if (N == 0) return NVSF_OK;
    REQUIRE(weights && z_vals && nears && fars);
    hipLaunchKernelGGL(k_ray_depth_stats_fwd, dim3(cdiv(N, kStatRays)), dim3(kStatBlock), 0, stream, weights, z_vals, nears, fars, N, T, lv, Q,
                       normalize ? 1 : 0, quantiles, mode, std_dev, state);
    return nvsf_launch_status();
}

NVSF_API int nvsf_ray_depth_quantile_bwd(const float* weights, const float* z_vals, const float* nears, const float* fars, uint32_t N,
                                         uint32_t T, const double* q_levels, uint32_t Q, int normalize, const double* state,
                                         const float* grad_quantiles, float* grad_weights, hipStream_t stream) {
    StatLevels lv;
    REQUIRE(T >= 1 && (uint64_t)N * T <= (1ull << 31) && levels_ok(q_levels, Q, lv));
    if (N == 0) return NVSF_OK;
    REQUIRE(weights && z_vals && nears && fars && state && grad_quantiles && grad_weights);
    hipLaunchKernelGGL(k_ray_depth_quantile_bwd, dim3(cdiv(N, kStatRays)), dim3(kStatBlock), 0, stream, weights, z_vals, nears, fars, N, T, lv,
                       Q, normalize ? 1 : 0, state, grad_quantiles, grad_weights);
    return nvsf_launch_status();
}
