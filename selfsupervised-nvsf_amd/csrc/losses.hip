// Per-ray loss terms of the thin training step for gfx950.
//
// Trainer.train_step (nvsf/nerf/trainer.py:187-219, criteria with reduction="none" from main_nvsf.py:205-221, summed at
// trainer.py:540-543) forms the LiDAR terms from five [N] vectors with ~25 elementwise / reduction launches and autograd adds
// ~35 more on the way back; at N = 4096 rays every one of them is a launch latency.  Here the three sums, the masked range and
// the two point clouds the chamfer term compares are ONE single-workgroup launch (deterministic tree sums), and the gradients
// with respect to the rendered image / range are one elementwise launch:
//   gt_int = gt_intensity * gt_raydrop, gt_depth = gt_range * gt_raydrop            (trainer.py:187-189)
//   pred_rd = image[:, 0], pred_int = image[:, 1] * gt_raydrop, pred_depth = depth * gt_raydrop
//   L_depth = sum alpha_d |pred_depth - gt_depth|                                   (L1, trainer.py:193-197)
//   L_raydrop = sum alpha_r (pred_rd - clamp(gt_raydrop, s, 1 - s))^2               (trainer.py:209-215, s = smooth_factor)
//   L_intensity = sum alpha_i (pred_int - gt_int)^2                                 (trainer.py:199-207)
//   pred_pts = rays_d * pred_depth / scale, gt_pts = rays_d * gt_depth / scale      (trainer.py:229-233, inputs of chamfer_3DDist)
// and for the camera batch L_rgb = sum alpha_rgb (image - gt)^2 (trainer.py:491-503).
#include "common.h"

#include <type_traits>

namespace {
constexpr int kBlock = 1024;

// fp32 partials, wave-level final fold; k_camera_loss_fwd promises another order (fp64 partials, serial fold) and keeps its own
// (T = double: the sums under a chosen criterion, same fold)
template <int K, typename T>
__device__ __forceinline__ void block_sums(T (&v)[K], float* __restrict__ out[K]) {
    __shared__ T part[K][kBlock / kWave];
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = wave_sum(v[k]);
        if (lane == 0) part[k][wave] = v[k];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            T s = lane < kBlock / kWave ? part[k][lane] : T(0);
            s = wave_sum(s);
            if (lane == 0) *out[k] = (float)s;
        }
    }
}

__device__ __forceinline__ float sgnf(float e) { return e > 0.0f ? 1.0f : (e < 0.0f ? -1.0f : 0.0f); }  // d|x|/dx, 0 at 0 (torch.abs backward)
struct LidarRay { float m, gd, gi, pd, pr, pi, tr; };  // mask; true range, intensity x mask; rendered range x mask, ray-drop, intensity x mask; smoothed target
__device__ __forceinline__ LidarRay lidar_ray(const float* __restrict__ image, const float* __restrict__ depth, const float* __restrict__ gt_rd,
                                              const float* __restrict__ gt_i, const float* __restrict__ gt_d, uint32_t n, float smooth) {
    const float m = gt_rd[n];
    return {m, gt_d[n] * m, gt_i[n] * m, depth[n] * m, image[2 * (size_t)n], image[2 * (size_t)n + 1] * m, fminf(fmaxf(m, smooth), 1.0f - smooth)};
}
__device__ __forceinline__ void min_max_bits(uint32_t* __restrict__ stats, float v) {  // running (min, max) of the per-ray losses (see below)
    if (stats && v >= 0.0f) { atomicMin(stats, __float_as_uint(v)); atomicMax(stats + 1, __float_as_uint(v)); }
}

// ---- selectable criteria of the per-ray terms: `--depth_loss`, `--raydrop_loss`, `--intensity_loss`, `--rgb_loss` ----------------
// (main_nvsf.py:83-88, 205-222).  crit(prediction, target, kind, param) and its derivative are cd_crit / cd_crit_grad (codes 0 L1, 1 MSE,
// 2 Huber, 3 SmoothL1, 4 BCE-with-logits; sr_crit: the same of a residual, codes 0-3), the one pair every kernel of this file shares.
// The values exist in fp32 (per-ray losses, the patch regulariser, the camera depth term: the calls they always made) and in fp64: the
// sums under a chosen criterion evaluate their terms in fp64 and round once, so they carry less error than the fp32 torch expression
// whatever the criterion.  kCrit = false instantiations are the default criteria (L1 range, MSE elsewhere) as they were.
__device__ __forceinline__ float t_abs(float x) { return fabsf(x); }
__device__ __forceinline__ double t_abs(double x) { return fabs(x); }
__device__ __forceinline__ float t_max0(float x) { return fmaxf(x, 0.0f); }
__device__ __forceinline__ double t_max0(double x) { return fmax(x, 0.0); }
__device__ __forceinline__ float t_exp(float x) { return expf(x); }
__device__ __forceinline__ double t_exp(double x) { return exp(x); }
__device__ __forceinline__ float t_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double t_log1p(double x) { return log1p(x); }
template <typename T>
__device__ __forceinline__ T sr_crit(T e, int kind, T param) {
    const T a = t_abs(e);
    if (kind == 0) return a;                                                       // L1
    if (kind == 1) return e * e;                                                   // MSE
    if (kind == 2) return a <= param ? T(0.5) * e * e : param * (a - T(0.5) * param);  // Huber(delta)
    return a < param ? T(0.5) * e * e / param : a - T(0.5) * param;                    // SmoothL1(beta)
}
__device__ __forceinline__ float sr_crit_grad(float e, int kind, float param) {
    const float sgn = sgnf(e), a = fabsf(e);
    if (kind == 0) return sgn;
    if (kind == 1) return 2.0f * e;
    if (kind == 2) return a <= param ? e : param * sgn;
    return a < param ? e / param : sgn;
}
template <typename T>
__device__ __forceinline__ T cd_crit(T x, T y, int kind, T param) {
    if (kind < 4) return sr_crit(x - y, kind, param);
    return (t_max0(x) - x * y) + t_log1p(t_exp(-t_abs(x)));  // BCEWithLogitsLoss, logits x, targets y
}
__device__ __forceinline__ float cd_crit_grad(float x, float y, int kind, float param) {
    if (kind < 4) return sr_crit_grad(x - y, kind, param);
    return 1.0f / (1.0f + expf(-x)) - y;
}
struct TermCrit { int kind; float param; };
struct LidarCrit { TermCrit d, r, i; };  // range, ray-drop, intensity
// With `--raydrop_loss bce` the reference passes the ray-drop prediction through a sigmoid first (trainer.py:208-209) and then into
// BCEWithLogitsLoss, which applies a second one: matched as written, that is what the reference trains with.
template <typename T>
__device__ __forceinline__ T raydrop_input(T pr, int kind) { return kind == 4 ? T(1) / (T(1) + t_exp(-pr)) : pr; }
template <typename T>
struct LidarTerms { T d, r, i; };  // the three weighted per-ray terms (trainer.py:216-218)
template <typename T>
__device__ __forceinline__ LidarTerms<T> lidar_terms(const LidarRay& t, const LidarCrit& c, float alpha_d, float alpha_r, float alpha_i) {
    return {(T)alpha_d * cd_crit((T)t.pd, (T)t.gd, c.d.kind, (T)c.d.param),
            (T)alpha_r * cd_crit(raydrop_input((T)t.pr, c.r.kind), (T)t.tr, c.r.kind, (T)c.r.param),
            (T)alpha_i * cd_crit((T)t.pi, (T)t.gi, c.i.kind, (T)c.i.param)};
}

template <bool kCrit>
__global__ __launch_bounds__(kBlock) void k_lidar_losses_fwd(const float* __restrict__ image, const float* __restrict__ depth,
                                                             const float* __restrict__ gt_rd, const float* __restrict__ gt_i,
                                                             const float* __restrict__ gt_d, const float* __restrict__ rays_d, uint32_t N,
                                                             float alpha_d, float alpha_r, float alpha_i, float smooth, float scale, LidarCrit crit,
                                                             float* __restrict__ l_depth, float* __restrict__ l_rd, float* __restrict__ l_int,
                                                             float* __restrict__ pred_depth, float* __restrict__ pred_pts,
                                                             float* __restrict__ gt_pts) {
    std::conditional_t<kCrit, double, float> acc[3] = {0, 0, 0};
    for (uint32_t n = threadIdx.x; n < N; n += kBlock) {
        const LidarRay t = lidar_ray(image, depth, gt_rd, gt_i, gt_d, n, smooth);
        if constexpr (kCrit) {
            const LidarTerms<double> v = lidar_terms<double>(t, crit, alpha_d, alpha_r, alpha_i);
            acc[0] += v.d;
            acc[1] += v.r;
            acc[2] += v.i;
        } else {
            acc[0] += alpha_d * fabsf(t.pd - t.gd);
            const float er = t.pr - t.tr, ei = t.pi - t.gi;
            acc[1] += alpha_r * (er * er);
            acc[2] += alpha_i * (ei * ei);
        }
        pred_depth[n] = t.pd;
        if (pred_pts) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float d = rays_d[3 * (size_t)n + k];
                pred_pts[3 * (size_t)n + k] = d * t.pd / scale;
                gt_pts[3 * (size_t)n + k] = d * t.gd / scale;
            }
        }
    }
    float* out[3] = {l_depth, l_rd, l_int};
    block_sums<3>(acc, out);
}

template <bool kCrit>
__global__ __launch_bounds__(256) void k_lidar_losses_bwd(const float* __restrict__ image, const float* __restrict__ depth,
                                                          const float* __restrict__ gt_rd, const float* __restrict__ gt_i,
                                                          const float* __restrict__ gt_d, const float* __restrict__ rays_d, uint32_t N,
                                                          float alpha_d, float alpha_r, float alpha_i, float smooth, float scale, LidarCrit crit,
                                                          const float* __restrict__ g_depth, const float* __restrict__ g_rd,
                                                          const float* __restrict__ g_int, const float* __restrict__ g_pred_depth,
                                                          const float* __restrict__ g_pred_pts, float* __restrict__ grad_image,
                                                          float* __restrict__ grad_depth) {
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= N) return;
    const float gD = g_depth ? *g_depth : 0.0f, gR = g_rd ? *g_rd : 0.0f, gI = g_int ? *g_int : 0.0f;
    const LidarRay t = lidar_ray(image, depth, gt_rd, gt_i, gt_d, n, smooth);
    float gpd, gpr, gpi;  // gradients of the masked range, the ray-drop channel, the masked intensity
    if constexpr (kCrit) {
        gpd = gD * alpha_d * cd_crit_grad(t.pd, t.gd, crit.d.kind, crit.d.param);
        const float x = raydrop_input(t.pr, crit.r.kind);
        float dr = cd_crit_grad(x, t.tr, crit.r.kind, crit.r.param);
        if (crit.r.kind == 4) dr *= x * (1.0f - x);  // through the first sigmoid
        gpr = gR * alpha_r * dr;
        gpi = gI * alpha_i * cd_crit_grad(t.pi, t.gi, crit.i.kind, crit.i.param);
    } else {
        gpd = gD * alpha_d * sgnf(t.pd - t.gd);
        gpr = gR * alpha_r * 2.0f * (t.pr - t.tr);
        gpi = gI * alpha_i * 2.0f * (t.pi - t.gi);
    }
    if (g_pred_depth) gpd += g_pred_depth[n];
    if (g_pred_pts) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) s += g_pred_pts[3 * (size_t)n + k] / scale * rays_d[3 * (size_t)n + k];
        gpd += s;
    }
    grad_depth[n] = gpd * t.m;
    grad_image[2 * (size_t)n] = gpr;
    grad_image[2 * (size_t)n + 1] = gpi * t.m;
}

// the colour term sum alpha crit(a, b) (trainer.py:503); kCrit = false: MSE
template <bool kCrit>
__global__ __launch_bounds__(kBlock) void k_mse_sum_fwd(const float* __restrict__ a, const float* __restrict__ b, uint32_t n, float alpha,
                                                        TermCrit crit, float* __restrict__ out) {
    std::conditional_t<kCrit, double, float> acc[1] = {0};
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
        if constexpr (kCrit) {
            acc[0] += (double)alpha * cd_crit((double)a[i], (double)b[i], crit.kind, (double)crit.param);
        } else {
            const float e = a[i] - b[i];
            acc[0] += alpha * (e * e);
        }
    }
    float* o[1] = {out};
    block_sums<1>(acc, o);
}

template <bool kCrit>
__global__ __launch_bounds__(256) void k_mse_sum_bwd(const float* __restrict__ a, const float* __restrict__ b, uint32_t n, float alpha,
                                                     TermCrit crit, const float* __restrict__ g, float* __restrict__ grad_a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if constexpr (kCrit) grad_a[i] = *g * alpha * cd_crit_grad(a[i], b[i], crit.kind, crit.param);
    else grad_a[i] = *g * alpha * 2.0f * (a[i] - b[i]);
}

// ---- structural regularisation on LiDAR patches: the `grad_loss` branch of Trainer.train_step (trainer.py:296-470) ----------------
// The batch is num_patch patches of pH x pW range-image pixels in row-major patch order (dataset_utils.py:407-503 draws them so):
// pixel j = (p pH + r) pW + c, inds[j] = h W + w.  With q = depth / scale (metres):
//   grad_x(j) = q(j) - q(j + 1)          for c < pW - 1,   grad_x(r, pW - 1) = grad_x(r, pW - 2)      (trainer.py:340-343, 381-384)
//   grad_y(j) = q(j) - q(j + pW)         for r < pH - 1,   grad_y(pH - 1, c) = grad_y(pH - 2, c)
// for the rendered and the true range alike.  The terms are masked by the true ray-drop channel and by the flatness of the TRUE
// range image around the pixel (trainer.py:386-431): first differences of the whole frame (same padding rule), their absolute second
// differences, mask = |second difference at (h, w)| < 0.05.  loss = alpha sum_j crit(grad_x m_x, gt_grad_x m_x) + the same in y
// (trainer.py:449-458: criterion with reduction "none", summed), crit in {L1, MSE, Huber(delta), SmoothL1(beta)} (main_nvsf.py:204-221);
// the cosine criterion and the Sobel gradients of the same block: sr_cos / sr_tap below.
struct PatchGeom {
    uint32_t pH, pW, H, W;
    float scale;
};

// first difference of the frame's range channel along x at (h, w), in metres, with the reference's padding of the last column
__device__ __forceinline__ float pano_dx(const float* __restrict__ pano, uint32_t stride, uint32_t h, uint32_t w, const PatchGeom& g) {
    const uint32_t ww = w < g.W - 1 ? w : g.W - 2;
    const float* row = pano + (size_t)h * g.W * stride;
    return (row[(size_t)ww * stride] - row[(size_t)(ww + 1) * stride]) / g.scale;
}
__device__ __forceinline__ float pano_dy(const float* __restrict__ pano, uint32_t stride, uint32_t h, uint32_t w, const PatchGeom& g) {
    const uint32_t hh = h < g.H - 1 ? h : g.H - 2;
    return (pano[((size_t)hh * g.W + w) * stride] - pano[((size_t)(hh + 1) * g.W + w) * stride]) / g.scale;
}
// d grad_dir(j) / d q(k) for two pixels of ONE patch (0 where pixel k does not enter the gradient at pixel j):
//   manual differences: grad(j) = q(a) - q(b) with (a, b) = (j, j + step), in the last column / row the pair of the one before;
//   --sobel_grad: F.conv2d(patch, K, padding = 1) (trainer.py:316-328, 367-380): cross-correlation with
//                 Kx = [[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], Ky = Kx^T, zero padding at the PATCH border.
__device__ __forceinline__ float sr_tap(uint32_t rj, uint32_t cj, uint32_t rk, uint32_t ck, int dir, const PatchGeom& g, bool sobel) {
    const int dr = (int)rk - (int)rj, dc = (int)ck - (int)cj;
    if (sobel) {
        if (dr < -1 || dr > 1 || dc < -1 || dc > 1) return 0.0f;
        const int along = dir == 0 ? dc : dr, across = dir == 0 ? dr : dc;
        return (float)along * (across == 0 ? 2.0f : 1.0f);
    }
    if (dir == 0) {
        if (dr != 0) return 0.0f;
        const uint32_t a = cj < g.pW - 1 ? cj : cj - 1;
        return ck == a ? 1.0f : (ck == a + 1 ? -1.0f : 0.0f);
    }
    if (dc != 0) return 0.0f;
    const uint32_t a = rj < g.pH - 1 ? rj : rj - 1;
    return rk == a ? 1.0f : (rk == a + 1 ? -1.0f : 0.0f);
}
// gradient of the patch image q = v / scale at pixel j = (patch base + rj pW + cj)
__device__ __forceinline__ float sr_grad(const float* __restrict__ v, uint32_t base, uint32_t rj, uint32_t cj, int dir, const PatchGeom& g, bool sobel) {
    if (!sobel) {
        uint32_t a, b;
        if (dir == 0) { a = base + rj * g.pW + (cj < g.pW - 1 ? cj : cj - 1); b = a + 1; }
        else { a = base + (rj < g.pH - 1 ? rj : rj - 1) * g.pW + cj; b = a + g.pW; }
        return v[a] / g.scale - v[b] / g.scale;
    }
    float acc = 0.0f;  // row-major over the 3 x 3 window, zero taps skipped
    for (int dr = -1; dr <= 1; ++dr)
        for (int dc = -1; dc <= 1; ++dc) {
            const int r = (int)rj + dr, c = (int)cj + dc;
            if (r < 0 || c < 0 || r >= (int)g.pH || c >= (int)g.pW) continue;
            const float k = sr_tap(rj, cj, (uint32_t)r, (uint32_t)c, dir, g, true);
            if (k != 0.0f) acc += k * (v[base + (uint32_t)r * g.pW + (uint32_t)c] / g.scale);
        }
    return acc;
}
// mask of pixel j in direction dir: true ray-drop channel x flatness of the TRUE frame at the pixel (trainer.py:388-439)
__device__ __forceinline__ float sr_mask(const float* __restrict__ gt_rd, const long long* __restrict__ inds, const float* __restrict__ pano,
                                         uint32_t pano_stride, uint32_t j, int dir, const PatchGeom& g) {
    const uint32_t h = (uint32_t)(inds[j] / (long long)g.W), w = (uint32_t)(inds[j] % (long long)g.W);
    float second;
    if (dir == 0) {
        const uint32_t ww = w < g.W - 1 ? w : g.W - 2;  // padding of the second difference's last column
        second = fabsf(pano_dx(pano, pano_stride, h, ww, g)) - fabsf(pano_dx(pano, pano_stride, h, ww + 1, g));
    } else {
        const uint32_t hh = h < g.H - 1 ? h : g.H - 2;
        second = fabsf(pano_dy(pano, pano_stride, hh, w, g)) - fabsf(pano_dy(pano, pano_stride, hh + 1, w, g));
    }
    return gt_rd[j] * (fabsf(second) < 0.05f ? 1.0f : 0.0f);
}
struct SrTerm { float u, v, m; };  // masked gradient of the rendered range, of the true range, the mask
__device__ __forceinline__ SrTerm sr_term(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ gt_rd,
                                          const long long* __restrict__ inds, const float* __restrict__ pano, uint32_t pano_stride, uint32_t j,
                                          int dir, const PatchGeom& g, bool sobel) {
    const uint32_t area = g.pH * g.pW, base = j / area * area, rj = (j - base) / g.pW, cj = (j - base) % g.pW;
    SrTerm t;
    t.m = sr_mask(gt_rd, inds, pano, pano_stride, j, dir, g);
    t.u = sr_grad(pred, base, rj, cj, dir, g, sobel) * t.m;
    t.v = sr_grad(gt, base, rj, cj, dir, g, sobel) * t.m;
    return t;
}

// criterion 4, `--depth_grad_loss cos` (main_nvsf.py:211, trainer.py:442-452): per patch and direction cos = <u, v> / (max(|u|, eps)
// max(|v|, eps)) over the patch's pH pW masked gradients (torch.nn.CosineSimilarity(dim = 1, eps = 1e-8) on the flattened patch), and
// (1 - cos) expanded over the patch and summed: loss = alpha pH pW sum_patches (1 - cos_x) + (1 - cos_y).
// patch_stats [P, 6] = (<u,v>, <u,u>, <v,v>) for x, then for y -- written by the forward, read by the backward.
constexpr float kCosEps = 1e-8f;
__device__ __forceinline__ float sr_cos(const float* __restrict__ st) {
    return st[0] / (fmaxf(sqrtf(st[1]), kCosEps) * fmaxf(sqrtf(st[2]), kCosEps));
}

__global__ __launch_bounds__(kBlock) void k_lidar_grad_loss_fwd(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                const float* __restrict__ gt_rd, const long long* __restrict__ inds,
                                                                const float* __restrict__ pano, uint32_t pano_stride, uint32_t N, PatchGeom g,
                                                                int kind, float param, float alpha, int sobel, float* __restrict__ patch_stats,
                                                                float* __restrict__ loss) {
    float acc[1] = {0.0f};
    if (kind < 4) {
        for (uint32_t j = threadIdx.x; j < N; j += kBlock) {
            const SrTerm x = sr_term(pred, gt, gt_rd, inds, pano, pano_stride, j, 0, g, sobel != 0);
            const SrTerm y = sr_term(pred, gt, gt_rd, inds, pano, pano_stride, j, 1, g, sobel != 0);
            acc[0] += alpha * (sr_crit(x.u - x.v, kind, param) + sr_crit(y.u - y.v, kind, param));
        }
    } else {
        const uint32_t area = g.pH * g.pW;
        for (uint32_t p = threadIdx.x; p < N / area; p += kBlock) {
            float st[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            for (uint32_t j = p * area; j < (p + 1) * area; ++j)
                for (int dir = 0; dir < 2; ++dir) {
                    const SrTerm t = sr_term(pred, gt, gt_rd, inds, pano, pano_stride, j, dir, g, sobel != 0);
                    st[3 * dir] += t.u * t.v;
                    st[3 * dir + 1] += t.u * t.u;
                    st[3 * dir + 2] += t.v * t.v;
                }
            for (int k = 0; k < 6; ++k) patch_stats[6 * (size_t)p + k] = st[k];
            acc[0] += alpha * (float)area * ((1.0f - sr_cos(st)) + (1.0f - sr_cos(st + 3)));
        }
    }
    float* o[1] = {loss};
    block_sums<1>(acc, o);
}

// d loss / d pred(k): pixel k enters the gradients of the pixels of its 3 x 3 neighbourhood inside its patch (sr_tap)
__global__ __launch_bounds__(256) void k_lidar_grad_loss_bwd(const float* __restrict__ pred, const float* __restrict__ gt,
                                                             const float* __restrict__ gt_rd, const long long* __restrict__ inds,
                                                             const float* __restrict__ pano, uint32_t pano_stride, uint32_t N, PatchGeom g,
                                                             int kind, float param, float alpha, int sobel, const float* __restrict__ patch_stats,
                                                             const float* __restrict__ g_loss, float* __restrict__ grad_pred) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= N) return;
    const uint32_t area = g.pH * g.pW, p = k / area, base = p * area, rk = (k - base) / g.pW, ck = (k - base) % g.pW;
    float sum = 0.0f;
    for (int dr = -1; dr <= 1; ++dr)
        for (int dc = -1; dc <= 1; ++dc) {
            const int r = (int)rk + dr, c = (int)ck + dc;
            if (r < 0 || c < 0 || r >= (int)g.pH || c >= (int)g.pW) continue;
            const uint32_t j = base + (uint32_t)r * g.pW + (uint32_t)c;
            for (int dir = 0; dir < 2; ++dir) {
                const float tap = sr_tap((uint32_t)r, (uint32_t)c, rk, ck, dir, g, sobel != 0);
                if (tap == 0.0f) continue;
                const SrTerm t = sr_term(pred, gt, gt_rd, inds, pano, pano_stride, j, dir, g, sobel != 0);
                float d;  // d loss / d u(j)
                if (kind < 4) {
                    d = alpha * sr_crit_grad(t.u - t.v, kind, param);
                } else {
                    const float* st = patch_stats + 6 * (size_t)p + 3 * dir;
                    const float nu_raw = sqrtf(st[1]), nu = fmaxf(nu_raw, kCosEps), nv = fmaxf(sqrtf(st[2]), kCosEps);
                    float dcos = t.v / (nu * nv);
                    if (nu_raw > kCosEps) dcos -= st[0] / (nu * nu * nv) * (t.u / nu_raw);
                    d = -alpha * (float)area * dcos;
                }
                sum += tap * d * t.m;
            }
        }
    grad_pred[k] = *g_loss * sum / g.scale;
}

// ---- the two camera terms of a ray batch: trainer.py:491-518 ---------------------------------------------------------------------
//   L_rgb = sum alpha_rgb (image - gt_rgb)^2 over rays and channels
//   gt = min(gt_m scale, max_depth), pred = min(depth, max_depth) (a ray the cap changes gets no gradient: the reference assigns into the
//   tensor), mask = gt > 0, L_depth = sum alpha_rd crit(pred mask, gt mask) over ALL rays (a masked ray gives crit(0, 0): log 2 under
//   BCE-with-logits).  Per-ray terms are fp32; every thread adds its terms in index order into an fp64 partial, a wave folds its lanes in
//   a fixed butterfly and thread 0 the 16 wave partials in wave order: no atomic, two runs give the same bits.
struct CamDepth { float x, y, m; bool capped; };  // masked prediction, masked truth, mask, prediction above the cap
__device__ __forceinline__ CamDepth cam_depth(float depth, float gt_m, float scale, float max_depth) {
    CamDepth t;
    float g = gt_m * scale;
    g = g > max_depth ? max_depth : g;
    t.capped = depth > max_depth;
    const float p = t.capped ? max_depth : depth;
    t.m = g > 0.0f ? 1.0f : 0.0f;
    t.x = p * t.m;
    t.y = g * t.m;
    return t;
}

// kCrit: the colour term under `--rgb_loss` (rgb) instead of MSE
template <bool kCrit>
__global__ __launch_bounds__(kBlock) void k_camera_loss_fwd(const float* __restrict__ image, const float* __restrict__ gt_rgb,
                                                            const float* __restrict__ depth, const float* __restrict__ gt_m, uint32_t N,
                                                            float alpha_rgb, float alpha_rd, float scale, float max_depth, int kind, float param,
                                                            TermCrit rgb, float* __restrict__ l_rgb, float* __restrict__ l_depth) {
    __shared__ double part[2][kBlock / kWave];
    double acc[2] = {0.0, 0.0};
    for (uint32_t i = threadIdx.x; i < 3 * N; i += kBlock) {
        if constexpr (kCrit) {
            acc[0] += (double)alpha_rgb * cd_crit((double)image[i], (double)gt_rgb[i], rgb.kind, (double)rgb.param);
        } else {
            const float e = image[i] - gt_rgb[i];
            acc[0] += (double)(alpha_rgb * (e * e));
        }
    }
    for (uint32_t n = threadIdx.x; n < N; n += kBlock) {
        const CamDepth t = cam_depth(depth[n], gt_m[n], scale, max_depth);
        acc[1] += (double)(alpha_rd * cd_crit(t.x, t.y, kind, param));
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        acc[k] = wave_sum(acc[k]);
        if (lane_id() == 0) part[k][threadIdx.x >> 6] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r[2] = {0.0, 0.0};
        for (int w = 0; w < kBlock / kWave; ++w) { r[0] += part[0][w]; r[1] += part[1][w]; }
        *l_rgb = (float)r[0];
        *l_depth = (float)r[1];
    }
}

template <bool kCrit>
__global__ __launch_bounds__(256) void k_camera_loss_bwd(const float* __restrict__ image, const float* __restrict__ gt_rgb,
                                                         const float* __restrict__ depth, const float* __restrict__ gt_m, uint32_t N,
                                                         float alpha_rgb, float alpha_rd, float scale, float max_depth, int kind, float param,
                                                         TermCrit rgb, const float* __restrict__ g_rgb, const float* __restrict__ g_depth,
                                                         float* __restrict__ grad_image, float* __restrict__ grad_depth) {
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= N) return;
    const float gR = g_rgb ? *g_rgb : 0.0f, gD = g_depth ? *g_depth : 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const size_t i = 3 * (size_t)n + k;
        if constexpr (kCrit) grad_image[i] = gR * alpha_rgb * cd_crit_grad(image[i], gt_rgb[i], rgb.kind, rgb.param);
        else grad_image[i] = gR * alpha_rgb * 2.0f * (image[i] - gt_rgb[i]);
    }
    const CamDepth t = cam_depth(depth[n], gt_m[n], scale, max_depth);
    grad_depth[n] = (t.capped || t.m == 0.0f) ? 0.0f : gD * alpha_rd * cd_crit_grad(t.x, t.y, kind, param);
}

// ---- error map of the pixel sampler (trainer.py:552-630) -----------------------------------------------------------------------
// per-ray LiDAR loss = alpha_d |.| + alpha_r (.)^2 + alpha_i (.)^2 (trainer.py:213-216, reduction "none") / per-ray camera loss =
// sum over channels of alpha_rgb (.)^2 (trainer.py:598); stats[0 .. 1] = (min, max) over the rays as ordered unsigned bit patterns
// (the losses are >= 0), to be initialised to (0x7f800000, 0) by the caller
__global__ __launch_bounds__(256) void k_lidar_ray_losses(const float* __restrict__ image, const float* __restrict__ depth, const float* __restrict__ gt_rd,
                                                          const float* __restrict__ gt_i, const float* __restrict__ gt_d, uint32_t N, float alpha_d,
                                                          float alpha_r, float alpha_i, float smooth, float* __restrict__ out, uint32_t* __restrict__ stats) {
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= N) return;
    const LidarRay t = lidar_ray(image, depth, gt_rd, gt_i, gt_d, n, smooth);
    const float er = t.pr - t.tr, ei = t.pi - t.gi;
    const float v = alpha_d * fabsf(t.pd - t.gd) + alpha_r * (er * er) + alpha_i * (ei * ei);
    out[n] = v;
    min_max_bits(stats, v);
}
__global__ __launch_bounds__(256) void k_mse_rows(const float* __restrict__ a, const float* __restrict__ b, uint32_t N, uint32_t C, float alpha,
                                                  float* __restrict__ out, uint32_t* __restrict__ stats) {
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= N) return;
    float v = 0.0f;
    for (uint32_t k = 0; k < C; ++k) {
        const float e = a[(size_t)n * C + k] - b[(size_t)n * C + k];
        v += alpha * (e * e);
    }
    out[n] = v;
    min_max_bits(stats, v);
}
// error = (loss - min) / (max - min + eps) * 999 + 1; cell = (floor(h eH / H), floor(w eW / W)); map[cell] = 0.1 map[cell] + 0.9 error.
// Several rays of a batch may fall into one cell: the reference's indexed assignment keeps an unspecified one of them (each computed
// from the OLD map value); here the ray with the LARGEST index wins (what a sequential execution of the assignment gives): pass 1
// leaves max(ray index + 1) per touched cell in `owner` (zero on entry), pass 2 lets that ray write and clears the slot again.
__device__ __forceinline__ size_t error_map_cell(long long ind, uint32_t W, uint32_t eH, uint32_t eW, float sh, float sw) {
    const uint32_t h = (uint32_t)(ind / (long long)W), w = (uint32_t)(ind % (long long)W);
    const uint32_t ch = (uint32_t)((float)h * sh), cw = (uint32_t)((float)w * sw);
    return (size_t)(ch < eH ? ch : eH - 1) * eW + (cw < eW ? cw : eW - 1);  // (a caller-side scale that rounds up: stay inside the map)
}
__global__ __launch_bounds__(256) void k_error_map_claim(const long long* __restrict__ inds, uint32_t N, uint32_t W, uint32_t eH, uint32_t eW,
                                                         float sh, float sw, uint32_t* __restrict__ owner) {
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= N) return;
    atomicMax(owner + error_map_cell(inds[n], W, eH, eW, sh, sw), n + 1u);
}
__global__ __launch_bounds__(256) void k_error_map_write(const float* __restrict__ loss, const long long* __restrict__ inds, uint32_t N,
                                                         uint32_t W, uint32_t eH, uint32_t eW, float sh, float sw, const uint32_t* __restrict__ stats,
                                                         uint32_t* __restrict__ owner, float* __restrict__ map) {
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= N) return;
    const size_t cell = error_map_cell(inds[n], W, eH, eW, sh, sw);
    if (owner[cell] != n + 1u) return;
    const float lo = __uint_as_float(stats[0]), hi = __uint_as_float(stats[1]);
    float e = (loss[n] - lo) / (hi - lo + 1.1920928955078125e-07f);  // torch.finfo().eps
    e = e * (1000.0f - 1.0f) + 1.0f;
    map[cell] = 0.1f * map[cell] + 0.9f * e;
    owner[cell] = 0u;
}

// The per-ray losses under the selectable criteria.  BCE against a target outside [0, 1] (the range term) can be negative, which the
// unsigned bit-pattern order of min_max_bits does not cover: here ONE workgroup walks the rays and folds (min, max) in a fixed tree of
// fminf / fmaxf, then WRITES them as the float bit patterns k_error_map_write reads (nothing to initialise, no atomics).
__device__ __forceinline__ void block_min_max(float lo, float hi, uint32_t* __restrict__ stats) {
    __shared__ float part[2][kBlock / kWave];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if (lane_id() == 0) { part[0][threadIdx.x >> 6] = lo; part[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0 && stats) {
        for (int w = 1; w < kBlock / kWave; ++w) { lo = fminf(lo, part[0][w]); hi = fmaxf(hi, part[1][w]); }
        stats[0] = __float_as_uint(lo);
        stats[1] = __float_as_uint(hi);
    }
}
__global__ __launch_bounds__(kBlock) void k_lidar_ray_losses_crit(const float* __restrict__ image, const float* __restrict__ depth,
                                                                  const float* __restrict__ gt_rd, const float* __restrict__ gt_i,
                                                                  const float* __restrict__ gt_d, uint32_t N, float alpha_d, float alpha_r,
                                                                  float alpha_i, float smooth, LidarCrit crit, float* __restrict__ out,
                                                                  uint32_t* __restrict__ stats) {
    float lo = INFINITY, hi = -INFINITY;
    for (uint32_t n = threadIdx.x; n < N; n += kBlock) {
        const LidarTerms<float> t = lidar_terms<float>(lidar_ray(image, depth, gt_rd, gt_i, gt_d, n, smooth), crit, alpha_d, alpha_r, alpha_i);
        const float v = t.d + t.r + t.i;
        out[n] = v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    block_min_max(lo, hi, stats);
}
__global__ __launch_bounds__(kBlock) void k_crit_rows(const float* __restrict__ a, const float* __restrict__ b, uint32_t N, uint32_t C, float alpha,
                                                      TermCrit crit, float* __restrict__ out, uint32_t* __restrict__ stats) {
    float lo = INFINITY, hi = -INFINITY;
    for (uint32_t n = threadIdx.x; n < N; n += kBlock) {
        float v = 0.0f;
        for (uint32_t k = 0; k < C; ++k) v += alpha * cd_crit(a[(size_t)n * C + k], b[(size_t)n * C + k], crit.kind, crit.param);
        out[n] = v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    block_min_max(lo, hi, stats);
}

// ---- line-of-sight loss of Urban Radiance Fields (`--use_urf_loss`, trainer.py:276-294) over weights / z_vals [N, T] ---------------
//   lo = g - eps, hi = g + eps (one fp32 rounding each, as the reference's fp32 tensors), near = lo < z < hi, empty = z < lo or z > hi
//   r = exp(-d^2 / (2 sigma^2)), sigma = eps / 3, d = near ? z - g : 0;  E = max r over EVERY element (distr.max() / c: the constant
//   c = 1 / (sigma sqrt(2 pi)) cancels in distr / distr.max());  n = #{g > 0}
//   loss = 0.1 sum (empty w)^2 / n + 0.1 sum (near w - near r / E)^2 / n
// A pure stream (w and z once forward; w, z and the gradient backward): 16-byte loads along the flat array, grid-stride from the CU
// count.  An element that is not near has r = 1, so E = 1 as soon as one exists; a launch in which EVERY element is near has
// E = exp(-min d^2 / (2 sigma^2)) < 1 unless a sample sits on g.  One pass covers both: every thread sums (w - r)^2 (the near term if
// E = 1) next to w^2, w r and r^2, from which the fold forms sum (w - r / E)^2 = sum w^2 - 2 sum w r / E + sum r^2 / E^2 in the
// all-near case (fp64: the cancellation costs ~1e-16 of sum w^2 + sum r^2 / E^2).  Per-element terms and partials are fp64, a wave folds
// by a fixed butterfly, a block its waves in order, the second launch the blocks in order: no atomics, two runs give the same bits.
constexpr int kUrfBlock = 256, kUrfMaxBlocks = 1024, kUrfSlots = 8;  // partials per block: 5 sums, min |d|, #not near, #{g > 0}
struct UrfAcc { double se, sn, sww, swr, srr, dmin; uint32_t far; };
struct UrfBand { bool near, empty; double d; };
__device__ __forceinline__ UrfBand urf_band(float z, float g, float eps) {
    const float lo = __fsub_rn(g, eps), hi = __fadd_rn(g, eps);
    UrfBand b;
    b.near = z > lo && z < hi;
    b.empty = z < lo || z > hi;
    b.d = (double)z - (double)g;
    return b;
}
__device__ __forceinline__ void urf_elem(float w, float z, float g, float eps, double inv2s2, UrfAcc& a) {
    const UrfBand b = urf_band(z, g, eps);
    if (b.near) {
        const double r = exp(-(b.d * b.d * inv2s2)), t = (double)w - r;
        a.sn += t * t;
        a.sww += (double)w * (double)w;
        a.swr += (double)w * r;
        a.srr += r * r;
        a.dmin = fmin(a.dmin, fabs(b.d));
    } else {
        a.far = 1u;
        if (b.empty) a.se += (double)w * (double)w;
    }
}
__device__ __forceinline__ double urf_grad_elem(float w, float z, float g, float eps, double inv2s2, double E) {
    const UrfBand b = urf_band(z, g, eps);
    if (b.near) return (double)w - exp(-(b.d * b.d * inv2s2)) / E;
    return b.empty ? (double)w : 0.0;
}
// kVec: both arrays 16-byte aligned -> float4 chunks of the flat array (whatever T: a chunk may span rows), the last total % 4 elements
// one by one; otherwise every element on its own.  kRows4: T % 4 == 0, a chunk lies in one row.
template <bool kVec, bool kRows4>
__global__ __launch_bounds__(kUrfBlock) void k_urf_partials(const float* __restrict__ w, const float* __restrict__ z, const float* __restrict__ g,
                                                            uint32_t N, uint32_t T, float eps, double inv2s2, double* __restrict__ partials) {
    __shared__ double part[kUrfSlots][kUrfBlock / kWave];
    const uint32_t total = N * T, tid = blockIdx.x * kUrfBlock + threadIdx.x, stride = gridDim.x * kUrfBlock;  // total <= 2^31 (launcher)
    UrfAcc a = {0.0, 0.0, 0.0, 0.0, 0.0, INFINITY, 0u};
    const uint32_t chunks = kVec ? total / 4 : 0;
    for (uint32_t c = tid; c < chunks; c += stride) {
        const float4 w4 = reinterpret_cast<const float4*>(w)[c], z4 = reinterpret_cast<const float4*>(z)[c];
        const float wv[4] = {w4.x, w4.y, w4.z, w4.w}, zv[4] = {z4.x, z4.y, z4.z, z4.w};
        if constexpr (kRows4) {
            const float gr = g[(4 * c) / T];
#pragma unroll
            for (int j = 0; j < 4; ++j) urf_elem(wv[j], zv[j], gr, eps, inv2s2, a);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) urf_elem(wv[j], zv[j], g[(4 * c + j) / T], eps, inv2s2, a);
        }
    }
    for (uint32_t e = 4 * chunks + tid; e < total; e += stride) urf_elem(w[e], z[e], g[e / T], eps, inv2s2, a);
    uint32_t valid = 0;
    for (uint32_t r = tid; r < N; r += stride) valid += g[r] > 0.0f ? 1u : 0u;
    double v[kUrfSlots] = {a.se, a.sn, a.sww, a.swr, a.srr, a.dmin, (double)a.far, (double)valid};  // counts < 2^53: exact
#pragma unroll
    for (int k = 0; k < kUrfSlots; ++k) {
        if (k == 5) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v[k] = fmin(v[k], __shfl_xor(v[k], o, 64));
        } else {
            v[k] = wave_sum(v[k]);
        }
        if (lane_id() == 0) part[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < kUrfSlots) {
        const int k = threadIdx.x;
        double s = part[k][0];
        for (int q = 1; q < kUrfBlock / kWave; ++q) s = k == 5 ? fmin(s, part[k][q]) : s + part[k][q];
        partials[(size_t)blockIdx.x * kUrfSlots + k] = s;
    }
}
// folds the blocks' partials in block order; state = (E, n) for the backward
__global__ __launch_bounds__(kWave) void k_urf_fold(const double* __restrict__ partials, uint32_t blocks, double inv2s2, float* __restrict__ loss,
                                                    double* __restrict__ state) {
    double v[kUrfSlots];
#pragma unroll
    for (int k = 0; k < kUrfSlots; ++k) v[k] = k == 5 ? (double)INFINITY : 0.0;
    for (uint32_t b = threadIdx.x; b < blocks; b += kWave) {
#pragma unroll
        for (int k = 0; k < kUrfSlots; ++k) {
            const double p = partials[(size_t)b * kUrfSlots + k];
            v[k] = k == 5 ? fmin(v[k], p) : v[k] + p;
        }
    }
#pragma unroll
    for (int k = 0; k < kUrfSlots; ++k) {
        if (k == 5) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v[k] = fmin(v[k], __shfl_xor(v[k], o, 64));
        } else {
            v[k] = wave_sum(v[k]);
        }
    }
    if (threadIdx.x != 0) return;
    const double n = v[7];
    double E = 1.0, near = v[1];
    if (v[6] == 0.0 && v[5] < (double)INFINITY) {  // every element is near: distr.max() is the sample closest to its g
        E = exp(-(v[5] * v[5] * inv2s2));
        near = v[2] - 2.0 * v[3] / E + v[4] / (E * E);
    }
    *loss = (float)(0.1 * (v[0] / n) + 0.1 * (near / n));  // n = 0: what IEEE division gives, as the torch expression
    state[0] = E;
    state[1] = n;
}
template <bool kVec, bool kRows4>
__global__ __launch_bounds__(kUrfBlock) void k_urf_bwd(const float* __restrict__ w, const float* __restrict__ z, const float* __restrict__ g,
                                                       uint32_t N, uint32_t T, float eps, double inv2s2, const double* __restrict__ state,
                                                       const float* __restrict__ g_loss, float* __restrict__ grad_w) {
    const uint32_t total = N * T, tid = blockIdx.x * kUrfBlock + threadIdx.x, stride = gridDim.x * kUrfBlock;  // total <= 2^31 (launcher)
    const double E = state[0], k = (double)*g_loss * 0.2 / state[1];
    const uint32_t chunks = kVec ? total / 4 : 0;
    for (uint32_t c = tid; c < chunks; c += stride) {
        const float4 w4 = reinterpret_cast<const float4*>(w)[c], z4 = reinterpret_cast<const float4*>(z)[c];
        const float wv[4] = {w4.x, w4.y, w4.z, w4.w}, zv[4] = {z4.x, z4.y, z4.z, z4.w};
        float o[4];
        if constexpr (kRows4) {
            const float gr = g[(4 * c) / T];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (float)(k * urf_grad_elem(wv[j], zv[j], gr, eps, inv2s2, E));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (float)(k * urf_grad_elem(wv[j], zv[j], g[(4 * c + j) / T], eps, inv2s2, E));
        }
        reinterpret_cast<float4*>(grad_w)[c] = make_float4(o[0], o[1], o[2], o[3]);
    }
    for (uint32_t e = 4 * chunks + tid; e < total; e += stride) grad_w[e] = (float)(k * urf_grad_elem(w[e], z[e], g[e / T], eps, inv2s2, E));
}

// ---- distortion loss of mip-NeRF 360 (Barron et al. 2022, eq. 15) over weights / z_vals [N, T]: `distortion_loss` ------------------
// Per ray, with the compositor's intervals (uniform.hip: delta_i = z_{i+1} - z_i, delta_{T-1} = (far - near) / T), R = far - near,
//   m_i = (z_i + delta_i / 2 - near) / R,  d_i = delta_i / R                              (normalised midpoint and width)
//   ray = sum_i sum_j w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i,   loss = alpha sum_n ray_n / N
// z is non-decreasing, so the midpoints are, and the double sum is 2 sum_i w_i (m_i W_<i - M_<i) with the exclusive prefix sums of w and
// w m: one scan per ray.  d ray / d w_k = 2 [m_k (W_<k - W_>k) - M_<k + M_>k] + 2/3 w_k d_k with the suffix sums from the row totals
// the forward leaves in `state`, so the backward is one pass as well.  m W - M cancels (a ray whose weight sits in a few samples at
// the far end loses 2e-5 of the loss in fp32): every term and both scans are fp64, rounded once on store.
// One wave per ray, four rays per workgroup, lane = sample in tiles of 64 (4-byte loads, any alignment; z_{i+1} is a second load shifted
// by one); the running totals cross the tiles in a wave-uniform pair.  A ray whose R is not finite or not > 0 (a camera ray that misses
// the box) gives 0 and a zero gradient row.  No atomics: per-workgroup partials, one fold in block order, two runs give the same bits.
constexpr int kDistBlock = 256, kDistRays = kDistBlock / kWave;
struct DistRay { double near, R, last; bool ok; };  // last = delta_{T-1} = R / T
__device__ __forceinline__ DistRay dist_ray(const float* __restrict__ nears, const float* __restrict__ fars, uint32_t n, uint32_t T) {
    DistRay r;
    r.near = (double)nears[n];
    r.R = (double)fars[n] - r.near;
    r.ok = r.R > 0.0 && r.R < (double)INFINITY;
    r.last = r.R / (double)T;
    return r;
}
// one tile of a row: this lane's weight, midpoint and width (zero past T) and the prefix sums of w and w m over the row up to the lane
struct DistTile { double w, m, d, w_lt, m_lt, w_le, m_le; bool valid; };
__device__ __forceinline__ DistTile dist_tile(const float* __restrict__ w, const float* __restrict__ z, uint32_t base, uint32_t T,
                                              const DistRay& r, double& run_w, double& run_m) {
    const uint32_t i = base + (uint32_t)lane_id();
    DistTile t;
    t.valid = i < T;
    t.w = t.m = t.d = 0.0;
    double wm = 0.0;
    if (t.valid) {
        const double zi = (double)z[i], delta = i + 1 < T ? (double)z[i + 1] - zi : r.last;
        t.w = (double)w[i];
        t.m = (zi + delta / 2.0 - r.near) / r.R;
        t.d = delta / r.R;
        wm = t.w * t.m;
    }
    const double sw = wave_scan_add_f64(t.w), sm = wave_scan_add_f64(wm);
    double ew = __shfl_up(sw, 1, 64), em = __shfl_up(sm, 1, 64);
    if (lane_id() == 0) ew = em = 0.0;
    t.w_lt = run_w + ew;
    t.m_lt = run_m + em;
    t.w_le = run_w + sw;
    t.m_le = run_m + sm;
    run_w += wave_last_f64(sw);
    run_m += wave_last_f64(sm);
    return t;
}
__global__ __launch_bounds__(kDistBlock) void k_distortion_fwd(const float* __restrict__ weights, const float* __restrict__ z_vals,
                                                               const float* __restrict__ nears, const float* __restrict__ fars, uint32_t N,
                                                               uint32_t T, float* __restrict__ ray_loss, double* __restrict__ state,
                                                               double* __restrict__ partials) {
    __shared__ double part[kDistRays];
    const uint32_t wave = threadIdx.x >> 6, n = blockIdx.x * kDistRays + wave;
    double ray = 0.0;  // whole waves take each branch: n and the ray's range are wave-uniform
    if (n < N) {
        const DistRay r = dist_ray(nears, fars, n, T);
        double run_w = 0.0, run_m = 0.0;
        if (r.ok) {
            const float* w = weights + (size_t)n * T;
            const float* z = z_vals + (size_t)n * T;
            double pair = 0.0, self = 0.0;
            for (uint32_t base = 0; base < T; base += kWave) {
                const DistTile t = dist_tile(w, z, base, T, r, run_w, run_m);
                if (t.valid) {
                    pair += t.w * (t.m * t.w_lt - t.m_lt);
                    self += t.w * t.w * t.d;
                }
            }
            ray = 2.0 * wave_sum(pair) + wave_sum(self) / 3.0;
        }
        if (lane_id() == 0) {
            if (ray_loss) ray_loss[n] = (float)ray;
            state[2 * (size_t)n] = run_w;
            state[2 * (size_t)n + 1] = run_m;
        }
    }
    if (lane_id() == 0) part[wave] = ray;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = part[0];
        for (int q = 1; q < kDistRays; ++q) s += part[q];
        partials[blockIdx.x] = s;
    }
}
// folds the workgroups' partials: every thread its blocks in order, a wave by a fixed butterfly, thread 0 the waves in order
__global__ __launch_bounds__(kBlock) void k_distortion_fold(const double* __restrict__ partials, uint32_t blocks, double scale, float* __restrict__ loss) {
    __shared__ double part[kBlock / kWave];
    double s = 0.0;
    for (uint32_t b = threadIdx.x; b < blocks; b += kBlock) s += partials[b];
    s = wave_sum(s);
    if (lane_id() == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = part[0];
        for (int q = 1; q < kBlock / kWave; ++q) r += part[q];
        *loss = (float)(r * scale);
    }
}
__global__ __launch_bounds__(kDistBlock) void k_distortion_bwd(const float* __restrict__ weights, const float* __restrict__ z_vals,
                                                               const float* __restrict__ nears, const float* __restrict__ fars, uint32_t N,
                                                               uint32_t T, double scale, const double* __restrict__ state,
                                                               const float* __restrict__ g_loss, float* __restrict__ grad_w) {
    const uint32_t n = blockIdx.x * kDistRays + (threadIdx.x >> 6);
    if (n >= N) return;
    const DistRay r = dist_ray(nears, fars, n, T);
    float* out = grad_w + (size_t)n * T;
    if (!r.ok) {
        for (uint32_t i = (uint32_t)lane_id(); i < T; i += kWave) out[i] = 0.0f;
        return;
    }
    const float* w = weights + (size_t)n * T;
    const float* z = z_vals + (size_t)n * T;
    const double k = (double)*g_loss * scale, w_tot = state[2 * (size_t)n], m_tot = state[2 * (size_t)n + 1];
    double run_w = 0.0, run_m = 0.0;
    for (uint32_t base = 0; base < T; base += kWave) {
        const DistTile t = dist_tile(w, z, base, T, r, run_w, run_m);
        const double w_gt = w_tot - t.w_le, m_gt = m_tot - t.m_le;
        const double g = 2.0 * (t.m * (t.w_lt - w_gt) - t.m_lt + m_gt) + 2.0 / 3.0 * (t.w * t.d);
        if (t.valid) out[base + (uint32_t)lane_id()] = (float)(k * g);
    }
}
}  // namespace

// criterion codes 0 .. 4; Huber (2) and SmoothL1 (3) need their positive parameter
static inline bool criterion_ok(int kind, float param) { return kind >= 0 && kind <= 4 && (kind < 2 || kind == 4 || param > 0.0f); }
static inline bool patch_geom_ok(uint32_t N, uint32_t pH, uint32_t pW, uint32_t H, uint32_t W, float scale) {
    return pH >= 2 && pW >= 2 && N % (pH * pW) == 0 && H >= 2 && W >= 2 && scale != 0.0f;
}

// the entries with selectable criteria share their launchers with the default ones: crit == nullptr is the default instantiation
static inline bool lidar_crit_ok(const LidarCrit& c) {
    return criterion_ok(c.d.kind, c.d.param) && criterion_ok(c.r.kind, c.r.param) && criterion_ok(c.i.kind, c.i.param);
}

static int lidar_losses_fwd(const float* image_lidar, const float* depth_lidar, const float* gt_raydrop, const float* gt_intensity,
                            const float* gt_range, const float* rays_d, uint32_t N, float alpha_d, float alpha_r, float alpha_i,
                            float smooth_factor, float scale, const LidarCrit* crit, float* loss_depth, float* loss_raydrop,
                            float* loss_intensity, float* pred_depth, float* pred_points, float* gt_points, hipStream_t stream) {
    REQUIRE(loss_depth && loss_raydrop && loss_intensity && (!crit || lidar_crit_ok(*crit)));
    if (N == 0) {
        if (hipMemsetAsync(loss_depth, 0, 4, stream) != hipSuccess || hipMemsetAsync(loss_raydrop, 0, 4, stream) != hipSuccess ||
            hipMemsetAsync(loss_intensity, 0, 4, stream) != hipSuccess)
            return (int)hipGetLastError();
        return NVSF_OK;
    }
    REQUIRE(image_lidar && depth_lidar && gt_raydrop && gt_intensity && gt_range && pred_depth);
    REQUIRE((pred_points == nullptr) == (gt_points == nullptr) && (!pred_points || (rays_d && scale != 0.0f)));
    hipLaunchKernelGGL(crit ? k_lidar_losses_fwd<true> : k_lidar_losses_fwd<false>, dim3(1), dim3(kBlock), 0, stream, image_lidar, depth_lidar,
                       gt_raydrop, gt_intensity, gt_range, rays_d, N, alpha_d, alpha_r, alpha_i, smooth_factor, scale, crit ? *crit : LidarCrit{},
                       loss_depth, loss_raydrop, loss_intensity, pred_depth, pred_points, gt_points);
    return nvsf_launch_status();
}

static int lidar_losses_bwd(const float* image_lidar, const float* depth_lidar, const float* gt_raydrop, const float* gt_intensity,
                            const float* gt_range, const float* rays_d, uint32_t N, float alpha_d, float alpha_r, float alpha_i,
                            float smooth_factor, float scale, const LidarCrit* crit, const float* grad_loss_depth,
                            const float* grad_loss_raydrop, const float* grad_loss_intensity, const float* grad_pred_depth,
                            const float* grad_pred_points, float* grad_image_lidar, float* grad_depth_lidar, hipStream_t stream) {
    REQUIRE(!crit || lidar_crit_ok(*crit));
    if (N == 0) return NVSF_OK;
    REQUIRE(image_lidar && depth_lidar && gt_raydrop && gt_intensity && gt_range && grad_image_lidar && grad_depth_lidar);
    REQUIRE(!grad_pred_points || (rays_d && scale != 0.0f));
    hipLaunchKernelGGL(crit ? k_lidar_losses_bwd<true> : k_lidar_losses_bwd<false>, dim3(cdiv(N, 256)), dim3(256), 0, stream, image_lidar,
                       depth_lidar, gt_raydrop, gt_intensity, gt_range, rays_d, N, alpha_d, alpha_r, alpha_i, smooth_factor, scale,
                       crit ? *crit : LidarCrit{}, grad_loss_depth, grad_loss_raydrop, grad_loss_intensity, grad_pred_depth, grad_pred_points,
                       grad_image_lidar, grad_depth_lidar);
    return nvsf_launch_status();
}

NVSF_API int nvsf_lidar_losses_fwd(const float* image_lidar, const float* depth_lidar, const float* gt_raydrop, const float* gt_intensity,
                                   const float* gt_range, const float* rays_d, uint32_t N, float alpha_d, float alpha_r, float alpha_i,
                                   float smooth_factor, float scale, float* loss_depth, float* loss_raydrop, float* loss_intensity,
                                   float* pred_depth, float* pred_points, float* gt_points, hipStream_t stream) {
    return lidar_losses_fwd(image_lidar, depth_lidar, gt_raydrop, gt_intensity, gt_range, rays_d, N, alpha_d, alpha_r, alpha_i, smooth_factor, scale,
                            nullptr, loss_depth, loss_raydrop, loss_intensity, pred_depth, pred_points, gt_points, stream);
}

NVSF_API int nvsf_lidar_losses_bwd(const float* image_lidar, const float* depth_lidar, const float* gt_raydrop, const float* gt_intensity,
                                   const float* gt_range, const float* rays_d, uint32_t N, float alpha_d, float alpha_r, float alpha_i,
                                   float smooth_factor, float scale, const float* grad_loss_depth, const float* grad_loss_raydrop,
                                   const float* grad_loss_intensity, const float* grad_pred_depth, const float* grad_pred_points,
                                   float* grad_image_lidar, float* grad_depth_lidar, hipStream_t stream) {
    return lidar_losses_bwd(image_lidar, depth_lidar, gt_raydrop, gt_intensity, gt_range, rays_d, N, alpha_d, alpha_r, alpha_i, smooth_factor, scale,
                            nullptr, grad_loss_depth, grad_loss_raydrop, grad_loss_intensity, grad_pred_depth, grad_pred_points, grad_image_lidar,
                            grad_depth_lidar, stream);
}

NVSF_API int nvsf_lidar_losses_crit_fwd(const float* image_lidar, const float* depth_lidar, const float* gt_raydrop, const float* gt_intensity,
                                        const float* gt_range, const float* rays_d, uint32_t N, float alpha_d, float alpha_r, float alpha_i,
                                        float smooth_factor, float scale, int depth_criterion, float depth_param, int raydrop_criterion,
                                        float raydrop_param, int intensity_criterion, float intensity_param, float* loss_depth,
                                        float* loss_raydrop, float* loss_intensity, float* pred_depth, float* pred_points, float* gt_points,
                                        hipStream_t stream) {
    const LidarCrit crit = {{depth_criterion, depth_param}, {raydrop_criterion, raydrop_param}, {intensity_criterion, intensity_param}};
    return lidar_losses_fwd(image_lidar, depth_lidar, gt_raydrop, gt_intensity, gt_range, rays_d, N, alpha_d, alpha_r, alpha_i, smooth_factor, scale,
                            &crit, loss_depth, loss_raydrop, loss_intensity, pred_depth, pred_points, gt_points, stream);
}

NVSF_API int nvsf_lidar_losses_crit_bwd(const float* image_lidar, const float* depth_lidar, const float* gt_raydrop, const float* gt_intensity,
                                        const float* gt_range, const float* rays_d, uint32_t N, float alpha_d, float alpha_r, float alpha_i,
                                        float smooth_factor, float scale, int depth_criterion, float depth_param, int raydrop_criterion,
                                        float raydrop_param, int intensity_criterion, float intensity_param, const float* grad_loss_depth,
                                        const float* grad_loss_raydrop, const float* grad_loss_intensity, const float* grad_pred_depth,
                                        const float* grad_pred_points, float* grad_image_lidar, float* grad_depth_lidar, hipStream_t stream) {
    const LidarCrit crit = {{depth_criterion, depth_param}, {raydrop_criterion, raydrop_param}, {intensity_criterion, intensity_param}};
    return lidar_losses_bwd(image_lidar, depth_lidar, gt_raydrop, gt_intensity, gt_range, rays_d, N, alpha_d, alpha_r, alpha_i, smooth_factor, scale,
                            &crit, grad_loss_depth, grad_loss_raydrop, grad_loss_intensity, grad_pred_depth, grad_pred_points, grad_image_lidar,
                            grad_depth_lidar, stream);
}

static int crit_sum_fwd(const float* a, const float* b, uint32_t n, float alpha, const TermCrit* crit, float* loss, hipStream_t stream) {
    REQUIRE(loss && (!crit || criterion_ok(crit->kind, crit->param)));
    if (n == 0) return hipMemsetAsync(loss, 0, 4, stream) == hipSuccess ? NVSF_OK : (int)hipGetLastError();
    REQUIRE(a && b);
    hipLaunchKernelGGL(crit ? k_mse_sum_fwd<true> : k_mse_sum_fwd<false>, dim3(1), dim3(kBlock), 0, stream, a, b, n, alpha,
                       crit ? *crit : TermCrit{}, loss);
    return nvsf_launch_status();
}

static int crit_sum_bwd(const float* a, const float* b, uint32_t n, float alpha, const TermCrit* crit, const float* grad_loss, float* grad_a,
                        hipStream_t stream) {
    REQUIRE(!crit || criterion_ok(crit->kind, crit->param));
    if (n == 0) return NVSF_OK;
    REQUIRE(a && b && grad_loss && grad_a);
    hipLaunchKernelGGL(crit ? k_mse_sum_bwd<true> : k_mse_sum_bwd<false>, dim3(cdiv(n, 256)), dim3(256), 0, stream, a, b, n, alpha,
                       crit ? *crit : TermCrit{}, grad_loss, grad_a);
    return nvsf_launch_status();
}

NVSF_API int nvsf_mse_sum_fwd(const float* a, const float* b, uint32_t n, float alpha, float* loss, hipStream_t stream) {
    return crit_sum_fwd(a, b, n, alpha, nullptr, loss, stream);
}

NVSF_API int nvsf_mse_sum_bwd(const float* a, const float* b, uint32_t n, float alpha, const float* grad_loss, float* grad_a, hipStream_t stream) {
    return crit_sum_bwd(a, b, n, alpha, nullptr, grad_loss, grad_a, stream);
}

NVSF_API int nvsf_crit_sum_fwd(const float* a, const float* b, uint32_t n, float alpha, int criterion, float criterion_param, float* loss,
                               hipStream_t stream) {
    const TermCrit crit = {criterion, criterion_param};
    return crit_sum_fwd(a, b, n, alpha, &crit, loss, stream);
}

NVSF_API int nvsf_crit_sum_bwd(const float* a, const float* b, uint32_t n, float alpha, int criterion, float criterion_param,
                               const float* grad_loss, float* grad_a, hipStream_t stream) {
    const TermCrit crit = {criterion, criterion_param};
    return crit_sum_bwd(a, b, n, alpha, &crit, grad_loss, grad_a, stream);
}

static int camera_loss_fwd(const float* image, const float* gt_rgb, const float* depth, const float* gt_depth_m, uint32_t N, float alpha_rgb,
                           float alpha_rd, float scale, float max_depth, int criterion, float criterion_param, const TermCrit* rgb,
                           float* loss_rgb, float* loss_depth, hipStream_t stream) {
    REQUIRE(loss_rgb && loss_depth && N <= (1u << 30));
    REQUIRE(criterion_ok(criterion, criterion_param) && max_depth == max_depth && (!rgb || criterion_ok(rgb->kind, rgb->param)));
    REQUIRE(N == 0 || (image && gt_rgb && depth && gt_depth_m));
    hipLaunchKernelGGL(rgb ? k_camera_loss_fwd<true> : k_camera_loss_fwd<false>, dim3(1), dim3(kBlock), 0, stream, image, gt_rgb, depth,
                       gt_depth_m, N, alpha_rgb, alpha_rd, scale, max_depth, criterion, criterion_param, rgb ? *rgb : TermCrit{}, loss_rgb,
                       loss_depth);
    return nvsf_launch_status();
}

static int camera_loss_bwd(const float* image, const float* gt_rgb, const float* depth, const float* gt_depth_m, uint32_t N, float alpha_rgb,
                           float alpha_rd, float scale, float max_depth, int criterion, float criterion_param, const TermCrit* rgb,
                           const float* grad_loss_rgb, const float* grad_loss_depth, float* grad_image, float* grad_depth, hipStream_t stream) {
    REQUIRE(N <= (1u << 30) && criterion_ok(criterion, criterion_param) && max_depth == max_depth);
    REQUIRE(!rgb || criterion_ok(rgb->kind, rgb->param));
    if (N == 0) return NVSF_OK;
    REQUIRE(image && gt_rgb && depth && gt_depth_m && grad_image && grad_depth);
    hipLaunchKernelGGL(rgb ? k_camera_loss_bwd<true> : k_camera_loss_bwd<false>, dim3(cdiv(N, 256)), dim3(256), 0, stream, image, gt_rgb, depth,
                       gt_depth_m, N, alpha_rgb, alpha_rd, scale, max_depth, criterion, criterion_param, rgb ? *rgb : TermCrit{}, grad_loss_rgb,
                       grad_loss_depth, grad_image, grad_depth);
    return nvsf_launch_status();
}

NVSF_API int nvsf_camera_loss_fwd(const float* image, const float* gt_rgb, const float* depth, const float* gt_depth_m, uint32_t N,
                                  float alpha_rgb, float alpha_rd, float scale, float max_depth, int criterion, float criterion_param,
                                  float* loss_rgb, float* loss_depth, hipStream_t stream) {
    return camera_loss_fwd(image, gt_rgb, depth, gt_depth_m, N, alpha_rgb, alpha_rd, scale, max_depth, criterion, criterion_param, nullptr,
                           loss_rgb, loss_depth, stream);
}

NVSF_API int nvsf_camera_loss_bwd(const float* image, const float* gt_rgb, const float* depth, const float* gt_depth_m, uint32_t N,
                                  float alpha_rgb, float alpha_rd, float scale, float max_depth, int criterion, float criterion_param,
                                  const float* grad_loss_rgb, const float* grad_loss_depth, float* grad_image, float* grad_depth,
                                  hipStream_t stream) {
    return camera_loss_bwd(image, gt_rgb, depth, gt_depth_m, N, alpha_rgb, alpha_rd, scale, max_depth, criterion, criterion_param, nullptr,
                           grad_loss_rgb, grad_loss_depth, grad_image, grad_depth, stream);
}

NVSF_API int nvsf_camera_loss_crit_fwd(const float* image, const float* gt_rgb, const float* depth, const float* gt_depth_m, uint32_t N,
                                       float alpha_rgb, float alpha_rd, float scale, float max_depth, int criterion, float criterion_param,
                                       int rgb_criterion, float rgb_param, float* loss_rgb, float* loss_depth, hipStream_t stream) {
    const TermCrit rgb = {rgb_criterion, rgb_param};
    return camera_loss_fwd(image, gt_rgb, depth, gt_depth_m, N, alpha_rgb, alpha_rd, scale, max_depth, criterion, criterion_param, &rgb, loss_rgb,
                           loss_depth, stream);
}

NVSF_API int nvsf_camera_loss_crit_bwd(const float* image, const float* gt_rgb, const float* depth, const float* gt_depth_m, uint32_t N,
                                       float alpha_rgb, float alpha_rd, float scale, float max_depth, int criterion, float criterion_param,
                                       int rgb_criterion, float rgb_param, const float* grad_loss_rgb, const float* grad_loss_depth,
                                       float* grad_image, float* grad_depth, hipStream_t stream) {
    const TermCrit rgb = {rgb_criterion, rgb_param};
    return camera_loss_bwd(image, gt_rgb, depth, gt_depth_m, N, alpha_rgb, alpha_rd, scale, max_depth, criterion, criterion_param, &rgb,
                           grad_loss_rgb, grad_loss_depth, grad_image, grad_depth, stream);
}

NVSF_API int nvsf_lidar_grad_loss_fwd(const float* pred_depth, const float* gt_depth, const float* gt_raydrop, const int64_t* pano_inds,
                                      const float* pano_range, uint32_t pano_stride, uint32_t N, uint32_t patch_h, uint32_t patch_w, uint32_t H,
                                      uint32_t W, float scale, int criterion, float criterion_param, float alpha, int sobel, float* patch_stats,
                                      float* loss, hipStream_t stream) {
    REQUIRE(loss);
    if (N == 0) return hipMemsetAsync(loss, 0, 4, stream) == hipSuccess ? NVSF_OK : (int)hipGetLastError();
    REQUIRE(pred_depth && gt_depth && gt_raydrop && pano_inds && pano_range && pano_stride >= 1);
    REQUIRE(patch_geom_ok(N, patch_h, patch_w, H, W, scale) && criterion_ok(criterion, criterion_param) && (criterion != 4 || patch_stats));
    const PatchGeom g = {patch_h, patch_w, H, W, scale};
    hipLaunchKernelGGL(k_lidar_grad_loss_fwd, dim3(1), dim3(kBlock), 0, stream, pred_depth, gt_depth, gt_raydrop,
                       reinterpret_cast<const long long*>(pano_inds), pano_range, pano_stride, N, g, criterion, criterion_param, alpha, sobel,
                       patch_stats, loss);
    return nvsf_launch_status();
}

NVSF_API int nvsf_lidar_grad_loss_bwd(const float* pred_depth, const float* gt_depth, const float* gt_raydrop, const int64_t* pano_inds,
                                      const float* pano_range, uint32_t pano_stride, uint32_t N, uint32_t patch_h, uint32_t patch_w, uint32_t H,
                                      uint32_t W, float scale, int criterion, float criterion_param, float alpha, int sobel,
                                      const float* patch_stats, const float* grad_loss, float* grad_pred_depth, hipStream_t stream) {
    if (N == 0) return NVSF_OK;
    REQUIRE(pred_depth && gt_depth && gt_raydrop && pano_inds && pano_range && pano_stride >= 1 && grad_loss && grad_pred_depth);
    REQUIRE(patch_geom_ok(N, patch_h, patch_w, H, W, scale) && criterion_ok(criterion, criterion_param) && (criterion != 4 || patch_stats));
    const PatchGeom g = {patch_h, patch_w, H, W, scale};
    hipLaunchKernelGGL(k_lidar_grad_loss_bwd, dim3(cdiv(N, 256)), dim3(256), 0, stream, pred_depth, gt_depth, gt_raydrop,
                       reinterpret_cast<const long long*>(pano_inds), pano_range, pano_stride, N, g, criterion, criterion_param, alpha, sobel,
                       patch_stats, grad_loss, grad_pred_depth);
    return nvsf_launch_status();
}

NVSF_API int nvsf_lidar_ray_losses(const float* image_lidar, const float* depth_lidar, const float* gt_raydrop, const float* gt_intensity,
                                   const float* gt_range, uint32_t N, float alpha_d, float alpha_r, float alpha_i, float smooth_factor,
                                   float* ray_loss, uint32_t* min_max_bits, hipStream_t stream) {
    if (N == 0) return NVSF_OK;
    REQUIRE(image_lidar && depth_lidar && gt_raydrop && gt_intensity && gt_range && ray_loss);
    hipLaunchKernelGGL(k_lidar_ray_losses, dim3(cdiv(N, 256)), dim3(256), 0, stream, image_lidar, depth_lidar, gt_raydrop, gt_intensity, gt_range, N,
                       alpha_d, alpha_r, alpha_i, smooth_factor, ray_loss, min_max_bits);
    return nvsf_launch_status();
}

NVSF_API int nvsf_mse_rows(const float* a, const float* b, uint32_t N, uint32_t C, float alpha, float* row_loss, uint32_t* min_max_bits,
                           hipStream_t stream) {
    if (N == 0) return NVSF_OK;
    REQUIRE(a && b && row_loss && C >= 1);
    hipLaunchKernelGGL(k_mse_rows, dim3(cdiv(N, 256)), dim3(256), 0, stream, a, b, N, C, alpha, row_loss, min_max_bits);
    return nvsf_launch_status();
}

NVSF_API int nvsf_lidar_ray_losses_crit(const float* image_lidar, const float* depth_lidar, const float* gt_raydrop, const float* gt_intensity,
                                        const float* gt_range, uint32_t N, float alpha_d, float alpha_r, float alpha_i, float smooth_factor,
                                        int depth_criterion, float depth_param, int raydrop_criterion, float raydrop_param,
                                        int intensity_criterion, float intensity_param, float* ray_loss, uint32_t* min_max_bits,
                                        hipStream_t stream) {
    const LidarCrit crit = {{depth_criterion, depth_param}, {raydrop_criterion, raydrop_param}, {intensity_criterion, intensity_param}};
    REQUIRE(lidar_crit_ok(crit));
    if (N == 0) return NVSF_OK;
    REQUIRE(image_lidar && depth_lidar && gt_raydrop && gt_intensity && gt_range && ray_loss);
    hipLaunchKernelGGL(k_lidar_ray_losses_crit, dim3(1), dim3(kBlock), 0, stream, image_lidar, depth_lidar, gt_raydrop, gt_intensity, gt_range, N,
                       alpha_d, alpha_r, alpha_i, smooth_factor, crit, ray_loss, min_max_bits);
    return nvsf_launch_status();
}

NVSF_API int nvsf_crit_rows(const float* a, const float* b, uint32_t N, uint32_t C, float alpha, int criterion, float criterion_param,
                            float* row_loss, uint32_t* min_max_bits, hipStream_t stream) {
    REQUIRE(criterion_ok(criterion, criterion_param));
    if (N == 0) return NVSF_OK;
    REQUIRE(a && b && row_loss && C >= 1);
    hipLaunchKernelGGL(k_crit_rows, dim3(1), dim3(kBlock), 0, stream, a, b, N, C, alpha, TermCrit{criterion, criterion_param}, row_loss,
                       min_max_bits);
    return nvsf_launch_status();
}

// ---- line-of-sight loss ---------------------------------------------------------------------------------------------------------
struct UrfLaunch { uint32_t blocks; bool vec, rows4; double inv2s2; };
static UrfLaunch urf_launch(const void* a, const void* b, const void* c, uint32_t N, uint32_t T, float eps, float eps_lo) {
    UrfLaunch l;
    const uint64_t total = (uint64_t)N * T;
    l.vec = (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u) == 0;
    l.rows4 = l.vec && T % 4 == 0;
    const uint64_t items = l.vec ? total / 4 + 3 : total;  // grid-stride: a few workgroups per CU, not one thread per element
    const uint64_t want = (items + kUrfBlock - 1) / kUrfBlock, cap = (uint64_t)4 * (uint64_t)nvsf_cu_count();
    uint64_t blocks = want < cap ? want : cap;
    blocks = blocks < 1 ? 1 : (blocks > (uint64_t)kUrfMaxBlocks ? (uint64_t)kUrfMaxBlocks : blocks);
    l.blocks = (uint32_t)blocks;
    const double sigma = ((double)eps + (double)eps_lo) / 3.0;
    l.inv2s2 = 1.0 / (2.0 * sigma * sigma);
    return l;
}

NVSF_API int nvsf_urf_loss_fwd(const float* weights, const float* z_vals, const float* gt_depth, uint32_t N, uint32_t T, float eps, float eps_lo,
                               void* workspace, size_t ws_bytes, float* loss, double* state, hipStream_t stream) {
    REQUIRE(loss && state && workspace && ((uintptr_t)workspace & 7u) == 0 && ws_bytes >= (size_t)kUrfMaxBlocks * kUrfSlots * sizeof(double));
    REQUIRE((uint64_t)N * T <= (1ull << 31) && eps > 0.0f && (double)eps + (double)eps_lo > 0.0);
    REQUIRE((uint64_t)N * T == 0 || (weights && z_vals));
    REQUIRE(N == 0 || gt_depth);
    const UrfLaunch l = urf_launch(weights, z_vals, nullptr, N, T, eps, eps_lo);
    double* partials = static_cast<double*>(workspace);
    const auto kernel = l.rows4 ? k_urf_partials<true, true> : (l.vec ? k_urf_partials<true, false> : k_urf_partials<false, false>);
    hipLaunchKernelGGL(kernel, dim3(l.blocks), dim3(kUrfBlock), 0, stream, weights, z_vals, gt_depth, N, T, eps, l.inv2s2, partials);
    hipLaunchKernelGGL(k_urf_fold, dim3(1), dim3(kWave), 0, stream, partials, l.blocks, l.inv2s2, loss, state);
    return nvsf_launch_status();
}

NVSF_API int nvsf_urf_loss_bwd(const float* weights, const float* z_vals, const float* gt_depth, uint32_t N, uint32_t T, float eps, float eps_lo,
                               const double* state, const float* grad_loss, float* grad_weights, hipStream_t stream) {
    REQUIRE((uint64_t)N * T <= (1ull << 31) && eps > 0.0f && (double)eps + (double)eps_lo > 0.0);
    if ((uint64_t)N * T == 0) return NVSF_OK;
    REQUIRE(weights && z_vals && gt_depth && state && grad_loss && grad_weights);
    const UrfLaunch l = urf_launch(weights, z_vals, grad_weights, N, T, eps, eps_lo);
    const auto kernel = l.rows4 ? k_urf_bwd<true, true> : (l.vec ? k_urf_bwd<true, false> : k_urf_bwd<false, false>);
    hipLaunchKernelGGL(kernel, dim3(l.blocks), dim3(kUrfBlock), 0, stream, weights, z_vals, gt_depth, N, T, eps, l.inv2s2, state, grad_loss,
                       grad_weights);
    return nvsf_launch_status();
}

// ---- distortion loss ------------------------------------------------------------------------------------------------------------
NVSF_API int nvsf_distortion_loss_fwd(const float* weights, const float* z_vals, const float* nears, const float* fars, uint32_t N, uint32_t T,
                                      float alpha, void* workspace, size_t ws_bytes, float* ray_loss, float* loss, double* state,
                                      hipStream_t stream) {
    REQUIRE(loss && T >= 1 && (uint64_t)N * T <= (1ull << 31));
    if (N == 0) return hipMemsetAsync(loss, 0, 4, stream) == hipSuccess ? NVSF_OK : (int)hipGetLastError();
    const uint32_t blocks = cdiv(N, kDistRays);
    REQUIRE(weights && z_vals && nears && fars && state && workspace && ((uintptr_t)workspace & 7u) == 0);
    REQUIRE(ws_bytes >= (size_t)blocks * sizeof(double));
    double* partials = static_cast<double*>(workspace);
    hipLaunchKernelGGL(k_distortion_fwd, dim3(blocks), dim3(kDistBlock), 0, stream, weights, z_vals, nears, fars, N, T, ray_loss, state, partials);
    hipLaunchKernelGGL(k_distortion_fold, dim3(1), dim3(kBlock), 0, stream, partials, blocks, (double)alpha / (double)N, loss);
    return nvsf_launch_status();
}

NVSF_API int nvsf_distortion_loss_bwd(const float* weights, const float* z_vals, const float* nears, const float* fars, uint32_t N, uint32_t T,
                                      float alpha, const double* state, const float* grad_loss, float* grad_weights, hipStream_t stream) {
    REQUIRE(T >= 1 && (uint64_t)N * T <= (1ull << 31));
    if (N == 0) return NVSF_OK;
    REQUIRE(weights && z_vals && nears && fars && state && grad_loss && grad_weights);
    hipLaunchKernelGGL(k_distortion_bwd, dim3(cdiv(N, kDistRays)), dim3(kDistBlock), 0, stream, weights, z_vals, nears, fars, N, T,
                       (double)alpha / (double)N, state, grad_loss, grad_weights);
    return nvsf_launch_status();
}

NVSF_API int nvsf_error_map_update(const float* ray_loss, const int64_t* pixel_inds, uint32_t N, uint32_t W, float* error_map, uint32_t map_h,
                                   uint32_t map_w, float scale_h, float scale_w, const uint32_t* min_max_bits, uint32_t* owner, hipStream_t stream) {
    if (N == 0) return NVSF_OK;
    REQUIRE(ray_loss && pixel_inds && error_map && min_max_bits && owner && W >= 1 && map_h >= 1 && map_w >= 1 && scale_h > 0.0f && scale_w > 0.0f);
    hipLaunchKernelGGL(k_error_map_claim, dim3(cdiv(N, 256)), dim3(256), 0, stream, reinterpret_cast<const long long*>(pixel_inds), N, W, map_h,
                       map_w, scale_h, scale_w, owner);
    hipLaunchKernelGGL(k_error_map_write, dim3(cdiv(N, 256)), dim3(256), 0, stream, ray_loss, reinterpret_cast<const long long*>(pixel_inds), N, W,
                       map_h, map_w, scale_h, scale_w, min_max_bits, owner, error_map);
    return nvsf_launch_status();
}
