// Fused space-time hash encoder (the dynamic half of HashGrid4D) and the flow-field grid reduction for gfx950.
// Reference: /root/reference/nvsf/nerf/models/hash_field.py:29-88 (HashGridT), :148-159 (forward_dynamic) and
// flow_field.py:105-128 -- there: per coordinate pair two tcnn HashGrid launches (the time slices around t), a linear
// blend, a view/chunk and seven elementwise kernels for the cubic Lagrange reduction, three times per call, three
// calls per density evaluation (t, t+1, t-1): ~40 launches and ~30 [M,32] temporaries per call.
// Here: ONE launch per (positions, time): every (sample, pair, level) item gathers its 2 x 4 corners, blends the two
// slices and reduces its 4 features with the Lagrange weights; results are staged in LDS and leave as whole rows.
//
// The reference's arithmetic depends on the operand types PyTorch sees (hash_field.py docstring in this repo):
//   mode 0 ("tensor t"): blend and reduction in fp32, output fp32;
//   mode 1 ("0-dim t", the flow-warped neighbour frames): every product and every sum is rounded to fp16.
// Both are reproduced operation by operation (tests/test_dynamic_gpu.py against fixtures from the reference code).
#include <stdlib.h>
#include "hashgrid_device.h"

namespace {
constexpr int kBlock = 256;
constexpr int kSamplesPerBlock = 64;
constexpr int kPlaneLevels = 8;   // HashGridT: n_levels = 8, F = 4, num_basis = 4 (hash_field.py:35-38)
constexpr int kF = 4;

// The time side of one evaluation: the two slices around t and the time weights.  T = const _Float16: the slice tables of a forward;
// T = float: their fp32 gradient buffers.
template <typename T>
struct TimeSet {
    T* table_lo[3];               // slice floor(idx) of the pairs (x,y), (x,z), (y,z)
    T* table_hi[3];               // slice ceil(idx)
    float blend_lo, blend_hi;     // (k2 - idx), (idx - k1)
    float lag[4];                 // Lagrange weights at t
    int same_slice;               // idx integral: no blend, the slice features are used as they are (fp16)
};
struct PlaneSet {
    TimeSet<const _Float16> ts;
    GridMeta meta[3];
};

__device__ __forceinline__ float r16(float v) { return (float)(_Float16)v; }  // round-trip through fp16

template <int MODE, typename T>
__device__ __forceinline__ float blend_reduce(const float (&f_lo)[kF], const float (&f_hi)[kF], const TimeSet<T>& ps) {
    float feat[kF];
#pragma unroll
    for (int i = 0; i < kF; ++i) {
        if (ps.same_slice) feat[i] = f_lo[i];
        else if (MODE == 0) feat[i] = ps.blend_lo * f_lo[i] + ps.blend_hi * f_hi[i];
        else feat[i] = r16(r16(ps.blend_lo * f_lo[i]) + r16(ps.blend_hi * f_hi[i]));
    }
    float acc;
    if (MODE == 0) {
        acc = ps.lag[0] * feat[0];
#pragma unroll
        for (int i = 1; i < kF; ++i) acc = acc + ps.lag[i] * feat[i];
    } else {
        acc = r16(ps.lag[0] * feat[0]);
#pragma unroll
        for (int i = 1; i < kF; ++i) acc = r16(acc + r16(ps.lag[i] * feat[i]));
    }
    return acc;
}

// Prologue of the sample-per-lane kernels: p = x[m, 0:3] (+ offset[m, off_col : off_col + 3] where there is one).  A lane past the end
// takes the last sample: it computes a valid position and is dropped at the store.  Returns the clamped sample index.
__device__ __forceinline__ uint32_t load_position(const float* __restrict__ x, uint32_t x_stride, const float* __restrict__ offset, uint32_t off_stride,
                                              uint32_t off_col, uint32_t m, uint32_t M, float (&p)[3]) {
    const uint32_t mm = m < M ? m : M - 1;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        p[d] = x[(size_t)mm * x_stride + d];
        if (offset) p[d] = p[d] + offset[(size_t)mm * off_stride + off_col + d];
    }
    return mm;
}

// Epilogue: the workgroup's rows of a staging tile (`pitch` floats apart, filled before a barrier) leave as whole rows of n_cols values of T
template <typename T>
__device__ __forceinline__ void store_staged_rows(const float* stage, uint32_t pitch, uint32_t n_cols, uint32_t M, T* __restrict__ out) {
    const uint32_t n_rows = min((uint32_t)kSamplesPerBlock, M - blockIdx.x * kSamplesPerBlock);
    for (uint32_t c = threadIdx.x; c < n_rows * n_cols; c += kBlock) {
        const uint32_t row = c / n_cols, col = c - row * n_cols;
        out[(size_t)(blockIdx.x * kSamplesPerBlock + row) * n_cols + col] = (T)stage[row * pitch + col];
    }
}

// x' = x[:, 0:3] (+ offset[:, off_col : off_col+3]); out [M, 24]: fp32 (MODE 0) or fp16 (MODE 1)
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_hash_dynamic(const float* __restrict__ x, uint32_t x_stride, const float* __restrict__ offset,
                                                         uint32_t off_stride, uint32_t off_col, uint32_t M, PlaneSet ps,
                                                         void* __restrict__ out) {
    __shared__ float stage[kSamplesPerBlock][3 * kPlaneLevels + 1];
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform by construction: level tables, pointers and loop control in SGPRs
    float p[3];
    load_position(x, x_stride, offset, off_stride, off_col, blockIdx.x * kSamplesPerBlock + lane, M, p);
    for (int item = wave; item < 3 * kPlaneLevels; item += 4) {
        const int pl = item / kPlaneLevels, l = item - pl * kPlaneLevels;
        const float xy[2] = {p[pl == 2 ? 1 : 0], p[pl == 0 ? 1 : 2]};
        const GridMeta& g = ps.meta[pl];
        const uint32_t rows = g.offset[l + 1] - g.offset[l];
        float f_lo[kF], f_hi[kF];
        encode_level<2, kF>(xy, ps.ts.table_lo[pl], g.scale[l], g.res[l], g.offset[l], rows, f_lo);
#pragma unroll
        for (int i = 0; i < kF; ++i) f_lo[i] = r16(f_lo[i]);  // the slice encoders return fp16
        if (!ps.ts.same_slice) {
            encode_level<2, kF>(xy, ps.ts.table_hi[pl], g.scale[l], g.res[l], g.offset[l], rows, f_hi);
#pragma unroll
            for (int i = 0; i < kF; ++i) f_hi[i] = r16(f_hi[i]);
        } else {
#pragma unroll
            for (int i = 0; i < kF; ++i) f_hi[i] = 0.0f;
        }
        stage[lane][item] = blend_reduce<MODE>(f_lo, f_hi, ps.ts);
    }
    __syncthreads();
    if (MODE == 0) store_staged_rows(&stage[0][0], 3 * kPlaneLevels + 1, 3 * kPlaneLevels, M, reinterpret_cast<float*>(out));
    else store_staged_rows(&stage[0][0], 3 * kPlaneLevels + 1, 3 * kPlaneLevels, M, reinterpret_cast<_Float16*>(out));
}

// Coordinate gradient of the encoder above: dL/dp of the piecewise-bilinear function k_hash_dynamic evaluates, on its own
// cell, p = x (+ offset).  The fp16 rounding points of both forward regimes pass the gradient straight through, so one derivative serves
// mode 0 and mode 1.  Per (pair, level) item with axes (a, b), in fp32:
//   s[c][i] = lo[row(c)][i]  (same_slice)   or   blend_lo lo[row(c)][i] + blend_hi hi[row(c)][i];   e[c] = sum_i lag_i s[c][i]
//   G = grad_scale grad_out[m, 8 pair + level]
//   acc_a += scale G ((1 - frac_b) (e[10] - e[00]) + frac_b (e[11] - e[01]))
//   acc_b += scale G ((1 - frac_a) (e[01] - e[00]) + frac_a (e[11] - e[10]))
// The corner pairs along an axis are differenced first (as k_hashgrid_grad_x does): a table that does not vary along an axis gives an
// exact zero.  Mapping of k_hashgrid_grad_x: lanes = 64 consecutive samples, the four waves split the 24 items, the 2 x 4 gathers of an
// item in flight before any arithmetic, three partial sums per wave, added through LDS in wave order.  No atomics: reruns are
// bit-identical.
__global__ __launch_bounds__(kBlock) void k_hash_dynamic_grad_x(const float* __restrict__ x, uint32_t x_stride, const float* __restrict__ offset,
                                                                uint32_t off_stride, uint32_t off_col, uint32_t M, PlaneSet ps,
                                                                const float* __restrict__ grad_out, uint32_t go_stride, float grad_scale,
                                                                float* __restrict__ grad_x, uint32_t gx_stride, int accumulate) {
    __shared__ float part[kBlock / 64][3][64];  // [wave][axis][lane]
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform by construction: level tables, pointers and loop control in SGPRs
    const uint32_t m = blockIdx.x * kSamplesPerBlock + lane;
    float p[3];
    const uint32_t mm = load_position(x, x_stride, offset, off_stride, off_col, m, M, p);  // also the row of grad_out
    float sum[3] = {0.0f, 0.0f, 0.0f};
    for (int item = wave; item < 3 * kPlaneLevels; item += 4) {
        const int pl = item / kPlaneLevels, l = item - pl * kPlaneLevels;
        const int ia = pl == 2 ? 1 : 0, ib = pl == 0 ? 1 : 2;
        const float xy[2] = {p[ia], p[ib]};
        const GridMeta& g = ps.meta[pl];
        const float scale = g.scale[l];
        const uint32_t row0 = g.offset[l], rows = g.offset[l + 1] - row0;
        const float G = grad_scale * grad_out[(size_t)mm * go_stride + item];
        float frac[2];
        uint32_t cell[2];
        grid_cell<2>(xy, scale, cell, frac);
        float v_lo[4][kF], v_hi[4][kF];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t cc[2] = {cell[0] + (uint32_t)(c & 1), cell[1] + (uint32_t)(c >> 1)};
            const size_t row = (size_t)row0 + grid_row<2>(cc, g.res[l], rows);
            load_feat<kF>(ps.ts.table_lo[pl], row, v_lo[c]);
            if (!ps.ts.same_slice) load_feat<kF>(ps.ts.table_hi[pl], row, v_hi[c]);
        }
        float e[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float s[kF];
#pragma unroll
            for (int i = 0; i < kF; ++i) s[i] = ps.ts.same_slice ? v_lo[c][i] : ps.ts.blend_lo * v_lo[c][i] + ps.ts.blend_hi * v_hi[c][i];
            e[c] = ps.ts.lag[0] * s[0];
#pragma unroll
            for (int i = 1; i < kF; ++i) e[c] = e[c] + ps.ts.lag[i] * s[i];
        }
        const float da = (1.0f - frac[1]) * (e[1] - e[0]) + frac[1] * (e[3] - e[2]);
        const float db = (1.0f - frac[0]) * (e[2] - e[0]) + frac[0] * (e[3] - e[1]);
        const float sg = scale * G;
        // the axes of a pair are wave-uniform: branched on, not indexed, so that sum[] stays in registers
        if (pl == 0) { sum[0] = sum[0] + sg * da; sum[1] = sum[1] + sg * db; }
        else if (pl == 1) { sum[0] = sum[0] + sg * da; sum[2] = sum[2] + sg * db; }
        else { sum[1] = sum[1] + sg * da; sum[2] = sum[2] + sg * db; }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) part[wave][d][lane] = sum[d];
    __syncthreads();
    if (wave == 0 && m < M) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float v = ((part[0][d][lane] + part[1][d][lane]) + part[2][d][lane]) + part[3][d][lane];
            float* dst = grad_x + (size_t)m * gx_stride + d;
            *dst = accumulate ? *dst + v : v;
        }
    }
}

// The three space-time evaluations of one density query (network_dynamic.py:220-271) in one launch: features at (x, t) in
// regime 0 and at the flow-warped positions (x + f1, t1), (x + f2, t2) of the neighbour frames in regime 1.  The warped
// positions are fractions of a cell away from x at the coarse levels (and everywhere the scene is static), and the
// neighbour frames usually fall between the same two time slices as t: whenever a neighbour's cell at a level equals the
// base cell and its slices are the base slices, the 2 x 4 table entries the base evaluation has just gathered (kept as
// raw 8-byte values, 16 registers) are re-used and only the weights differ; otherwise the neighbour gathers its own.
// Same gathers / same arithmetic per evaluation as three k_hash_dynamic launches: bit-identical outputs.
struct PlaneSet3 {
    TimeSet<const _Float16> ev[3];  // what differs between the evaluations
    GridMeta meta[3];  // per pair (shared by the evaluations)
    int enabled[3];    // ev[0] always; ev[1], ev[2]: neighbour present
    int share[3];      // ev[e] reads the same slice tables as ev[0] (same k1, k2): its cells may re-use ev[0]'s gathers
};

typedef u32x2_t u2_t;

// Two lanes per sample (lane = 2 * sample + x-bit, 32 samples per pass, two passes per item): a lane gathers the two corners with
// its x-bit of a slice, so a gather instruction fetches BOTH x-neighbours of 32 samples -- the same 16-byte pair for even cells,
// the same 128-byte line otherwise -- and the kernel, which is bound by the L1 look-ups of its ~200 eight-byte gathers per sample,
// makes half of them.  The even lane blends features 0, 1 of all four corners, the odd lane features 2, 3 (the partner's halves
// arrive by lane_swap), each in the corner order of encode_level<2, 4>; the odd lane then hands its two rounded features per
// slice to the even lane, which runs blend_reduce as the one-lane form does: bit-identical outputs.
// gather_pair: this lane's two corners (x-bit xb, y = 0, 1) of the cell of xy
__device__ __forceinline__ void gather_pair(const float (&xy)[2], uint32_t xb, const _Float16* __restrict__ table, float scale, uint32_t res,
                                            uint32_t row0, uint32_t hsize, uint32_t (&cell)[2], float (&frac)[2], u2_t (&raw)[2]) {
    grid_cell<2>(xy, scale, cell, frac);
#pragma unroll
    for (int y = 0; y < 2; ++y) {
        const uint32_t cc[2] = {cell[0] + xb, cell[1] + (uint32_t)y};
        raw[y] = *reinterpret_cast<const u2_t*>(table + ((size_t)row0 + grid_row<2>(cc, res, hsize)) * kF);
    }
}
// features (2 xb, 2 xb + 1) of the cell, blended over the four corners in encode_level's order, rounded to fp16 as the slice encoders return them
__device__ __forceinline__ void blend_pair(const u2_t (&raw)[2], uint32_t xb, const float (&frac)[2], float (&f)[2]) {
    uint32_t mine[4];  // this lane's feature pair of corner c = x + 2 y
    exchange_halves<2>(raw, xb, mine);
    f[0] = f[1] = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float wc = 1.0f;
#pragma unroll
        for (int d = 0; d < 2; ++d) wc = wc * ((c & (1 << d)) ? frac[d] : (1.0f - frac[d]));
        const h2_t v = __builtin_bit_cast(h2_t, mine[c]);
        f[0] = fmaf(wc, (float)v[0], f[0]);
        f[1] = fmaf(wc, (float)v[1], f[1]);
    }
    f[0] = r16(f[0]);
    f[1] = r16(f[1]);
}

// One evaluation's features from its gathered slices: both slices blended over the corners, features 2, 3 fetched from the odd lane, and the
// even lane reduces (*dst belongs to the sample; the odd lane writes nothing)
template <int MODE>
__device__ __forceinline__ void reduce_pairs(const u2_t (&lo)[2], const u2_t (&hi)[2], uint32_t xb, const float (&frac)[2],
                                             const TimeSet<const _Float16>& ts, float* dst) {
    float a[2], b[2] = {0.0f, 0.0f};
    blend_pair(lo, xb, frac, a);
    if (!ts.same_slice) blend_pair(hi, xb, frac, b);
    const float a2 = lane_swap_f(a[0]), a3 = lane_swap_f(a[1]), b2 = lane_swap_f(b[0]), b3 = lane_swap_f(b[1]);
    const float f_lo[kF] = {a[0], a[1], a2, a3}, f_hi[kF] = {b[0], b[1], b2, b3};
    if (xb == 0u) *dst = blend_reduce<MODE>(f_lo, f_hi, ts);
}

__global__ __launch_bounds__(kBlock) void k_hash_dynamic3(const float* __restrict__ x, uint32_t x_stride, const float* __restrict__ off,
                                                          uint32_t off_stride, uint32_t M, PlaneSet3 ps, float* __restrict__ out0,
                                                          _Float16* __restrict__ out1, _Float16* __restrict__ out2) {
    __shared__ float stage[3][kSamplesPerBlock][3 * kPlaneLevels + 1];
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform by construction: level tables, pointers and loop control in SGPRs
    const uint32_t xb = (uint32_t)(lane & 1);
    float p[2][3][3];  // [pass][evaluation][axis]
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t m = blockIdx.x * kSamplesPerBlock + 32u * h + (uint32_t)(lane >> 1);
        // load_position, restated: one read of x serves the three evaluations (calling it per evaluation moved 2 VGPRs / 2 SGPRs in this kernel)
        const uint32_t mm = m < M ? m : M - 1;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float xd = x[(size_t)mm * x_stride + d];
            p[h][0][d] = xd;
            p[h][1][d] = ps.enabled[1] ? xd + off[(size_t)mm * off_stride + d] : xd;
            p[h][2][d] = ps.enabled[2] ? xd + off[(size_t)mm * off_stride + 3 + d] : xd;
        }
    }
    for (int item = wave; item < 3 * kPlaneLevels; item += 4) {
        const int pl = item / kPlaneLevels, l = item - pl * kPlaneLevels;
        const int ia = pl == 2 ? 1 : 0, ib = pl == 0 ? 1 : 2;
        const GridMeta& g = ps.meta[pl];
        const float scale = g.scale[l];
        const uint32_t res = g.res[l], row0 = g.offset[l], rows = g.offset[l + 1] - g.offset[l];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = 32 * h + (lane >> 1);
            // ---- base evaluation: gathers kept
            uint32_t cell0[2];
            float frac0[2];
            u2_t lo0[2], hi0[2];
            {
                const float xy[2] = {p[h][0][ia], p[h][0][ib]};
                gather_pair(xy, xb, ps.ev[0].table_lo[pl], scale, res, row0, rows, cell0, frac0, lo0);
                if (!ps.ev[0].same_slice) {
                    uint32_t c_[2];
                    float f_[2];
                    gather_pair(xy, xb, ps.ev[0].table_hi[pl], scale, res, row0, rows, c_, f_, hi0);
                } else {
                    hi0[0] = lo0[0];
                    hi0[1] = lo0[1];
                }
                reduce_pairs<0>(lo0, hi0, xb, frac0, ps.ev[0], &stage[0][row][item]);
            }
            // ---- neighbour evaluations (regime 1)
#pragma unroll
            for (int e = 1; e < 3; ++e) {
                if (!ps.enabled[e]) continue;
                const TimeSet<const _Float16>& pe = ps.ev[e];
                const float xy[2] = {p[h][e][ia], p[h][e][ib]};
                uint32_t cell[2];
                float frac[2];
                grid_cell<2>(xy, scale, cell, frac);
                u2_t lo[2], hi[2];
                const bool reuse = ps.share[e] && cell[0] == cell0[0] && cell[1] == cell0[1];  // the same for both lanes of a sample
                if (reuse) {
#pragma unroll
                    for (int y = 0; y < 2; ++y) { lo[y] = lo0[y]; hi[y] = hi0[y]; }
                } else {
                    uint32_t c_[2];
                    float f_[2];
                    gather_pair(xy, xb, pe.table_lo[pl], scale, res, row0, rows, c_, f_, lo);
                    if (!pe.same_slice) gather_pair(xy, xb, pe.table_hi[pl], scale, res, row0, rows, c_, f_, hi);
                    else { hi[0] = lo[0]; hi[1] = lo[1]; }
                }
                reduce_pairs<1>(lo, hi, xb, frac, pe, &stage[e][row][item]);
            }
        }
    }
    __syncthreads();
    // store_staged_rows, restated: the three tiles leave in ONE loop (a call per tile added 26 instructions and failed the timing rule in
    // tools/bench_dynamic.py)
    const uint32_t n_rows = min((uint32_t)kSamplesPerBlock, M - blockIdx.x * kSamplesPerBlock);
    constexpr int kOut = 3 * kPlaneLevels;
    for (uint32_t c = threadIdx.x; c < n_rows * kOut; c += kBlock) {
        const uint32_t row = c / kOut, col = c - row * kOut;
        const size_t o = (size_t)(blockIdx.x * kSamplesPerBlock + row) * kOut + col;
        out0[o] = stage[0][row][col];
        if (ps.enabled[1]) out1[o] = (_Float16)stage[1][row][col];
        if (ps.enabled[2]) out2[o] = (_Float16)stage[2][row][col];
    }
}

// Flow-field front end (flow_field.py:123-128): 3-D grid (L levels, F = 8) -> .float() -> Lagrange reduction over the
// two groups of 4 features of every level -> fp32 [M, 2 L].
__global__ __launch_bounds__(kBlock) void k_hash3d_lagrange(const float* __restrict__ x, uint32_t x_stride, uint32_t M,
                                                            const _Float16* __restrict__ table, uint32_t L, GridMeta meta, float w0, float w1,
                                                            float w2, float w3, float* __restrict__ out) {
    extern __shared__ float stage_dyn[];  // [64][2L + 1]
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform by construction: level tables, pointers and loop control in SGPRs
    const uint32_t pitch = 2 * L + 1;
    float p[3];
    load_position(x, x_stride, nullptr, 0u, 0u, blockIdx.x * kSamplesPerBlock + lane, M, p);
    const float w[4] = {w0, w1, w2, w3};
    for (uint32_t l = wave; l < L; l += 4) {
        float f[8];
        encode_level<3, 8>(p, table, meta.scale[l], meta.res[l], meta.offset[l], meta.offset[l + 1] - meta.offset[l], f);
        // x.view(-1, L, 8) chunked into 4 along the feature axis: chunk i = features (2i, 2i+1)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float acc = w[0] * r16(f[e]);
#pragma unroll
            for (int i = 1; i < 4; ++i) acc = acc + w[i] * r16(f[2 * i + e]);
            stage_dyn[lane * pitch + 2 * l + e] = acc;
        }
    }
    __syncthreads();
    store_staged_rows(stage_dyn, pitch, 2 * L, M, out);
}

// Table gradients of the fused space-time encoder, regime 0 (fp32 blend / reduction: the current frame, the only call that
// records a gradient -- the neighbour frames are evaluated under no_grad, network_dynamic.py:242-271):
//   out[pair][level] = sum_i lag_i (blend_lo f_lo[i] + blend_hi f_hi[i]),  f_*[i] = sum_corners w_c table_*[row_c][i]
//   => d L / d table_lo[row_c][i] += g[pair][level] lag_i blend_lo w_c      (the fp16 rounding of f passes the gradient)
// One launch for the three pairs and both slices instead of six hash-grid backward launches fed by ~30 elementwise kernels
// that materialise per-slice gradient matrices.  Same scheme as k_hashgrid_bwd_corners (hashgrid.hip): an item = (chunk of
// rows, pair, level, slice), 16 lanes per item (lane = corner x 4 + feature), the sums of the current cell in registers,
// one atomic instruction per cell change covering whole 16-byte table entries.
struct PlaneGrads {
    TimeSet<float> ts;  // the slice gradients: fp32 buffers in the layout of the slice tables
    GridMeta meta[3];
};

// The run-merging walk of one item: rows [m0, m1) of column `gcol` of grad_out at one level of the pair with coordinate columns (ca, cb), on
// 4 lanes (corner c) per scattered float.  The lane keeps the sum of its corner of the current cell and adds it to dst_of(row of the corner)
// when the cell changes.  `factor`: what the gradient is multiplied by before the weight (the literal 1 folds away).
template <class Dst>
__device__ __forceinline__ void walk_runs(const float* __restrict__ x, uint32_t x_stride, const float* __restrict__ grad_out, uint32_t gcol, uint32_t m0,
                                          uint32_t m1, uint32_t ca, uint32_t cb, const GridMeta& g, uint32_t l, int c, float factor, Dst dst_of) {
    const float scale = g.scale[l];
    const uint32_t res = g.res[l], row0 = g.offset[l], hsize = g.offset[l + 1] - row0;
    float acc = 0.0f;
    uint32_t cur[2] = {0u, 0u};
    bool have = false;
    float* dst = dst_of(0);
    float xy_n[2] = {x[(size_t)m0 * x_stride + ca], x[(size_t)m0 * x_stride + cb]};
    float g_n = grad_out[(size_t)m0 * (3 * kPlaneLevels) + gcol];
    for (uint32_t m = m0; m < m1; ++m) {
        const float xy[2] = {xy_n[0], xy_n[1]}, go = g_n;
        if (m + 1 < m1) {
            xy_n[0] = x[(size_t)(m + 1) * x_stride + ca];
            xy_n[1] = x[(size_t)(m + 1) * x_stride + cb];
            g_n = grad_out[(size_t)(m + 1) * (3 * kPlaneLevels) + gcol];
        }
        if (go == 0.0f) continue;
        float frac[2];
        uint32_t cell[2];
        grid_cell<2>(xy, scale, cell, frac);
        const float w = ((c & 1) ? frac[0] : (1.0f - frac[0])) * ((c & 2) ? frac[1] : (1.0f - frac[1]));
        if (!(have && cell[0] == cur[0] && cell[1] == cur[1])) {
            if (acc != 0.0f) atomicAdd(dst, acc);
            acc = 0.0f;
            have = true;
            cur[0] = cell[0]; cur[1] = cell[1];
            const uint32_t cc[2] = {cell[0] + (uint32_t)(c & 1), cell[1] + (uint32_t)((c >> 1) & 1)};
            dst = dst_of((size_t)row0 + grid_row<2>(cc, res, hsize));
        }
        acc += w * (go * factor);
    }
    if (acc != 0.0f) atomicAdd(dst, acc);
}

__global__ __launch_bounds__(kBlock) void k_hash_dynamic_bwd(const float* __restrict__ x, uint32_t x_stride, uint32_t M,
                                                             const float* __restrict__ grad_out, PlaneGrads pg, uint32_t run) {
    const int lane = lane_id();
    const int sub = lane >> 4, r = lane & 15, c = r >> 2, f = r & 3;
    const uint32_t n_sl = pg.ts.same_slice ? 1u : 2u;
    const uint32_t per_chunk = 3u * kPlaneLevels * n_sl;
    const unsigned long long item = ((unsigned long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 4ull + (unsigned)sub;
    const uint32_t chunk = (uint32_t)(item / per_chunk), rest = (uint32_t)(item - (unsigned long long)chunk * per_chunk);
    const uint32_t pl = rest / (kPlaneLevels * n_sl), l = (rest / n_sl) % kPlaneLevels, sl = rest % n_sl;
    const unsigned long long first = (unsigned long long)chunk * run;
    if (first >= M) return;
    const uint32_t m0 = (uint32_t)first, m1 = (uint32_t)(first + run < M ? first + run : M);
    float* table = sl ? pg.ts.table_hi[pl] : pg.ts.table_lo[pl];
    const float factor = pg.ts.lag[f] * (pg.ts.same_slice ? 1.0f : (sl ? pg.ts.blend_hi : pg.ts.blend_lo));
    const uint32_t ca = pl == 2 ? 1u : 0u, cb = pl == 0 ? 1u : 2u;  // coordinate columns of the pair: (x,y), (x,z), (y,z)
    walk_runs(x, x_stride, grad_out, pl * kPlaneLevels + l, m0, m1, ca, cb, pg.meta[pl], l, c, factor,
              [&](size_t row) { return table + row * kF + f; });
}

// The scalar form of the same gradient: the four features of a table entry are the four Lagrange chunks, so their gradients
// are lag_i * blend * G[row] with ONE scattered sum G[row] = sum_samples g[pair][level] * w_corner per entry (and per pair,
// shared by the two slices).  Items = (chunk, pair, level) on 4 lanes (lane = corner), 16 items per wave: a sixteenth of the
// atomic floats and a quarter of the atomic instructions of k_hash_dynamic_bwd; the host expands G to the slice gradients.
struct PlaneSums {
    float* g[3];       // per pair: fp32 [rows]
    GridMeta meta[3];
};
__global__ __launch_bounds__(kBlock) void k_hash_dynamic_bwd_scalar(const float* __restrict__ x, uint32_t x_stride, uint32_t M,
                                                                    const float* __restrict__ grad_out, PlaneSums pg, uint32_t run) {
    const int lane = lane_id();
    const int sub = lane >> 2, c = lane & 3;
    constexpr uint32_t per_chunk = 3u * kPlaneLevels;
    const unsigned long long item = ((unsigned long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 16ull + (unsigned)sub;
    const uint32_t chunk = (uint32_t)(item / per_chunk), rest = (uint32_t)(item - (unsigned long long)chunk * per_chunk);
    const uint32_t pl = rest / kPlaneLevels, l = rest % kPlaneLevels;
    const unsigned long long first = (unsigned long long)chunk * run;
    if (first >= M) return;
    const uint32_t m0 = (uint32_t)first, m1 = (uint32_t)(first + run < M ? first + run : M);
    float* table = pg.g[pl];
    const uint32_t ca = pl == 2 ? 1u : 0u, cb = pl == 0 ? 1u : 2u;
    walk_runs(x, x_stride, grad_out, pl * kPlaneLevels + l, m0, m1, ca, cb, pg.meta[pl], l, c, 1.0f, [&](size_t row) { return table + row; });
}

// The same sums through LDS (the form nvsf_hashgrid4d_dynamic_bwd_scalar launches).  A time-sliced 2-D grid has 2^13 - 2^15
// rows per level (hash_size_dynamic = [15, 13, 13], hash_field.py:96): ONE level of ONE pair is a small table of scalar sums that
// fits the 160 KB of LDS of a CU.  So a workgroup owns (pair, level, row range, slice of the samples), accumulates its slice into an
// LDS image of its rows (no memory-side atomic per sample and corner: those cost one 64-byte segment each, 2.96 ms per 1.6 M
// samples in the run-merging kernel above) and adds the image to the global sums once, with contiguous atomics (the full-rate
// shape).  The image is fp64 (ds_add_f64): an addend w g is an fp32 number, its conversion is exact, and the fp64 sum of a slice's
// addends rounds at 2^-53 of the running sum -- the arrival order of the waves changes the image by ~1e-13 of an entry, far below the
// one fp32 rounding on the way out.  (Rounds 2-5 used 64-bit fixed point, scale 2^(36 - e) from the largest |g| of the slice and
// level: that needs a pass over the gradient column before the walk.  Round 6 measured the fp64 form: config-5 step 28.9-29.2 against
// 29.5-29.7 ms on the same box -- one read of the column instead of two, a one-instruction conversion instead of the float -> int64
// sequence; the LDS fp64 adder is no slower here than the integer one was.)  A non-finite gradient (fp16 overflow under GradScaler)
// travels through the sums as through the memory-side atomics: the rows it touches end up non-finite and found_inf skips the step
// (ADVICE r3).  2^15-row levels take two workgroups per slice, one per half of the rows (128 KB each); both walk the slice, each
// keeps the addends of its rows.
template <int SPLIT>
__global__ void k_hash_dynamic_bwd_lds(const float* __restrict__ x, uint32_t x_stride, uint32_t M, const float* __restrict__ grad_out,
                                       PlaneSums pg, uint32_t pl0, uint32_t chunk_len, uint32_t go_row, uint32_t go_col) {
    // grad_out[m * go_row + column * go_col]: rows [M, 24] (24, 1) or COLUMN-major (1, M) -- a workgroup reads ONE column of all its
    // samples: 4 bytes of every 96-byte row in the row form (every line of the matrix fetched by each of the 24 columns' workgroups:
    // 2.4 GB of line traffic per 1.57 M samples), contiguous in the column form
    extern __shared__ double s_sum[];
    const uint32_t part = blockIdx.y % SPLIT, yl = blockIdx.y / SPLIT;
    const uint32_t pl = pl0 + yl / kPlaneLevels, l = yl % kPlaneLevels;
    const GridMeta& g = pg.meta[pl];
    const float scale = g.scale[l];
    const uint32_t res = g.res[l], row0 = g.offset[l], hsize = g.offset[l + 1] - row0;
    const uint32_t rows_wg = (hsize + SPLIT - 1) / SPLIT, row_lo = part * rows_wg;
    const uint32_t n_rows = row_lo < hsize ? (hsize - row_lo < rows_wg ? hsize - row_lo : rows_wg) : 0u;
    const uint32_t ca = pl == 2 ? 1u : 0u, cb = pl == 0 ? 1u : 2u;
    const unsigned long long first = (unsigned long long)blockIdx.x * chunk_len;
    const uint32_t m0 = (uint32_t)(first < M ? first : M), m1 = (uint32_t)(first + chunk_len < M ? first + chunk_len : M);
    const size_t gcol = ((size_t)pl * kPlaneLevels + l) * go_col;
    if (n_rows == 0u || m0 >= m1) return;  // uniform
    for (uint32_t i = threadIdx.x; i < n_rows; i += blockDim.x) s_sum[i] = 0.0;
    __syncthreads();
    // four samples per thread and round: their (strided, line-per-sample) loads are in flight together
    constexpr int U = 4;
    for (uint32_t mb = m0 + threadIdx.x; mb < m1; mb += U * blockDim.x) {
        float go[U], xa[U], xb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t m = mb + (uint32_t)u * blockDim.x;
            const bool ok = m < m1;
            const size_t mm = ok ? m : m0;
            go[u] = ok ? grad_out[mm * go_row + gcol] : 0.0f;
            xa[u] = x[mm * x_stride + ca];
            xb[u] = x[mm * x_stride + cb];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (go[u] == 0.0f) continue;
            const float xy[2] = {xa[u], xb[u]};
            float frac[2];
            uint32_t cell[2];
            grid_cell<2>(xy, scale, cell, frac);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float w = ((c & 1) ? frac[0] : (1.0f - frac[0])) * ((c & 2) ? frac[1] : (1.0f - frac[1]));
                const uint32_t cc[2] = {cell[0] + (uint32_t)(c & 1), cell[1] + (uint32_t)((c >> 1) & 1)};
                const uint32_t row = grid_row<2>(cc, res, hsize) - row_lo;
                const float v = w * go[u];
                if (row < n_rows && v != 0.0f) atomicAdd(&s_sum[row], (double)v);
            }
        }
    }
    __syncthreads();
    float* table = pg.g[pl] + row0 + row_lo;
    for (uint32_t i = threadIdx.x; i < n_rows; i += blockDim.x) {
        const double v = s_sum[i];
        if (v != 0.0) atomicAdd(table + i, (float)v);
    }
}

// The level tables of the three pairs from the entry points' [3][8] / [3][9] arrays
int fill_pair_metas(GridMeta (&meta)[3], const float* h_scales, const uint32_t* h_res, const uint32_t* h_offsets) {
    for (int p = 0; p < 3; ++p) {
        const int st = fill_meta(meta[p], kPlaneLevels, h_scales + p * kPlaneLevels, h_res + p * kPlaneLevels, h_offsets + p * (kPlaneLevels + 1));
        if (st != NVSF_OK) return st;
    }
    return NVSF_OK;
}

// One evaluation's time side: tables6 = lo slice of pair 0,1,2 then hi slice of pair 0,1,2; h_time = {blend_lo, blend_hi, w0, w1, w2, w3}
template <typename T, typename P>
void fill_time_set(TimeSet<T>& ts, P* const* tables6, const float* h_time, int same_slice) {
    for (int p = 0; p < 3; ++p) {
        ts.table_lo[p] = reinterpret_cast<T*>(tables6[p]);
        ts.table_hi[p] = reinterpret_cast<T*>(tables6[3 + p]);
    }
    ts.blend_lo = h_time[0]; ts.blend_hi = h_time[1];
    for (int i = 0; i < 4; ++i) ts.lag[i] = h_time[2 + i];
    ts.same_slice = same_slice;
}
// every slice it reads is there (the hi slices only when there is a blend) and aligned to `align_mask` + 1 bytes
template <typename T>
bool time_set_ok(const TimeSet<T>& ts, uintptr_t align_mask) {
    for (int p = 0; p < 3; ++p) {
        if (!(ts.table_lo[p] && (ts.same_slice || ts.table_hi[p]))) return false;
        if (((reinterpret_cast<uintptr_t>(ts.table_lo[p]) | reinterpret_cast<uintptr_t>(ts.table_hi[p])) & align_mask) != 0) return false;
    }
    return true;
}
}  // namespace

// tables: 6 device pointers (lo slice of pair 0,1,2 then hi slice of pair 0,1,2); h_scales / h_res: [3][8];
// h_offsets: [3][9]; h_time: {blend_lo, blend_hi, w0, w1, w2, w3}
NVSF_API int nvsf_hashgrid4d_dynamic_fwd(const float* x, uint32_t x_stride, const float* offset, uint32_t off_stride, uint32_t off_col,
                                         uint32_t M, const void* const* h_tables_f16, const float* h_scales, const uint32_t* h_res,
                                         const uint32_t* h_offsets, const float* h_time, int same_slice, int mode, void* out,
                                         hipStream_t stream) {
    if (M == 0) return NVSF_OK;
    REQUIRE(x && h_tables_f16 && h_time && out && x_stride >= 3 && (mode == 0 || mode == 1));
    REQUIRE(!offset || off_stride >= off_col + 3);
    PlaneSet ps;
    fill_time_set(ps.ts, h_tables_f16, h_time, same_slice);
    REQUIRE(time_set_ok(ps.ts, 7u));
    const int st = fill_pair_metas(ps.meta, h_scales, h_res, h_offsets);
    if (st != NVSF_OK) return st;
    const dim3 grid(cdiv(M, kSamplesPerBlock)), block(kBlock);
    if (mode == 0) hipLaunchKernelGGL(k_hash_dynamic<0>, grid, block, 0, stream, x, x_stride, offset, off_stride, off_col, M, ps, out);
    else hipLaunchKernelGGL(k_hash_dynamic<1>, grid, block, 0, stream, x, x_stride, offset, off_stride, off_col, M, ps, out);
    return nvsf_launch_status();
}

// Coordinate gradient of nvsf_hashgrid4d_dynamic_fwd (same arguments up to same_slice; the derivative is the same for both modes).
// grad_out fp32 rows of 24 floats, go_stride >= 24 floats apart (column 8 pair + level); grad_x fp32 [M, gx_stride >= 3], 4-byte aligned:
// written, or added to when accumulate != 0.
NVSF_API int nvsf_hashgrid4d_dynamic_grad_x(const float* x, uint32_t x_stride, const float* offset, uint32_t off_stride, uint32_t off_col,
                                            uint32_t M, const void* const* h_tables_f16, const float* h_scales, const uint32_t* h_res,
                                            const uint32_t* h_offsets, const float* h_time, int same_slice, const float* grad_out,
                                            uint32_t go_stride, float grad_scale, float* grad_x, uint32_t gx_stride, int accumulate,
                                            hipStream_t stream) {
    if (M == 0) return NVSF_OK;
    REQUIRE(x && h_tables_f16 && h_time && grad_out && grad_x && x_stride >= 3 && go_stride >= 3u * kPlaneLevels && gx_stride >= 3);
    REQUIRE(!offset || off_stride >= off_col + 3);
    REQUIRE(((reinterpret_cast<uintptr_t>(grad_out) | reinterpret_cast<uintptr_t>(grad_x)) & 3u) == 0);
    PlaneSet ps;
    fill_time_set(ps.ts, h_tables_f16, h_time, same_slice);
    REQUIRE(time_set_ok(ps.ts, 7u));
    const int st = fill_pair_metas(ps.meta, h_scales, h_res, h_offsets);
    if (st != NVSF_OK) return st;
    hipLaunchKernelGGL(k_hash_dynamic_grad_x, dim3(cdiv(M, kSamplesPerBlock)), dim3(kBlock), 0, stream, x, x_stride, offset, off_stride, off_col,
                       M, ps, grad_out, go_stride, grad_scale, grad_x, gx_stride, accumulate);
    return nvsf_launch_status();
}

NVSF_API int nvsf_hashgrid3d_lagrange_fwd(const float* x, uint32_t x_stride, uint32_t M, const void* table_f16, uint32_t L, uint32_t F,
                                          const float* h_scales, const uint32_t* h_res, const uint32_t* h_offsets, const float* h_weights4,
                                          float* out, hipStream_t stream) {
    if (M == 0) return NVSF_OK;
    REQUIRE(x && table_f16 && h_weights4 && out && x_stride >= 3);
    if (F != 8) return NVSF_ERR_UNSUPPORTED;
    GridMeta meta;
    const int st = fill_meta(meta, L, h_scales, h_res, h_offsets);
    if (st != NVSF_OK) return st;
    const size_t lds = (size_t)kSamplesPerBlock * (2 * L + 1) * sizeof(float);
    hipLaunchKernelGGL(k_hash3d_lagrange, dim3(cdiv(M, kSamplesPerBlock)), dim3(kBlock), lds, stream, x, x_stride, M,
                       reinterpret_cast<const _Float16*>(table_f16), L, meta, h_weights4[0], h_weights4[1], h_weights4[2], h_weights4[3], out);
    return nvsf_launch_status();
}

// grad tables: 6 device pointers to fp32 buffers in the layout of the slice tables (lo slice of pair 0,1,2 then hi slice of pair 0,1,2;
// the hi pointers are ignored when same_slice); dL/dtable is ADDED to them.  grad_out fp32 [M, 24] (regime 0 only).
NVSF_API int nvsf_hashgrid4d_dynamic_bwd(const float* x, uint32_t x_stride, uint32_t M, const float* h_scales, const uint32_t* h_res,
                                         const uint32_t* h_offsets, const float* h_time, int same_slice, const float* grad_out,
                                         void* const* h_grad_tables_f32, hipStream_t stream) {
    if (M == 0) return NVSF_OK;
    REQUIRE(x && h_time && grad_out && h_grad_tables_f32 && x_stride >= 3);
    PlaneGrads pg;
    fill_time_set(pg.ts, h_grad_tables_f32, h_time, same_slice);
    REQUIRE(time_set_ok(pg.ts, 0u));
    const int st = fill_pair_metas(pg.meta, h_scales, h_res, h_offsets);
    if (st != NVSF_OK) return st;
    const uint32_t run = M >= (1u << 20) ? 128u : 32u;
    const unsigned long long items = (unsigned long long)cdiv(M, run) * 3ull * kPlaneLevels * (same_slice ? 1u : 2u);
    const unsigned long long waves = (items + 3) / 4;
    hipLaunchKernelGGL(k_hash_dynamic_bwd, dim3((uint32_t)((waves + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, stream, x, x_stride, M,
                       grad_out, pg, run);
    return nvsf_launch_status();
}

// The three evaluations of one density query.  h_tables_f16: 18 device pointers = for evaluation e = 0, 1, 2: lo slice of pair 0,1,2 then
// hi slice of pair 0,1,2; h_time: 18 floats = per evaluation {blend_lo, blend_hi, w0, w1, w2, w3}; h_flags: 9 ints = per evaluation
// {enabled, same_slice, shares the slice tables of evaluation 0}.  out0 fp32 [M,24] (regime 0), out1 / out2 fp16 [M,24] (regime 1).
// offsets fp32 [M, off_stride >= 6]: columns 0..2 warp evaluation 1, columns 3..5 evaluation 2.
NVSF_API int nvsf_hashgrid4d_dynamic3_fwd(const float* x, uint32_t x_stride, const float* offsets, uint32_t off_stride, uint32_t M,
                                          const void* const* h_tables_f16, const float* h_scales, const uint32_t* h_res,
                                          const uint32_t* h_offsets, const float* h_time, const int* h_flags, float* out0, void* out1,
                                          void* out2, hipStream_t stream) {
    if (M == 0) return NVSF_OK;
    REQUIRE(x && h_tables_f16 && h_time && h_flags && out0 && x_stride >= 3);
    PlaneSet3 ps;
    const int st = fill_pair_metas(ps.meta, h_scales, h_res, h_offsets);
    if (st != NVSF_OK) return st;
    for (int e = 0; e < 3; ++e) {
        ps.enabled[e] = e == 0 ? 1 : h_flags[3 * e];
        ps.share[e] = h_flags[3 * e + 2];
        TimeSet<const _Float16>& pe = ps.ev[e];
        fill_time_set(pe, h_tables_f16 + 6 * e, h_time + 6 * e, h_flags[3 * e + 1]);
        if (ps.enabled[e]) REQUIRE(time_set_ok(pe, 7u));
        if (e > 0 && ps.enabled[e]) {
            REQUIRE(offsets && off_stride >= 6 && (e == 1 ? out1 : out2));
            if (ps.share[e]) REQUIRE(pe.same_slice == ps.ev[0].same_slice);
        }
    }
    hipLaunchKernelGGL(k_hash_dynamic3, dim3(cdiv(M, kSamplesPerBlock)), dim3(kBlock), 0, stream, x, x_stride, offsets, off_stride, M, ps, out0,
                       reinterpret_cast<_Float16*>(out1), reinterpret_cast<_Float16*>(out2));
    return nvsf_launch_status();
}

// Scalar table-gradient sums of the space-time encoder: h_sums_f32 = 3 device pointers (one per pair) to fp32 [rows] buffers; the sum
// G[row] = sum over samples of grad_out[pair][level] * w_corner is ADDED to them.  dL/dtable[slice][row][i] = lag_i * blend_slice * G[row].
static int hash4d_bwd_scalar_impl(const float* x, uint32_t x_stride, uint32_t M, const float* h_scales, const uint32_t* h_res,
                                  const uint32_t* h_offsets, const float* grad_out, int grad_col_major, void* const* h_sums_f32, hipStream_t stream) {
    if (M == 0) return NVSF_OK;
    REQUIRE(x && grad_out && h_sums_f32 && x_stride >= 3);
    PlaneSums pg;
    for (int p = 0; p < 3; ++p) {
        pg.g[p] = reinterpret_cast<float*>(h_sums_f32[p]);
        REQUIRE(pg.g[p]);
    }
    const int st = fill_pair_metas(pg.meta, h_scales, h_res, h_offsets);
    if (st != NVSF_OK) return st;
    // LDS form: one launch per group of pairs with the same level size (pair 0: 2^15 rows = two row ranges of 128 KB of 64-bit sums,
    // 1024-thread workgroups; pairs 1, 2: 2^13 rows = 64 KB, 512 threads).  Variant 1 (tests) selects the run-merging global-atomic
    // kernel (the reference form; also taken when a level does not fit LDS or the batch is too small to fill the chip with slices).
    uint32_t max_rows[3];
    bool fits = true;
    for (int p = 0; p < 3; ++p) {
        max_rows[p] = 0;
        for (uint32_t l = 0; l < (uint32_t)kPlaneLevels; ++l) {
            const uint32_t rows = pg.meta[p].offset[l + 1] - pg.meta[p].offset[l];
            max_rows[p] = rows > max_rows[p] ? rows : max_rows[p];
        }
        fits = fits && max_rows[p] * sizeof(double) <= 2u * 128u * 1024u;
    }
    const uint32_t go_row = grad_col_major ? 1u : (uint32_t)(3 * kPlaneLevels), go_col = grad_col_major ? M : 1u;
    if (!(fits && M >= (1u << 16) && nvsf_variant(kVarHash4dBwd) == 0) && grad_col_major) return NVSF_ERR_UNSUPPORTED;  // rows for the other kernel
    if (fits && M >= (1u << 16) && nvsf_variant(kVarHash4dBwd) == 0) {
        int p = 0;
        while (p < 3) {
            int q = p + 1;
            while (q < 3 && max_rows[q] == max_rows[p]) ++q;  // consecutive pairs with equal level size share a launch
            const uint32_t split = max_rows[p] * (uint32_t)sizeof(double) > 128u * 1024u ? 2u : 1u;
            const uint32_t lds = (max_rows[p] + split - 1) / split * (uint32_t)sizeof(double);
            const uint32_t threads = lds > 64u * 1024u ? 1024u : 512u;
            const uint32_t n_slices = lds > 64u * 1024u ? 32u : 64u;
            const uint32_t chunk_len = (M + n_slices - 1) / n_slices;
            const dim3 grid(n_slices, (uint32_t)(q - p) * kPlaneLevels * split);
            if (split == 2)
                hipLaunchKernelGGL(k_hash_dynamic_bwd_lds<2>, grid, dim3(threads), lds, stream, x, x_stride, M, grad_out, pg, (uint32_t)p, chunk_len, go_row, go_col);
            else
                hipLaunchKernelGGL(k_hash_dynamic_bwd_lds<1>, grid, dim3(threads), lds, stream, x, x_stride, M, grad_out, pg, (uint32_t)p, chunk_len, go_row, go_col);
            p = q;
        }
        return nvsf_launch_status();
    }
    const uint32_t run = M >= (1u << 20) ? 128u : 32u;
    const unsigned long long items = (unsigned long long)cdiv(M, run) * 3ull * kPlaneLevels;
    const unsigned long long waves = (items + 15) / 16;
    hipLaunchKernelGGL(k_hash_dynamic_bwd_scalar, dim3((uint32_t)((waves + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, stream, x, x_stride,
                       M, grad_out, pg, run);
    return nvsf_launch_status();
}

NVSF_API int nvsf_hashgrid4d_dynamic_bwd_scalar(const float* x, uint32_t x_stride, uint32_t M, const float* h_scales, const uint32_t* h_res,
                                                const uint32_t* h_offsets, const float* grad_out, void* const* h_sums_f32, hipStream_t stream) {
    return hash4d_bwd_scalar_impl(x, x_stride, M, h_scales, h_res, h_offsets, grad_out, 0, h_sums_f32, stream);
}

// The same with the gradient COLUMN-major, fp32 [24][M] (what nvsf_density_tail_grad_split writes): the LDS kernel's workgroups read one
// column each.  NVSF_ERR_UNSUPPORTED where the launch would take the run-merging kernel (small batches, levels beyond LDS, test variant):
// the caller then passes rows.
NVSF_API int nvsf_hashgrid4d_dynamic_bwd_scalar_t(const float* x, uint32_t x_stride, uint32_t M, const float* h_scales, const uint32_t* h_res,
                                                  const uint32_t* h_offsets, const float* grad_out_t, void* const* h_sums_f32, hipStream_t stream) {
    return hash4d_bwd_scalar_impl(x, x_stride, M, h_scales, h_res, h_offsets, grad_out_t, 1, h_sums_f32, stream);
}
