// Device-side building blocks of the multiresolution hash-grid encoding (shared by hashgrid.hip and the
// fused field kernels).  Specification: DESIGN.md section 4.1 (restates Instant-NGP sec. 3 / the tcnn
// "HashGrid" encoding the reference instantiates at hash_field.py:47-57,109-119 and flow_field.py:70-80).
#pragma once
#include "common.h"
#include <hip/hip_fp16.h>

constexpr int kMaxLevels = 32;

// Per-level metadata, computed on the host once per encoder and passed by value (kernarg -> SGPRs).
struct GridMeta {
    float scale[kMaxLevels];        // exp2(l*log2(per_level_scale))*base_resolution - 1
    uint32_t res[kMaxLevels];       // ceil(scale)+1
    uint32_t offset[kMaxLevels + 1];  // first feature-vector row of each level; offset[L] = total rows
};

// Host: the level table of an entry point's (scales, res, offsets) arrays, checked
static inline int fill_meta(GridMeta& meta, uint32_t L, const float* scales, const uint32_t* res, const uint32_t* offsets) {
    if (L == 0 || L > (uint32_t)kMaxLevels || !scales || !res || !offsets) return NVSF_ERR_INVALID_ARG;
    for (uint32_t l = 0; l < L; ++l) {
        meta.scale[l] = scales[l];
        meta.res[l] = res[l];
        meta.offset[l] = offsets[l];
        if (offsets[l + 1] <= offsets[l] || res[l] == 0) return NVSF_ERR_INVALID_ARG;
    }
    meta.offset[L] = offsets[L];
    return NVSF_OK;
}

typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));

template <int F> struct FeatVec;
template <> struct FeatVec<1> { typedef _Float16 type; };
template <> struct FeatVec<2> { typedef h2_t type; };
template <> struct FeatVec<4> { typedef h4_t type; };
template <> struct FeatVec<8> { typedef h8_t type; };

template <int F>
__device__ __forceinline__ void load_feat(const _Float16* __restrict__ table, size_t row, float (&v)[F]) {
    if constexpr (F == 1) {
        v[0] = (float)table[row];
    } else {
        typedef typename FeatVec<F>::type vec_t;
        const vec_t t = *reinterpret_cast<const vec_t*>(table + row * F);
#pragma unroll
        for (int f = 0; f < F; ++f) v[f] = (float)t[f];
    }
}

// Element i of a gradient matrix that arrives as fp16 or fp32
template <bool GRAD_F16>
__device__ __forceinline__ float load_grad(const void* __restrict__ g, size_t i) {
    if constexpr (GRAD_F16) return (float)reinterpret_cast<const _Float16*>(g)[i];
    else return reinterpret_cast<const float*>(g)[i];
}

// Cell and position inside the cell of a sample at one level: pos = scale * x + 0.5 (one fma), cell = floor(pos), frac = pos - cell
template <int D>
__device__ __forceinline__ void grid_cell(const float (&x)[D], float scale, uint32_t (&cell)[D], float (&frac)[D]) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float pos = fmaf(scale, x[d], 0.5f);
        const float fl = floorf(pos);
        frac[d] = pos - fl;
        cell[d] = (uint32_t)(int32_t)fl;
    }
}

template <int D>
__device__ __forceinline__ uint32_t grid_row(const uint32_t (&cell)[D], uint32_t res, uint32_t hsize) {
    // dense index while res^d still fits the level's table, spatial hash otherwise
    unsigned long long stride = 1;
    uint32_t index = 0;
    bool dense = true;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        if (stride <= hsize) {
            index += cell[d] * (uint32_t)stride;
            stride *= res;
        } else {
            dense = false;
        }
    }
    if (!dense || hsize < stride) {
        constexpr uint32_t primes[3] = {1u, 2654435761u, 805459861u};
        index = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) index ^= cell[d] * primes[d];
    }
    // table sizes of hashed levels are powers of two: avoid the integer division on the hot path
    return (hsize & (hsize - 1u)) == 0u ? (index & (hsize - 1u)) : (index % hsize);
}

// ---- The fast forms of grid_row<3> and of the blend, shared by the gather kernels of fused_field.hip, hashgrid.hip and hashgrid4d.hip ----
// The kind of a level (dense or hashed) is decided once by the caller, for a position inside the unit cube.  N rows of the cell c:
// N = 8: its eight corners in the specification's order k = x + 2 y + 4 z (xb = 0); N = 4: the four corners with x-bit xb, in the order
// p = y + 2 z (the two-lanes-per-sample kernels: lane = 2 * sample + xb); N = 1: the corner c itself (xb = 0).
//
// dense_rows: c0 + c1 res + c2 res^2, wrapped by ONE conditional subtract (the index is below 2 * rows inside the unit cube).
template <int N>
__device__ __forceinline__ void dense_rows(const uint32_t (&c)[3], uint32_t xb, uint32_t res, uint32_t res2, uint32_t rows, uint32_t (&idx)[N]) {
    static_assert(N == 8 || N == 4 || N == 1, "the cell, one x-half of it, or one corner");
    constexpr int NX = N == 8 ? 2 : 1;
    const uint32_t b00 = c[0] + c[1] * res + c[2] * res2;
    const uint32_t b10 = b00 + res, b01 = b00 + res2, b11 = b10 + res2;
    const uint32_t base[4] = {b00, b10, b01, b11};
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const uint32_t v = base[k / NX] + (xb + (uint32_t)(k % NX));
        idx[k] = v >= rows ? v - rows : v;
    }
}

// hashed_rows: (x ^ y P1 ^ z P2) & mask with the y/z terms of the four (y, z) pairs shared by the x-neighbours; mask = rows - 1 (hashed
// levels are powers of two)
template <int N>
__device__ __forceinline__ void hashed_rows(const uint32_t (&c)[3], uint32_t xb, uint32_t mask, uint32_t (&idx)[N]) {
    static_assert(N == 8 || N == 4 || N == 1, "the cell, one x-half of it, or one corner");
    constexpr int NX = N == 8 ? 2 : 1;
    const uint32_t hy0 = c[1] * 2654435761u, hy1 = hy0 + 2654435761u;
    const uint32_t hz0 = c[2] * 805459861u, hz1 = hz0 + 805459861u;
    const uint32_t yz[4] = {hy0 ^ hz0, hy1 ^ hz0, hy0 ^ hz1, hy1 ^ hz1};
#pragma unroll
    for (int k = 0; k < N; ++k) idx[k] = ((c[0] + (xb + (uint32_t)(k % NX))) ^ yz[k / NX]) & mask;
}

// Partner exchange of the two-lanes-per-sample kernels.  The lane with x-bit xb holds NP gathered entries of two dwords (the corners
// with its x-bit); it keeps dword xb of each and receives dword xb of the partner's entries (the corners with the other x-bit) by
// lane_swap: mine[2 p + x] = dword xb of the entry of corner (x, p), i.e. this lane's feature pair in the specification's corner order.
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
template <int NP>
__device__ __forceinline__ void exchange_halves(const u32x2_t (&raw)[NP], uint32_t xb, uint32_t (&mine)[2 * NP]) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const uint32_t own = xb ? raw[p][1] : raw[p][0], send = xb ? raw[p][0] : raw[p][1];
        const uint32_t recv = lane_swap(send);
        mine[2 * p] = xb ? recv : own;
        mine[2 * p + 1] = xb ? own : recv;
    }
}

// Trilinear weight of corner k = x + 2 y + 4 z in the specification's product order, (wx wy) wz (encode_level's 1 * wx is exact)
__device__ __forceinline__ float corner_weight(int k, const float (&frac)[3]) {
    const float wx[2] = {1.0f - frac[0], frac[0]}, wy[2] = {1.0f - frac[1], frac[1]}, wz[2] = {1.0f - frac[2], frac[2]};
    return (wx[k & 1] * wy[(k >> 1) & 1]) * wz[k >> 2];
}

// What the level-sliced encode passes keep of one level (block-uniform: SGPRs)
template <int F>
struct SliceLevel {
    float scale;
    uint32_t res, res2, boff, rows;
    bool hashed;
};
template <int F>
__device__ __forceinline__ SliceLevel<F> slice_level(const GridMeta& meta, uint32_t l, uint32_t first_hashed) {
    SliceLevel<F> lv;
    lv.scale = meta.scale[l];
    lv.res = meta.res[l];
    lv.res2 = meta.res[l] * meta.res[l];
    lv.boff = meta.offset[l] * (uint32_t)(F * sizeof(_Float16));
    lv.rows = meta.offset[l + 1] - meta.offset[l];
    lv.hashed = l >= first_hashed;
    return lv;
}

// The inputs of sample s the ray-fed encode passes hand on: its depth, and (training) its unit-cube position
__device__ __forceinline__ void store_sample_inputs(float* __restrict__ z_vals, float* __restrict__ x01, uint32_t s, float z, const float (&x)[3]) {
    z_vals[s] = z;
    if (x01) { x01[3 * (size_t)s] = x[0]; x01[3 * (size_t)s + 1] = x[1]; x01[3 * (size_t)s + 2] = x[2]; }
}

// Encodes one sample at one level: acc[f] = sum_c w_c * table[row_c][f]  (fp32 fmaf chain, corner order c)
template <int D, int F>
__device__ __forceinline__ void encode_level(const float (&x)[D], const _Float16* __restrict__ table, float scale,
                                             uint32_t res, uint32_t row0, uint32_t hsize, float (&acc)[F]) {
    float frac[D];
    uint32_t cell[D];
    grid_cell<D>(x, scale, cell, frac);
#pragma unroll
    for (int f = 0; f < F; ++f) acc[f] = 0.0f;
    // issue all 2^D gathers first, then blend (keeps 2^D loads in flight per lane)
    float v[1 << D][F];
    float w[1 << D];
#pragma unroll
    for (int c = 0; c < (1 << D); ++c) {
        uint32_t cc[D];
        float wc = 1.0f;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (c & (1 << d)) { wc = wc * frac[d]; cc[d] = cell[d] + 1u; }
            else { wc = wc * (1.0f - frac[d]); cc[d] = cell[d]; }
        }
        w[c] = wc;
        load_feat<F>(table, (size_t)row0 + grid_row<D>(cc, res, hsize), v[c]);
    }
#pragma unroll
    for (int c = 0; c < (1 << D); ++c)
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = fmaf(w[c], v[c][f], acc[f]);
}
