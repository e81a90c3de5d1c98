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
