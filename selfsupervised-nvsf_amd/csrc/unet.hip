// Evaluation-mode forward of the ray-drop refinement U-Net (the reference's nvsf/nerf/models/unet.py, channels = 32) for one frame, gfx950.
// include/nvsf_hip.h section 13.  Activations and weights are fp32 and every product runs on the f32-input matrix instruction
// v_mfma_f32_32x32x2_f32: exact fp32, a k-ordered fma chain per output element.
//
// k_conv: implicit GEMM of a 3 x 3 (padding 1) or 1 x 1 convolution over one CHW frame.  A workgroup of four waves owns 4 rows x 32
// columns of output pixels and 32 or 64 output channels; wave w owns row w.  Per chunk of 16 input channels the workgroup stages in LDS
//   - the (4 + 2) x (32 + 2) input patch of every channel of the chunk, ALREADY normalised: the eval-mode BatchNorm folded to a
//     per-channel scale and shift, then the ReLU, are applied by the load (the convolution's own zero padding is applied after them,
//     as torch pads the normalised tensor).  The load also does the work of the layer in front of the convolution: MaxPool2d(2) (kPool),
//     or bilinear x2 upsampling with align_corners, the zero pad to the skip's size and the channel concatenation (kUpCat);
//   - the chunk's weights [channel][tap][output channel].
// The MFMA computes D[co][x] = sum_k Wt[co][k] P[k][x]: A operand = weights (row co on the lane, the two k = two input channels on the
// lane halves), B operand = the patch (column x on the lane); one LDS read each, conflict-free (the two lane halves read planes whose
// distance is 32 mod 64 words).  The result has x on the lane, so every store of the epilogue is one contiguous 128-byte row.
// k order of a chunk: channel pair, then tap; chunks in channel order.
//
// k_attn: the attention block's two products for one head and 32 queries per wave, keys in blocks of 32 with the running-maximum
// form of the softmax.  S^T = K^T Q leaves the query on the lane and the keys in the accumulator registers, so the softmax statistics are
// lane-local (+ one exchange between the lane halves) and P^T is directly the B operand of O^T += V^T P^T.  The result is written through
// the reference's reinterpretation of [8, HW, 32] as [H, W, 256].
//
// k_head: BatchNorm + ReLU + the 32 -> 1 convolution + sigmoid + the ray-drop gate of intensity and range, one thread per pixel.
#include "common.h"
#include <math.h>

namespace {
using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kTH = 4, kTW = 32;  // output tile of a workgroup: rows (one per wave) x columns (one MFMA column block)
constexpr int kKC = 16;           // input channels per staged chunk
constexpr int kBlock = 256;
enum { kPlain = 0, kPool = 1, kUpCat = 2, kPlanes = 3 };

// smallest m >= n with m = 32 (mod 64): the LDS plane stride that puts the two lane halves of a wave on disjoint banks
constexpr int pad32(int n) { return ((n + 31) / 64) * 64 + 32; }

struct ConvArgs {
    const float* in0;    // kPlain: [Cin, H, W]; kPool: [Cin, Hs, Ws]; kUpCat: the skip [C0, H, W]; kPlanes: plane 0
    const float* in1;    // kUpCat: the coarse tensor [Cin - C0, Hs, Ws]; kPlanes: plane 1
    const float* in2;    // kPlanes: plane 2
    const float* scale;  // [>= Cin] folded BatchNorm of the input
    const float* shift;
    const float* bias;   // [Cout]
    const float* w;      // [roundup(Cin, kKC) * T, Cout], row = channel * T + tap
    const float* resid;  // [Cout, H, W] added to the result, or null
    float* out;          // [Cout, H, W]
    int Cin, Cout, H, W;
    int C0, Hs, Ws, padT, padL;
    float sy, sx;        // (Hs - 1) / (2 Hs - 1), (Ws - 1) / (2 Ws - 1) in fp32
    int relu;
};

// One element of the input patch in flight: what fetch() read for it (1 value, or the 2 x 2 neighbourhood of the pool / the bilinear
// sample) and its channel's scale and shift.  finish() turns it into the value the convolution sees: 0 outside the image (the
// convolution's own padding), else act(scale * source + shift).  The two halves are apart so that a chunk's loads are in flight while the
// matrix cores work on the chunk before it.
template <int MODE>
struct Raw {
    float v[(MODE == kPool || MODE == kUpCat) ? 4 : 1];
    float sc, sh;
};

__device__ __forceinline__ bool inside(const ConvArgs& a, int ci, int y, int x) {
    return ci < a.Cin && y >= 0 && y < a.H && x >= 0 && x < a.W;
}

template <int MODE>
__device__ __forceinline__ Raw<MODE> fetch(const ConvArgs& a, int ci, int y, int x) {
    Raw<MODE> r;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(r.v) / sizeof(float)); ++i) r.v[i] = 0.0f;
    r.sc = 0.0f; r.sh = 0.0f;
    if (!inside(a, ci, y, x)) return r;
    r.sc = a.scale[ci]; r.sh = a.shift[ci];
    if (MODE == kPlain) {
        r.v[0] = a.in0[(ci * a.H + y) * a.W + x];
    } else if (MODE == kPlanes) {
        const float* p = ci == 0 ? a.in0 : (ci == 1 ? a.in1 : a.in2);
        r.v[0] = p[y * a.W + x];
    } else if (MODE == kPool) {  // H = Hs / 2, W = Ws / 2 (floor): rows 2y, 2y + 1 and columns 2x, 2x + 1 exist
        const float* p = a.in0 + (ci * a.Hs + 2 * y) * a.Ws + 2 * x;
        r.v[0] = p[0]; r.v[1] = p[1]; r.v[2] = p[a.Ws]; r.v[3] = p[a.Ws + 1];
    } else {
        if (ci < a.C0) {
            r.v[0] = a.in0[(ci * a.H + y) * a.W + x];
        } else {
            const int uy = y - a.padT, ux = x - a.padL;
            if (uy >= 0 && uy < 2 * a.Hs && ux >= 0 && ux < 2 * a.Ws) {  // else F.pad's zeros
                const int iy = (int)(a.sy * (float)uy), ix = (int)(a.sx * (float)ux);
                const int dy = iy < a.Hs - 1 ? a.Ws : 0, dx = ix < a.Ws - 1 ? 1 : 0;
                const float* p = a.in1 + ((ci - a.C0) * a.Hs + iy) * a.Ws + ix;
                r.v[0] = p[0]; r.v[1] = p[dx]; r.v[2] = p[dy]; r.v[3] = p[dy + dx];
            }
        }
    }
    return r;
}

template <int MODE>
__device__ __forceinline__ float finish(const ConvArgs& a, const Raw<MODE>& r, int ci, int y, int x) {
    if (!inside(a, ci, y, x)) return 0.0f;
    float v = r.v[0];
    if (MODE == kPool) {
        v = fmaxf(fmaxf(r.v[0], r.v[1]), fmaxf(r.v[2], r.v[3]));
    } else if (MODE == kUpCat) {
        if (ci >= a.C0) {  // upsample_bilinear2d, align_corners: source = scale * index, formed in fp32; F.pad's zeros give 0 here,
                           // in front of the BatchNorm, so they are normalised like any other value
            const int uy = y - a.padT, ux = x - a.padL;
            const float fy = a.sy * (float)uy, fx = a.sx * (float)ux;
            const float ly1 = fy - (float)(int)fy, lx1 = fx - (float)(int)fx, ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
            v = ly0 * (lx0 * r.v[0] + lx1 * r.v[1]) + ly1 * (lx0 * r.v[2] + lx1 * r.v[3]);
        }
    }
    v = v * r.sc + r.sh;
    return a.relu ? fmaxf(v, 0.0f) : v;
}

template <int KS, int MODE, int CB>
__global__ __launch_bounds__(kBlock) void k_conv(const ConvArgs a) {
    constexpr int R = KS / 2, T = KS * KS, PH = kTH + 2 * R, PW = kTW + 2 * R, PS = pad32(PH * PW), CO = 32 * CB, WS = pad32(T * CO);
    constexpr int NPE = kKC * PH * PW, NP = (NPE + kBlock - 1) / kBlock;          // patch elements of a chunk, per thread
    constexpr int NWE = kKC * T * (CO / 4), NW = (NWE + kBlock - 1) / kBlock;     // float4 of a chunk's weights, per thread
    __shared__ __attribute__((aligned(16))) float sp[kKC * PS];
    __shared__ __attribute__((aligned(16))) float sw[kKC * WS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, xl = lane & 31, h = lane >> 5;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH, co0 = blockIdx.z * CO;
    f32x16 acc[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;

    Raw<MODE> pr[NP];
    float4 wr[NW];
    auto fetch_chunk = [&](int c0) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int e = tid + i * kBlock, ci = e / (PH * PW), r = e - ci * (PH * PW), py = r / PW, px = r - py * PW;
            pr[i] = fetch<MODE>(a, e < NPE ? c0 + ci : a.Cin, y0 + py - R, x0 + px - R);
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int e = tid + i * kBlock, row = e / (CO / 4), q = e - row * (CO / 4), co = co0 + 4 * q;
            wr[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (e < NWE && co < a.Cout) wr[i] = *reinterpret_cast<const float4*>(a.w + (size_t)(c0 * T + row) * a.Cout + co);  // Cout % 4 == 0
        }
    };
    auto store_chunk = [&](int c0) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int e = tid + i * kBlock, ci = e / (PH * PW), r = e - ci * (PH * PW), py = r / PW, px = r - py * PW;
            if (e < NPE) sp[ci * PS + r] = finish<MODE>(a, pr[i], c0 + ci, y0 + py - R, x0 + px - R);
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int e = tid + i * kBlock, row = e / (CO / 4), q = e - row * (CO / 4), ci = row / T, tap = row - ci * T;
            if (e < NWE) *reinterpret_cast<float4*>(sw + ci * WS + tap * CO + 4 * q) = wr[i];
        }
    };

    fetch_chunk(0);
    for (int c0 = 0; c0 < a.Cin; c0 += kKC) {
        store_chunk(c0);
        __syncthreads();
        if (c0 + kKC < a.Cin) fetch_chunk(c0 + kKC);  // in flight during the products below
#pragma unroll 2
        for (int s = 0; s < kKC / 2; ++s) {
            const float* pp = sp + (2 * s + h) * PS + wave * PW + xl;
            const float* wp = sw + (2 * s + h) * WS + xl;
#pragma unroll
            for (int tap = 0; tap < T; ++tap) {
                const float b = pp[(tap / KS) * PW + (tap % KS)];
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
                    acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wp[tap * CO + 32 * cb], b, acc[cb], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    const int y = y0 + wave, x = x0 + xl;
    if (y >= a.H || x >= a.W) return;
    const int hw = a.H * a.W;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + 32 * cb + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (co < a.Cout) {
                const int idx = co * hw + y * a.W + x;
                float v = acc[cb][r] + a.bias[co];
                if (a.resid) v += a.resid[idx];
                a.out[idx] = v;
            }
        }
}

// qkv [768, N]: q, k, v of head hd in rows hd * 32 ... + 32 of their thirds.  out [256, N] = the reference's
// `h.view(B, H, W, C).permute(0, 3, 1, 2)` of the [8, N, 32] attention result.  One wave per (32 queries, head).
__global__ __launch_bounds__(64) void k_attn(const float* __restrict__ qkv, float* __restrict__ out, int N, float scale) {
    const int lane = threadIdx.x, xl = lane & 31, h = lane >> 5;
    const int hd = blockIdx.y, n = blockIdx.x * 32 + xl;
    const float* q = qkv + (size_t)(hd * 32) * N;
    const float* k = qkv + (size_t)(256 + hd * 32) * N;
    const float* v = qkv + (size_t)(512 + hd * 32) * N;
    float qr[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) qr[s] = n < N ? q[(size_t)(2 * s + h) * N + n] : 0.0f;
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.0f;
    float mrun = -INFINITY, lrun = 0.0f;
    for (int mb = 0; mb < N; mb += 32) {
        // S^T[m][n] = sum_c k[c][m] q[c][n]: keys in the registers (row (r & 3) + 8 (r >> 2) + 4 h), the query on the lane
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.0f;
        const int m = mb + xl;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float kv = m < N ? k[(size_t)(2 * s + h) * N + m] : 0.0f;
            st = __builtin_amdgcn_mfma_f32_32x32x2f32(kv, qr[s], st, 0, 0, 0);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int mm = mb + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float sv = mm < N ? st[r] * scale : -INFINITY;
            st[r] = sv;
            mx = fmaxf(mx, sv);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mnew = fmaxf(mrun, mx);      // finite: key mb exists
        const float alpha = expf(mrun - mnew);   // first block: exp(-inf) = 0
        float ps = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = expf(st[r] - mnew);
            st[r] = p;
            ps += p;
        }
        ps += __shfl_xor(ps, 32, 64);
        lrun = lrun * alpha + ps;
        mrun = mnew;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] *= alpha;
        // O^T[c][n] += sum_m v[c][m] P^T[m][n]: register r of the two lane halves holds keys m and m + 4 = the two k of one step
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int mm = mb + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float vv = mm < N ? v[(size_t)xl * N + mm] : 0.0f;
            o = __builtin_amdgcn_mfma_f32_32x32x2f32(vv, st[r], o, 0, 0, 0);
        }
    }
    if (n >= N) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int c = (r & 3) + 8 * (r >> 2) + 4 * h;
        const int f = (hd * N + n) * 32 + c;  // flat index of [8, N, 32], read back as [N, 256]
        out[(size_t)(f & 255) * N + (f >> 8)] = o[r] / lrun;
    }
}

// rec: scale [32], shift [32], bias [1], w [32]
__global__ __launch_bounds__(kBlock) void k_head(const float* __restrict__ x, const float* __restrict__ rec, const float* __restrict__ intensity,
                                                const float* __restrict__ range, int hw, float thres, float* __restrict__ prob,
                                                float* __restrict__ gi, float* __restrict__ gr) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= hw) return;
    float s = 0.0f;
#pragma unroll 8
    for (int c = 0; c < 32; ++c) {
        const float v = fmaxf(x[(size_t)c * hw + p] * rec[c] + rec[32 + c], 0.0f);
        s = fmaf(v, rec[65 + c], s);
    }
    s += rec[64];
    const float pr = 1.0f / (1.0f + expf(-s));
    prob[p] = pr;
    if (gi) {
        const float m = pr > thres ? 1.0f : 0.0f;  // a product, as the reference's `pred * raydrop_mask`
        gi[p] = intensity[p] * m;
        gr[p] = range[p] * m;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
struct Layer { int cin, t, cout; };
// order of the packed records (nvsf/nerf/refine.py packs in the same order)
constexpr Layer kLayers[20] = {
    {3, 1, 32},                                                                                  // inc
    {32, 9, 64}, {64, 9, 64}, {64, 9, 128}, {128, 9, 128}, {128, 9, 256}, {256, 9, 256}, {256, 9, 256}, {256, 9, 256},  // down1..4
    {256, 1, 768}, {256, 1, 256},                                                                // attention: qkv, proj
    {512, 9, 512}, {512, 9, 128}, {256, 9, 256}, {256, 9, 64}, {128, 9, 128}, {128, 9, 32}, {64, 9, 64}, {64, 9, 32},  // up1..4
    {32, 1, 1},                                                                                  // outc
};
constexpr size_t cin_pad(int cin) { return (size_t)((cin + kKC - 1) / kKC) * kKC; }
constexpr size_t rec_floats(const Layer& l) { return 2 * cin_pad(l.cin) + (size_t)l.cout + cin_pad(l.cin) * l.t * l.cout; }

size_t packed_floats() {
    size_t n = 0;
    for (const Layer& l : kLayers) n += rec_floats(l);
    return n;
}

struct Plan {
    int H[5], W[5];
    size_t x[5], mid, att, qkv, x4a, u[4], total;  // offsets in floats
};
constexpr int kC[5] = {32, 64, 128, 256, 256};
constexpr int kUpOut[4] = {128, 64, 32, 32};  // up1..up4

bool make_plan(uint32_t H, uint32_t W, Plan& p) {
    if (H < 16 || W < 16 || (uint64_t)H * W > (1u << 21)) return false;
    p.H[0] = (int)H; p.W[0] = (int)W;
    for (int l = 1; l < 5; ++l) { p.H[l] = p.H[l - 1] / 2; p.W[l] = p.W[l - 1] / 2; }
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += (n + 63) / 64 * 64; return o; };
    size_t px[5];
    for (int l = 0; l < 5; ++l) { px[l] = (size_t)p.H[l] * p.W[l]; p.x[l] = take(kC[l] * px[l]); }
    size_t mid = 64 * px[0];
    if (128 * px[1] > mid) mid = 128 * px[1];
    if (256 * px[2] > mid) mid = 256 * px[2];
    if (512 * px[3] > mid) mid = 512 * px[3];
    if (256 * px[4] > mid) mid = 256 * px[4];
    p.mid = take(mid);
    p.qkv = take(768 * px[4]);
    p.att = take(256 * px[4]);
    p.x4a = take(256 * px[4]);
    for (int i = 0; i < 4; ++i) p.u[i] = take(kUpOut[i] * px[3 - i]);
    p.total = off;
    return true;
}

template <int KS, int MODE>
void launch_conv(const ConvArgs& a, hipStream_t stream) {
    // 64 output channels per workgroup (the patch is staged half as often) where that still leaves a workgroup per compute unit
    const unsigned tiles = cdiv(a.W, kTW) * cdiv(a.H, kTH);
    const bool wide = a.Cout % 64 == 0 && tiles * (unsigned)(a.Cout / 64) >= 256u;
    dim3 grid(cdiv(a.W, kTW), cdiv(a.H, kTH), cdiv(a.Cout, wide ? 64 : 32));
    if (wide)
        hipLaunchKernelGGL((k_conv<KS, MODE, 2>), grid, dim3(kBlock), 0, stream, a);
    else
        hipLaunchKernelGGL((k_conv<KS, MODE, 1>), grid, dim3(kBlock), 0, stream, a);
}

// fills the weight pointers of `a` from record `i` of the packed buffer
void bind(ConvArgs& a, const float* packed, int i) {
    size_t off = 0;
    for (int j = 0; j < i; ++j) off += rec_floats(kLayers[j]);
    const Layer& l = kLayers[i];
    const float* r = packed + off;
    a.scale = r;
    a.shift = r + cin_pad(l.cin);
    a.bias = r + 2 * cin_pad(l.cin);
    a.w = a.bias + l.cout;
    a.Cin = l.cin;
    a.Cout = l.cout;
}
}  // namespace

NVSF_API int nvsf_unet_sizes(uint32_t H, uint32_t W, uint64_t* sizes, hipStream_t) {
    REQUIRE(sizes);
    Plan p;
    REQUIRE(make_plan(H, W, p));
    sizes[0] = (uint64_t)p.total * sizeof(float);
    sizes[1] = (uint64_t)packed_floats();
    return NVSF_OK;
}

NVSF_API int nvsf_unet_layout(uint32_t H, uint32_t W, uint64_t* layout, hipStream_t) {
    REQUIRE(layout);
    Plan p;
    REQUIRE(make_plan(H, W, p));
    uint64_t* row = layout;
    auto put = [&](size_t off, int c, int l) { row[0] = off; row[1] = (uint64_t)c; row[2] = (uint64_t)p.H[l]; row[3] = (uint64_t)p.W[l]; row += 4; };
    for (int l = 0; l < 5; ++l) put(p.x[l], kC[l], l);
    put(p.mid, kLayers[17].cout, 0);  // what up4's first convolution, the last launch that writes `mid`, leaves there
    put(p.qkv, 768, 4);
    put(p.att, 256, 4);
    put(p.x4a, 256, 4);
    for (int i = 0; i < 4; ++i) put(p.u[i], kUpOut[i], 3 - i);
    return NVSF_OK;
}

NVSF_API int nvsf_unet_forward(const float* raydrop, const float* intensity, const float* range, uint32_t H, uint32_t W, const float* packed,
                               size_t n_packed, void* workspace, size_t ws_bytes, float thres, float* prob, float* gated_intensity,
                               float* gated_range, hipStream_t stream) {
    REQUIRE(raydrop && intensity && range && packed && workspace && prob);
    REQUIRE((gated_intensity == nullptr) == (gated_range == nullptr));
    Plan p;
    REQUIRE(make_plan(H, W, p));
    REQUIRE(n_packed == packed_floats() && ws_bytes >= p.total * sizeof(float));
    REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)workspace & 15) == 0);
    float* ws = static_cast<float*>(workspace);
    float* x[5];
    for (int l = 0; l < 5; ++l) x[l] = ws + p.x[l];
    float* mid = ws + p.mid;

    ConvArgs a = {};
    // inc: 1 x 1, bias, no normalisation (identity scale in the record)
    bind(a, packed, 0);
    a.in0 = raydrop; a.in1 = intensity; a.in2 = range;
    a.out = x[0]; a.H = p.H[0]; a.W = p.W[0]; a.relu = 0;
    launch_conv<1, kPlanes>(a, stream);
    // down1..down4: pool folded into the first convolution's load
    for (int l = 1; l < 5; ++l) {
        a = ConvArgs{};
        bind(a, packed, 2 * l - 1);
        a.in0 = x[l - 1]; a.Hs = p.H[l - 1]; a.Ws = p.W[l - 1];
        a.out = mid; a.H = p.H[l]; a.W = p.W[l]; a.relu = 1;
        launch_conv<3, kPool>(a, stream);
        a = ConvArgs{};
        bind(a, packed, 2 * l);
        a.in0 = mid; a.out = x[l]; a.H = p.H[l]; a.W = p.W[l]; a.relu = 1;
        launch_conv<3, kPlain>(a, stream);
    }
    // attention at the bottom: BatchNorm (no ReLU) folded into the qkv load; the projection adds the block's input
    const int N = p.H[4] * p.W[4];
    a = ConvArgs{};
    bind(a, packed, 9);
    a.in0 = x[4]; a.out = ws + p.qkv; a.H = p.H[4]; a.W = p.W[4]; a.relu = 0;
    launch_conv<1, kPlain>(a, stream);
    hipLaunchKernelGGL(k_attn, dim3(cdiv(N, 32), 8), dim3(64), 0, stream, ws + p.qkv, ws + p.att, N, 0.17677669529663687f);
    a = ConvArgs{};
    bind(a, packed, 10);
    a.in0 = ws + p.att; a.resid = x[4]; a.out = ws + p.x4a; a.H = p.H[4]; a.W = p.W[4]; a.relu = 0;
    launch_conv<1, kPlain>(a, stream);
    // up1..up4: upsample, pad and concat folded into the first convolution's load
    const float* low = ws + p.x4a;
    for (int i = 0; i < 4; ++i) {
        const int ls = 3 - i;  // level of the skip and of the output
        a = ConvArgs{};
        bind(a, packed, 11 + 2 * i);
        a.in0 = x[ls]; a.in1 = low; a.C0 = kC[ls];
        a.Hs = p.H[ls + 1]; a.Ws = p.W[ls + 1];
        a.padT = (p.H[ls] - 2 * a.Hs) / 2; a.padL = (p.W[ls] - 2 * a.Ws) / 2;
        a.sy = 2 * a.Hs > 1 ? (float)(a.Hs - 1) / (float)(2 * a.Hs - 1) : 0.0f;
        a.sx = 2 * a.Ws > 1 ? (float)(a.Ws - 1) / (float)(2 * a.Ws - 1) : 0.0f;
        a.out = mid; a.H = p.H[ls]; a.W = p.W[ls]; a.relu = 1;
        launch_conv<3, kUpCat>(a, stream);
        a = ConvArgs{};
        bind(a, packed, 12 + 2 * i);
        a.in0 = mid; a.out = ws + p.u[i]; a.H = p.H[ls]; a.W = p.W[ls]; a.relu = 1;
        launch_conv<3, kPlain>(a, stream);
        low = ws + p.u[i];
    }
    size_t off = 0;
    for (int j = 0; j < 19; ++j) off += rec_floats(kLayers[j]);
    const int hw = p.H[0] * p.W[0];
    hipLaunchKernelGGL(k_head, dim3(cdiv(hw, kBlock)), dim3(kBlock), 0, stream, low, packed + off, intensity, range, hw, thres, prob,
                       gated_intensity, gated_range);
    return nvsf_launch_status();
}
