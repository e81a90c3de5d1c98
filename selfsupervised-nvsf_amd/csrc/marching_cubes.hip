// Marching cubes over a dense fp32 grid for gfx950: the mesh export of the learned density field.
// Reference: nvsf/nerf/utils.py:350-384 (extract_geometry -> mcubes.marching_cubes on the CPU), called by export_mesh_density
// (:559-608) at the end of every test run (scripts/main_nvsf.py:297-300).  Python side: nvsf/nerf/mesh.py, which owns the case
// tables (one copy, uploaded once per device; the kernels stage them in LDS).
//
// Contract: u[nx, ny, nz] C-contiguous (z fastest); a grid point is inside iff u >= iso (NaN: outside).
// Every grid point owns its +x, +y, +z edges; a crossing edge (one end inside, one outside) carries ONE vertex, at i + t along its
// axis with t = (iso - a) / (b - a) (a at the owning point, b at the far end; t clamped to [0, 1] and NaN -> 0.5 when an end is not
// finite).  Vertices are ordered by (point linear index, axis x < y < z), triangles by (cube linear index = linear index of the
// cube's corner 0, order in the case table): no atomics decide any position.
//
// Three launches and one host read:
//   k_mc_count  one workgroup per tile of kTile consecutive points: per point the crossing-edge mask and the case's triangle count,
//               the exclusive prefix of both inside the tile (packed into one word per point) and the tile's two sums;
//   k_mc_scan   one workgroup: exclusive scan of the tile sums into tile offsets (in place) + the two totals (uint64);
//   (the caller reads the totals and allocates the outputs)
//   k_mc_emit   the count pass's tiles again: vertices of the point's own edges, then the case's triangles, each corner edge
//               resolved to its owning point's vertex index = tile offset + in-tile prefix + rank of the axis in its mask.
#include "common.h"
#include <math.h>

namespace {
constexpr int kBlock = 256;
constexpr int kPerThread = 16;
constexpr int kTile = kBlock * kPerThread;  // 4096 points: in-tile prefixes stay below 3 * 4096 < 2^14 and 5 * 4096 < 2^15
constexpr int kScanBlock = 1024;

// case table layout (bytes; built by nvsf/nerf/mesh.py, tables_bytes()): tri[256][16] int8 (edge ids, -1 padded) | ntri[256] uint8 |
// edge[12][4] int8 (dx, dy, dz of the owning corner, axis) | corner[8][4] int8 (dx, dy, dz, 0)
constexpr int kTriOff = 0, kNtriOff = 4096, kEdgeOff = 4352, kCornerOff = 4400, kTableBytes = 4432;

// packed per-point word: bits 0-2 crossing mask of the point's +x / +y / +z edges, 3-16 vertex prefix in the tile, 17-31 triangle prefix
__device__ __forceinline__ uint32_t pack_point(uint32_t mask, uint32_t vpre, uint32_t tpre) { return mask | (vpre << 3) | (tpre << 17); }

__device__ __forceinline__ bool inside(float v, float iso) { return v >= iso; }  // NaN: false

__device__ __forceinline__ void stage_table(const uint32_t* __restrict__ tables, uint32_t* lds, int words) {
    for (int i = threadIdx.x; i < words; i += blockDim.x) lds[i] = tables[i];
    __syncthreads();
}

struct Grid {
    uint32_t nx, ny, nz;
    uint32_t syz;                 // ny * nz: stride of x
    uint32_t n;                   // nx * ny * nz (< 2^31)
    uint32_t step_x, step_y, step_z;  // kBlock points further in linear order = (+step_x, +step_y, +step_z) with carries
};

// Grid coordinates of a thread's points p = p0 + j kBlock, advanced without a division per point.
struct Cursor {
    uint32_t x, y, z;
    __device__ __forceinline__ Cursor(const Grid& g, uint32_t p) {
        x = p / g.syz;
        const uint32_t r = p - x * g.syz;
        y = r / g.nz;
        z = r - y * g.nz;
    }
    __device__ __forceinline__ void advance(const Grid& g) {  // step_z < nz, step_y < ny: one carry per axis at most
        z += g.step_z;
        uint32_t c = z >= g.nz ? 1u : 0u;
        z -= c ? g.nz : 0u;
        y += g.step_y + c;
        c = y >= g.ny ? 1u : 0u;
        y -= c ? g.ny : 0u;
        x += g.step_x + c;
    }
};

// Position index i = 4 dx + 2 dy + dz of each cube corner k, 3 bits per corner (from the corner table).
__device__ __forceinline__ uint32_t corner_positions(const int8_t* corner) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) r |= (uint32_t)(4 * corner[4 * k] + 2 * corner[4 * k + 1] + corner[4 * k + 2]) << (3 * k);
    return r;
}

// Crossing mask of the point's own edges (bit 0 x, 1 y, 2 z) and the case of the cube whose corner 0 it is (-1: no cube).  The eight
// loads are unconditional (a neighbour beyond the grid reads the point itself) so that they issue together.
__device__ __forceinline__ void point_state(const float* __restrict__ u, const Grid& g, float iso, uint32_t p, const Cursor& at,
                                            uint32_t corner_pos, uint32_t& mask, int& cube_case) {
    const bool hx = at.x + 1 < g.nx, hy = at.y + 1 < g.ny, hz = at.z + 1 < g.nz;
    const uint32_t sx = hx ? g.syz : 0u, sy = hy ? g.nz : 0u, sz = hz ? 1u : 0u;
    uint32_t m = 0;  // bit 4 dx + 2 dy + dz: that corner is inside
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t q = p + ((i & 4) ? sx : 0u) + ((i & 2) ? sy : 0u) + ((i & 1) ? sz : 0u);
        m |= (inside(u[q], iso) ? 1u : 0u) << i;
    }
    const uint32_t in0 = m & 1u;
    mask = (hx && ((m >> 4) & 1u) != in0 ? 1u : 0u) | (hy && ((m >> 2) & 1u) != in0 ? 2u : 0u) | (hz && ((m >> 1) & 1u) != in0 ? 4u : 0u);
    int c = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) c |= (int)((m >> ((corner_pos >> (3 * k)) & 7u)) & 1u) << k;
    cube_case = (hx && hy && hz) ? c : -1;
}

// number of set bits of m in the lanes below this one
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(kBlock) void k_mc_count(const float* __restrict__ u, Grid g, float iso, const uint32_t* __restrict__ tables,
                                                     uint32_t* __restrict__ tile_sums, uint32_t* __restrict__ point_words) {
    __shared__ uint32_t lds_tab[kTableBytes / 4];
    __shared__ uint32_t wave_tot[kPerThread][kBlock / kWave];
    stage_table(tables, lds_tab, kTableBytes / 4);
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(lds_tab);
    const uint32_t corner_pos = corner_positions(reinterpret_cast<const int8_t*>(tab + kCornerOff));
    const uint32_t base = blockIdx.x * (uint32_t)kTile;
    const int wave = threadIdx.x / kWave;
    uint64_t masks = 0;            // 3 bits per j (48 bits)
    uint32_t excl[kPerThread];     // exclusive prefix inside the wave of (vertices | triangles << 16) per j
    Cursor at(g, min(base + threadIdx.x, g.n - 1));
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const uint32_t p = base + j * kBlock + threadIdx.x;
        uint32_t mask = 0, nv = 0, nt = 0;
        if (p < g.n) {
            int c;
            point_state(u, g, iso, p, at, corner_pos, mask, c);
            nv = (uint32_t)__popc(mask);
            nt = c >= 0 ? (uint32_t)tab[kNtriOff + c] : 0u;
        }
        at.advance(g);
        masks |= (uint64_t)mask << (3 * j);
        // wave prefix of the small counts from their bits: nv < 4, nt < 8
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const uint64_t bal = __ballot((nv >> b) & 1u);
            pre += lanes_below(bal) << b;
            tot += (uint32_t)__popcll(bal) << b;
        }
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const uint64_t bal = __ballot((nt >> b) & 1u);
            pre += lanes_below(bal) << (16 + b);
            tot += (uint32_t)__popcll(bal) << (16 + b);
        }
        excl[j] = pre;
        if (lane_id() == 0) wave_tot[j][wave] = tot;
    }
    __syncthreads();
    uint32_t run = 0;  // packed sum of everything before row j
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        uint32_t pre = run;
        uint32_t row = 0;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) {
            const uint32_t t = wave_tot[j][w];
            if (w < wave) pre += t;
            row += t;
        }
        pre += excl[j];
        run += row;
        const uint32_t p = base + j * kBlock + threadIdx.x;
        if (p < g.n) point_words[p] = pack_point((uint32_t)(masks >> (3 * j)) & 7u, pre & 0xFFFFu, pre >> 16);
    }
    if (threadIdx.x == 0) {
        tile_sums[2 * blockIdx.x] = run & 0xFFFFu;
        tile_sums[2 * blockIdx.x + 1] = run >> 16;
    }
}

// One workgroup: thread i owns the tile range [i * per, (i + 1) * per); exclusive offsets are written over the sums.
__global__ __launch_bounds__(kScanBlock) void k_mc_scan(uint32_t* __restrict__ tile_sums, uint32_t n_tiles, uint32_t per,
                                                        unsigned long long* __restrict__ totals) {
    __shared__ unsigned long long sv[kScanBlock], st[kScanBlock];
    const uint32_t lo = threadIdx.x * per, hi = min(n_tiles, lo + per);
    unsigned long long v = 0, t = 0;
    for (uint32_t i = lo; i < hi; ++i) {
        v += tile_sums[2 * i];
        t += tile_sums[2 * i + 1];
    }
    sv[threadIdx.x] = v;
    st[threadIdx.x] = t;
    __syncthreads();
    for (int o = 1; o < kScanBlock; o <<= 1) {  // Hillis-Steele inclusive scan
        const unsigned long long av = threadIdx.x >= (unsigned)o ? sv[threadIdx.x - o] : 0ull;
        const unsigned long long at = threadIdx.x >= (unsigned)o ? st[threadIdx.x - o] : 0ull;
        __syncthreads();
        sv[threadIdx.x] += av;
        st[threadIdx.x] += at;
        __syncthreads();
    }
    unsigned long long ov = sv[threadIdx.x] - v, ot = st[threadIdx.x] - t;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t cv = tile_sums[2 * i], ct = tile_sums[2 * i + 1];
        tile_sums[2 * i] = (uint32_t)ov;  // the caller refuses totals >= 2^31 before any offset is used
        tile_sums[2 * i + 1] = (uint32_t)ot;
        ov += cv;
        ot += ct;
    }
    if (threadIdx.x == kScanBlock - 1) {
        totals[0] = sv[kScanBlock - 1];
        totals[1] = st[kScanBlock - 1];
    }
}

__device__ __forceinline__ float edge_t(float a, float b, float iso) {
    float t = (iso - a) / (b - a);
    if (!(isfinite(a) && isfinite(b))) t = isnan(t) ? 0.5f : fminf(fmaxf(t, 0.0f), 1.0f);
    return t;
}

__global__ __launch_bounds__(kBlock) void k_mc_emit(const float* __restrict__ u, Grid g, float iso, const uint32_t* __restrict__ tables,
                                                    const uint32_t* __restrict__ tile_offs, const uint32_t* __restrict__ point_words,
                                                    float* __restrict__ vertices, uint32_t n_vertices, int32_t* __restrict__ triangles,
                                                    uint32_t n_triangles) {
    __shared__ uint32_t lds_tab[kTableBytes / 4];
    stage_table(tables, lds_tab, kTableBytes / 4);
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(lds_tab);
    const int8_t* tri = reinterpret_cast<const int8_t*>(tab + kTriOff);
    const int8_t* edge = reinterpret_cast<const int8_t*>(tab + kEdgeOff);
    const int8_t* corner = reinterpret_cast<const int8_t*>(tab + kCornerOff);
    const uint32_t corner_pos = corner_positions(corner);
    const uint32_t base = blockIdx.x * (uint32_t)kTile;
    const uint32_t voff = tile_offs[2 * blockIdx.x], toff = tile_offs[2 * blockIdx.x + 1];
    Cursor at(g, min(base + threadIdx.x, g.n - 1));
    for (int j = 0; j < kPerThread; ++j, at.advance(g)) {
        const uint32_t p = base + j * kBlock + threadIdx.x;
        if (p >= g.n) break;
        uint32_t mask;
        int c;
        point_state(u, g, iso, p, at, corner_pos, mask, c);
        if (mask == 0 && (c <= 0 || c == 255)) continue;
        const uint32_t w = point_words[p];
        if (mask) {
            const float a = u[p];
            uint32_t vi = voff + ((w >> 3) & 0x3FFFu);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                if (!(mask & (1u << ax))) continue;
                const uint32_t step = ax == 0 ? g.syz : (ax == 1 ? g.nz : 1u);
                const float t = edge_t(a, u[p + step], iso);
                if (vi < n_vertices) {
                    float* o = vertices + (size_t)vi * 3;
                    o[0] = (float)at.x + (ax == 0 ? t : 0.0f);
                    o[1] = (float)at.y + (ax == 1 ? t : 0.0f);
                    o[2] = (float)at.z + (ax == 2 ? t : 0.0f);
                }
                ++vi;
            }
        }
        if (c <= 0 || c == 255) continue;
        const uint32_t nt = tab[kNtriOff + c];
        uint32_t ti = toff + (w >> 17);
        for (uint32_t k = 0; k < nt; ++k, ++ti) {
            int32_t vid[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const int e = tri[16 * c + 3 * k + m];
                const uint32_t q = p + (uint32_t)edge[4 * e] * g.syz + (uint32_t)edge[4 * e + 1] * g.nz + (uint32_t)edge[4 * e + 2];
                const uint32_t ax = (uint32_t)edge[4 * e + 3];
                const uint32_t wq = point_words[q];
                vid[m] = (int32_t)(tile_offs[2 * (q / kTile)] + ((wq >> 3) & 0x3FFFu) + (uint32_t)__popc(wq & 7u & ((1u << ax) - 1u)));
            }
            if (ti < n_triangles) {
                int32_t* o = triangles + (size_t)ti * 3;
                o[0] = vid[0];
                o[1] = vid[1];
                o[2] = vid[2];
            }
        }
    }
}

bool make_grid(uint32_t nx, uint32_t ny, uint32_t nz, Grid& g) {
    const unsigned long long n = (unsigned long long)nx * ny * nz;
    if (n >= (1ull << 31)) return false;
    g.nx = nx; g.ny = ny; g.nz = nz; g.syz = ny * nz; g.n = (uint32_t)n;
    g.step_z = kBlock % nz;
    g.step_y = (kBlock / nz) % ny;
    g.step_x = kBlock / nz / ny;
    return true;
}
}  // namespace

static inline size_t mc_ws_need(const Grid& g) {
    const size_t tiles = cdiv(g.n, kTile);
    return tiles * 8 + (size_t)g.n * 4;
}

NVSF_API int nvsf_marching_cubes_count(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, float iso, const void* tables, void* workspace,
                                       size_t ws_bytes, uint64_t* totals, hipStream_t stream) {
    REQUIRE(u && tables && workspace && totals && nx >= 1 && ny >= 1 && nz >= 1);
    REQUIRE((reinterpret_cast<uintptr_t>(tables) & 3u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 &&
            (reinterpret_cast<uintptr_t>(totals) & 7u) == 0);
    Grid g;
    REQUIRE(make_grid(nx, ny, nz, g));
    if (nx < 2 || ny < 2 || nz < 2) {  // a flat grid has no cube: empty mesh
        hipError_t e = hipMemsetAsync(totals, 0, 2 * sizeof(uint64_t), stream);
        return e == hipSuccess ? NVSF_OK : (int)e;
    }
    REQUIRE(ws_bytes >= mc_ws_need(g));
    const uint32_t tiles = cdiv(g.n, kTile);
    uint32_t* tile_sums = reinterpret_cast<uint32_t*>(workspace);
    uint32_t* point_words = tile_sums + 2 * (size_t)tiles;
    hipLaunchKernelGGL(k_mc_count, dim3(tiles), dim3(kBlock), 0, stream, u, g, iso, reinterpret_cast<const uint32_t*>(tables), tile_sums,
                       point_words);
    hipLaunchKernelGGL(k_mc_scan, dim3(1), dim3(kScanBlock), 0, stream, tile_sums, tiles, cdiv(tiles, kScanBlock),
                       reinterpret_cast<unsigned long long*>(totals));
    return nvsf_launch_status();
}

NVSF_API int nvsf_marching_cubes_emit(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, float iso, const void* tables,
                                      const void* workspace, size_t ws_bytes, uint32_t n_vertices, uint32_t n_triangles, float* vertices,
                                      uint32_t v_capacity, int32_t* triangles, uint32_t t_capacity, hipStream_t stream) {
    REQUIRE(u && tables && workspace && nx >= 1 && ny >= 1 && nz >= 1);
    REQUIRE((reinterpret_cast<uintptr_t>(tables) & 3u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0);
    Grid g;
    REQUIRE(make_grid(nx, ny, nz, g));
    REQUIRE(n_vertices < (1u << 31) && n_triangles < (1u << 31));
    REQUIRE(v_capacity >= n_vertices && t_capacity >= n_triangles);
    REQUIRE((vertices || n_vertices == 0) && (triangles || n_triangles == 0));
    if (nx < 2 || ny < 2 || nz < 2) return NVSF_OK;  // flat grid: nothing was counted, nothing to write
    REQUIRE(ws_bytes >= mc_ws_need(g));
    if (n_vertices == 0 && n_triangles == 0) return NVSF_OK;
    const uint32_t tiles = cdiv(g.n, kTile);
    const uint32_t* tile_offs = reinterpret_cast<const uint32_t*>(workspace);
    const uint32_t* point_words = tile_offs + 2 * (size_t)tiles;
    hipLaunchKernelGGL(k_mc_emit, dim3(tiles), dim3(kBlock), 0, stream, u, g, iso, reinterpret_cast<const uint32_t*>(tables), tile_offs,
                       point_words, vertices, n_vertices, triangles, n_triangles);
    return nvsf_launch_status();
}
