// hm_mesh_dev.h - the marching-cubes arithmetic shared by the dense volume (hm_mesh.hip) and the brick pool
// (hm_mesh_sparse.hip): the workgroup scan, the scan of the block sums, the gradient and the vertex.  Both files read
// their lattice through a Vol with nx, ny, nz and at(i, j, k), so the two paths run the same fp32 operations in the same
// order and their outputs agree bit for bit.
#pragma once
#include "hm_common.h"

constexpr int kMT = 256;                  // threads per workgroup
constexpr int kMRounds = 16;              // rounds of kMT consecutive points per workgroup
constexpr int kMBlock = kMT * kMRounds;   // 4096 lattice points per workgroup
constexpr int kScanT = 1024;

inline int64_t mc_up256(int64_t b) { return (b + 255) / 256 * 256; }

struct McWs {
    uint16_t *code;      // [n] bits 0-7 cell case (0 on the upper faces), bits 8-10 crossing axes
    int32_t *vbase;      // [n]
    int32_t *bsum;       // [3][nb] vertex sum, triangle sum, NaN bit per block
    int64_t *boff;       // [2][nb] exclusive block offsets of vertices and triangles
};

inline int64_t mc_ws_bytes(int64_t n) {
    const int64_t nb = (n + kMBlock - 1) / kMBlock;
    return mc_up256(2 * n) + mc_up256(4 * n) + mc_up256(12 * nb) + mc_up256(16 * nb);
}

inline McWs mc_carve(void *ws, int64_t n) {
    const int64_t nb = (n + kMBlock - 1) / kMBlock;
    char *p = static_cast<char *>(ws);
    McWs w;
    w.code = reinterpret_cast<uint16_t *>(p);
    p += mc_up256(2 * n);
    w.vbase = reinterpret_cast<int32_t *>(p);
    p += mc_up256(4 * n);
    w.bsum = reinterpret_cast<int32_t *>(p);
    p += mc_up256(12 * nb);
    w.boff = reinterpret_cast<int64_t *>(p);
    return w;
}

#ifdef __HIPCC__
// exclusive prefix of x over the workgroup's threads (in thread order) and the workgroup total
__device__ __forceinline__ int block_excl_scan(int x, int *lds_waves, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int s = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(s, o, 64);
        if (lane >= o) s += y;
    }
    if (lane == 63) lds_waves[wave] = s;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kMT / 64; ++w) {
        const int t = lds_waves[w];
        before += w < wave ? t : 0;
        total += t;
    }
    __syncthreads();
    return before + s - x;
}

// a classify kernel's tail: workgroup sums (fixed order: wave reduction, then the waves in order) -> bsum[.][block]
__device__ __forceinline__ void mc_block_sums(int nv, int nt, int nan, int32_t *__restrict__ bsum, int64_t nb) {
    __shared__ int red[3][kMT / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nv += __shfl_xor(nv, o, 64);
        nt += __shfl_xor(nt, o, 64);
        nan |= __shfl_xor(nan, o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = nv;
        red[1][wave] = nt;
        red[2][wave] = nan;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        int s = 0;
        for (int w = 0; w < kMT / 64; ++w) s = threadIdx.x == 2 ? (s | red[2][w]) : s + red[threadIdx.x][w];
        bsum[threadIdx.x * nb + blockIdx.x] = s;
    }
}

// exclusive prefix of the block sums (int64), totals[0..2] = vertices, triangles, NaN flag
static __global__ __launch_bounds__(kScanT) void mc_scan_kernel(const int32_t *__restrict__ bsum, int64_t nb,
                                                                int64_t *__restrict__ boff,
                                                                int64_t *__restrict__ totals) {
    __shared__ int64_t pv[kScanT], pt[kScanT];
    __shared__ int pn[kScanT];
    const int64_t per = (nb + kScanT - 1) / kScanT;
    const int64_t beg = min((int64_t)threadIdx.x * per, nb), end = min(beg + per, nb);
    int64_t sv = 0, st = 0;
    int nan = 0;
    for (int64_t b = beg; b < end; ++b) {
        sv += bsum[b];
        st += bsum[nb + b];
        nan |= bsum[2 * nb + b];
    }
    pv[threadIdx.x] = sv;
    pt[threadIdx.x] = st;
    pn[threadIdx.x] = nan;
    __syncthreads();
    for (int o = 1; o < kScanT; o <<= 1) {
        const int64_t av = (int)threadIdx.x >= o ? pv[threadIdx.x - o] : 0;
        const int64_t at = (int)threadIdx.x >= o ? pt[threadIdx.x - o] : 0;
        const int an = (int)threadIdx.x >= o ? pn[threadIdx.x - o] : 0;
        __syncthreads();
        pv[threadIdx.x] += av;
        pt[threadIdx.x] += at;
        pn[threadIdx.x] |= an;
        __syncthreads();
    }
    int64_t rv = pv[threadIdx.x] - sv, rt = pt[threadIdx.x] - st;
    for (int64_t b = beg; b < end; ++b) {
        boff[b] = rv;
        boff[nb + b] = rt;
        rv += bsum[b];
        rt += bsum[nb + b];
    }
    if (threadIdx.x == kScanT - 1) {
        totals[0] = pv[kScanT - 1];
        totals[1] = pt[kScanT - 1];
        totals[2] = pn[kScanT - 1];
    }
}

// central difference along each axis (one-sided at the border) over the spacing: numpy.gradient's rule
template <class Vol>
__device__ __forceinline__ void mc_grad(const Vol &V, int i, int j, int k, const float (&sp)[3], float (&g)[3]) {
    const int n[3] = {V.nx, V.ny, V.nz};
    const int p[3] = {i, j, k};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int lo = p[a] > 0 ? p[a] - 1 : p[a], hi = p[a] + 1 < n[a] ? p[a] + 1 : p[a];
        const float vlo = V.at(a == 0 ? lo : i, a == 1 ? lo : j, a == 2 ? lo : k);
        const float vhi = V.at(a == 0 ? hi : i, a == 1 ? hi : j, a == 2 ? hi : k);
        g[a] = (vhi - vlo) / ((float)(hi - lo) * sp[a]);
    }
}

// the vertex on the lattice edge from (i, j, k), value a and gradient g0, along axis ax: position and unit normal
template <class Vol>
__device__ __forceinline__ void mc_vertex(const Vol &V, float level, const float (&sp)[3], int i, int j, int k, int ax,
                                          float a, const float (&g0)[3], float (&pos)[3], float (&nrm)[3]) {
    const int i1 = i + (ax == 0), j1 = j + (ax == 1), k1 = k + (ax == 2);
    const float b = V.at(i1, j1, k1);
    const float t = (level - a) / (b - a);
    float g1[3], nn[3];
    mc_grad(V, i1, j1, k1, sp, g1);
#pragma unroll
    for (int m = 0; m < 3; ++m) nn[m] = g0[m] + t * (g1[m] - g0[m]);
    const float d = nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2];
    const float s = sqrtf(d);
    const int id[3] = {i, j, k};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        pos[m] = (m == ax ? (float)id[m] + t : (float)id[m]) * sp[m];
        nrm[m] = d > 0.0f ? nn[m] / s : 0.0f;
    }
}
#endif
