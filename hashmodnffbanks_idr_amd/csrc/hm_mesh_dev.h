// hm_mesh_dev.h - marching cubes, written once over a lattice type: the workspace, the classify / verts / faces kernels,
// the scan of the block sums, the gradient and the vertex.  hm_mesh.hip instantiates them for the dense volume (McVol),
// hm_mesh_sparse.hip for the listed bricks of the value pool (BrickLat), so the two paths run the same fp32 operations
// in the same order and their outputs agree bit for bit.  The wave and workgroup primitives are hm_block_dev.h's.
//
// A lattice Lat supplies
//   nx, ny, nz, at(i, j, k)     the values; has(i, j, k): is the point evaluated
//   point(q, i, j, k)           work item q -> its lattice point; false for a padding item
//   corner(q, i, j, k, c, p)    p = the work item that owns corner c (bit 0 +x, bit 1 +y, bit 2 +z) of the cell of item q
//                               at (i, j, k); false when it is not listed
//   vert_key(vi, i, j, k, ax), face_key(f, i, j, k, t)    record the sort key of an output
// For the dense lattice every item is a point, every point is evaluated and every corner is listed: has(), point() and
// corner() are the constant true there and the keys are empty, a compile-time property of the type, so the guards and
// the index arithmetic they would need compile to nothing and the dense kernels are the bodies without them.
#pragma once
#include "hm_block_dev.h"
#include "hm_mc_table.h"

constexpr int kMT = 256;                  // threads per workgroup
constexpr int kMRounds = 16;              // rounds of kMT consecutive points per workgroup
constexpr int kMBlock = kMT * kMRounds;   // 4096 lattice points per workgroup
constexpr int kScanT = 1024;

struct McWs {
    uint16_t *code;      // [n] bits 0-7 cell case (0 on the upper faces), bits 8-10 crossing axes
    int32_t *vbase;      // [n]
    int32_t *bsum;       // [3][nb] vertex sum, triangle sum, NaN bit per block
    int64_t *boff;       // [2][nb] exclusive block offsets of vertices and triangles
    int64_t nb, bytes;   // workgroup blocks of n work items; the size of the workspace
};

inline McWs mc_layout(void *ws, int64_t n) {
    HmCarve c(ws);
    McWs w;
    w.nb = (n + kMBlock - 1) / kMBlock;
    w.code = c.take<uint16_t>(n);
    w.vbase = c.take<int32_t>(n);
    w.bsum = c.take<int32_t>(3 * w.nb);
    w.boff = c.take<int64_t>(2 * w.nb);
    w.bytes = c.bytes;
    return w;
}

#ifdef __HIPCC__
// a classify kernel's tail: workgroup sums (fixed order: wave reduction, then the waves in order) -> bsum[.][block]
__device__ __forceinline__ void mc_block_sums(int nv, int nt, int nan, int32_t *__restrict__ bsum, int64_t nb) {
    __shared__ int red[3][kMT / 64];
    nv = hm_wave_reduce(nv, HmSum{});
    nt = hm_wave_reduce(nt, HmSum{});
    nan = hm_wave_reduce(nan, HmOr{});
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

// per work item: the sign-changing lattice edges its point owns (+x, +y, +z) and the case of the cell it is the lowest
// corner of -> code; per workgroup block: vertex and triangle sums and a NaN bit.  An edge or a cell with a corner that
// is not evaluated counts nothing.
template <class Lat>
__global__ __launch_bounds__(kMT) void mc_classify_kernel(Lat V, float level, int64_t n, uint16_t *__restrict__ code,
                                                          int32_t *__restrict__ bsum, int64_t nb) {
    const int64_t beg = (int64_t)blockIdx.x * kMBlock;
    int nv = 0, nt = 0, nan = 0;
    for (int r = 0; r < kMRounds; ++r) {
        const int64_t q = beg + (int64_t)r * kMT + threadIdx.x;
        if (q >= n) break;
        int i, j, k;
        if (!V.point(q, i, j, k) || !V.has(i, j, k)) {
            code[q] = 0;
            continue;
        }
        const float c0 = V.at(i, j, k);
        nan |= c0 != c0;
        const bool in0 = c0 < level;
        const bool hx = i + 1 < V.nx && V.has(i + 1, j, k), hy = j + 1 < V.ny && V.has(i, j + 1, k),
                   hz = k + 1 < V.nz && V.has(i, j, k + 1);
        // corner values of the cell (i, j, k) .. (i+1, j+1, k+1); only the ones that exist are read
        const float c1 = hx ? V.at(i + 1, j, k) : c0;
        const float c2 = hy ? V.at(i, j + 1, k) : c0;
        const float c4 = hz ? V.at(i, j, k + 1) : c0;
        const int mask = ((hx && (c1 < level) != in0) ? 1 : 0) | ((hy && (c2 < level) != in0) ? 2 : 0) |
                         ((hz && (c4 < level) != in0) ? 4 : 0);
        int cs = 0;
        if (hx && hy && hz && V.has(i + 1, j + 1, k) && V.has(i + 1, j, k + 1) && V.has(i, j + 1, k + 1) &&
            V.has(i + 1, j + 1, k + 1)) {
            const float c3 = V.at(i + 1, j + 1, k), c5 = V.at(i + 1, j, k + 1);
            const float c6 = V.at(i, j + 1, k + 1), c7 = V.at(i + 1, j + 1, k + 1);
            cs = (int)in0 | (int)(c1 < level) << 1 | (int)(c2 < level) << 2 | (int)(c3 < level) << 3 |
                 (int)(c4 < level) << 4 | (int)(c5 < level) << 5 | (int)(c6 < level) << 6 | (int)(c7 < level) << 7;
        }
        code[q] = (uint16_t)(cs | mask << 8);
        nv += __popc(mask);
        nt += hm_mc_tris[cs][0];
    }
    mc_block_sums(nv, nt, nan, bsum, nb);
}

// per work item: vertex base = block offset + in-block prefix (-> vbase), its vertices and normals
template <class Lat>
__global__ __launch_bounds__(kMT) void mc_verts_kernel(Lat V, float level, float spx, float spy, float spz, int64_t n,
                                                       const uint16_t *__restrict__ code, int32_t *__restrict__ vbase,
                                                       const int64_t *__restrict__ boff, int64_t cap_v,
                                                       float *__restrict__ verts, float *__restrict__ normals) {
    __shared__ int lds_waves[kMT / 64];
    const float sp[3] = {spx, spy, spz};
    const int64_t beg = (int64_t)blockIdx.x * kMBlock;
    int64_t base = boff[blockIdx.x];
    for (int r = 0; r < kMRounds; ++r) {
        if (beg + (int64_t)r * kMT >= n) break;  // uniform over the workgroup
        const int64_t q = beg + (int64_t)r * kMT + threadIdx.x;
        const int mask = q < n ? code[q] >> 8 : 0;
        const int nv = __popc(mask);
        int total;
        const int pre = hm_block_scan<kMT>(nv, lds_waves, total) - nv;
        if (q < n) {
            int64_t vi = base + pre;
            vbase[q] = (int32_t)vi;
            if (mask) {
                int i, j, k;
                V.point(q, i, j, k);   // true: the item has a code
                const float a = V.at(i, j, k);
                float g0[3];
                mc_grad(V, i, j, k, sp, g0);
                for (int ax = 0; ax < 3; ++ax) {
                    if (!((mask >> ax) & 1)) continue;
                    float pos[3], nrm[3];
                    mc_vertex(V, level, sp, i, j, k, ax, a, g0, pos, nrm);
                    if (vi < cap_v) {
#pragma unroll
                        for (int m = 0; m < 3; ++m) {
                            verts[vi * 3 + m] = pos[m];
                            normals[vi * 3 + m] = nrm[m];
                        }
                        V.vert_key(vi, i, j, k, ax);
                    }
                    ++vi;
                }
            }
        }
        base += total;
    }
}

// per cell: face base likewise; each edge of a table triangle is the vertex vbase[p] + (its axis' rank among p's
// crossing axes) of the work item p that owns one of the cell's 8 corners (-1 where that item is not listed)
template <class Lat>
__global__ __launch_bounds__(kMT) void mc_faces_kernel(Lat V, int64_t n, const uint16_t *__restrict__ code,
                                                       const int32_t *__restrict__ vbase,
                                                       const int64_t *__restrict__ boff, int64_t cap_f,
                                                       int32_t *__restrict__ faces) {
    __shared__ int lds_waves[kMT / 64];
    const int64_t beg = (int64_t)blockIdx.x * kMBlock;
    int64_t base = boff[blockIdx.x];
    for (int r = 0; r < kMRounds; ++r) {
        if (beg + (int64_t)r * kMT >= n) break;
        const int64_t q = beg + (int64_t)r * kMT + threadIdx.x;
        const int cs = q < n ? code[q] & 255 : 0;
        const int nt = hm_mc_tris[cs][0];
        int total;
        const int pre = hm_block_scan<kMT>(nt, lds_waves, total) - nt;
        int64_t f = base + pre;
        int i = 0, j = 0, k = 0;
        if (nt) V.point(q, i, j, k);
        for (int t = 0; t < nt; ++t, ++f) {
            if (f >= cap_f) break;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const int e = hm_mc_tris[cs][1 + 3 * t + m];
                const int c = hm_mc_edge_corner[e], ax = hm_mc_edge_axis[e];
                int64_t p;
                int32_t id = -1;
                if (V.corner(q, i, j, k, c, p)) {
                    const int pmask = code[p] >> 8;
                    id = vbase[p] + __popc(pmask & ((1 << ax) - 1));
                }
                faces[f * 3 + m] = id;
            }
            V.face_key(f, i, j, k, t);
        }
        base += total;
    }
}
#endif
