// hm_mesh_sparse.hip - marching cubes of a lattice that is evaluated only near the surface (Mesh extraction;
// the driver is ops.marching_cubes_sparse).
//
// The lattice [nx, ny, nz] is split into bricks of 8^3 points.  A dense int32 brick map [ceil(nx/8), ceil(ny/8),
// ceil(nz/8)] gives each brick a slot of the value pool [slots, 8, 8, 8] fp32, or -1 while it is not evaluated; a map
// entry outside [0, n_slots) reads as -1.  The cell block of a brick is its 8^3 cells: their corners are the 9^3 points
// [8b, 8b + 8] clipped to the lattice, so it reaches into the low faces of the upper neighbour bricks.
//   hm_mcs_points_bricks / _index   lattice points -> coordinates for the SDF (one fixed fp32 expression per point)
//   hm_mcs_status                   per listed brick: does its cell block / do its 6 block faces hold values on both
//                                   sides of the level, a NaN bit, and "a needed brick is not evaluated"
//   hm_mcs_count / hm_mcs_emit      the two phases of hm_mesh.hip over the points of the listed (surface) bricks, the
//                                   lattice read through the brick map; the arithmetic is hm_mesh_dev.h, shared with the
//                                   dense kernels.  A cell or an edge with a corner that is not evaluated emits nothing.
//                                   Outputs come in list order with an int64 key each; sorted by key they are the dense
//                                   kernels' outputs.
#include "hm_mc_table.h"
#include "hm_mesh_dev.h"

namespace {

constexpr int kB = HM_MCS_BRICK, kB3 = kB * kB * kB;   // 8, 512
static_assert(kB == 8 && kMBlock % kB3 == 0, "local indices are 3 bits per axis; a workgroup takes whole bricks");

struct BrickVol {
    const float *pool;
    const int32_t *map;
    int64_t n_slots;
    int32_t nx, ny, nz;
    int32_t bx, by, bz;
    __device__ __forceinline__ int64_t brick_of(int i, int j, int k) const {
        return ((int64_t)(i >> 3) * by + (j >> 3)) * bz + (k >> 3);
    }
    __device__ __forceinline__ int64_t slot(int i, int j, int k) const {
        const int64_t s = map[brick_of(i, j, k)];
        return s < n_slots ? s : -1;
    }
    __device__ __forceinline__ bool has(int i, int j, int k) const { return slot(i, j, k) >= 0; }
    // NaN where the brick is not evaluated (the halo makes every read of the emit phase an evaluated one)
    __device__ __forceinline__ float at(int i, int j, int k) const {
        const int64_t s = slot(i, j, k);
        return s < 0 ? __builtin_nanf("") : pool[s * kB3 + ((i & 7) << 6 | (j & 7) << 3 | (k & 7))];
    }
};

// point p of the brick list -> lattice point; false for a padding point or a brick id outside the map
__device__ __forceinline__ bool mcs_point(int64_t p, const int32_t *__restrict__ bricks, const BrickVol &V, int &i,
                                          int &j, int &k) {
    const int64_t b = bricks[p >> 9];
    if (b < 0 || b >= (int64_t)V.bx * V.by * V.bz) return false;
    const int l = (int)(p & (kB3 - 1));
    k = (int)(b % V.bz) * kB + (l & 7);
    j = (int)(b / V.bz % V.by) * kB + ((l >> 3) & 7);
    i = (int)(b / V.bz / V.by) * kB + (l >> 6);
    return i < V.nx && j < V.ny && k < V.nz;
}

struct LatAxes {
    const float *ax, *ay, *az;
    int32_t nx, ny, nz;
};
struct LatXform {
    float r[9], s[3];   // p -> p @ r + s
    int32_t on;
};

__device__ __forceinline__ void lat_point(const LatAxes &A, const LatXform &X, int i, int j, int k,
                                          float *__restrict__ out) {
    const float x = A.ax[i], y = A.ay[j], z = A.az[k];
    if (!X.on) {
        out[0] = x;
        out[1] = y;
        out[2] = z;
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = ((x * X.r[c] + y * X.r[3 + c]) + z * X.r[6 + c]) + X.s[c];
}

__global__ __launch_bounds__(256) void mcs_points_bricks_kernel(const int32_t *__restrict__ bricks, int64_t n,
                                                                LatAxes A, LatXform X, int32_t by, int32_t bz,
                                                                float *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int64_t b = bricks[p >> 9];
    const int l = (int)(p & (kB3 - 1));
    // padding points of a border brick take the border's coordinate; a brick id outside the map is clamped likewise
    const int i = (int)max((int64_t)0, min((int64_t)A.nx - 1, b / bz / by * kB + (l >> 6)));
    const int j = (int)max((int64_t)0, min((int64_t)A.ny - 1, b / bz % by * kB + ((l >> 3) & 7)));
    const int k = (int)max((int64_t)0, min((int64_t)A.nz - 1, b % bz * kB + (l & 7)));
    lat_point(A, X, i, j, k, out + p * 3);
}

__global__ __launch_bounds__(256) void mcs_points_index_kernel(const int64_t *__restrict__ q, int64_t n, LatAxes A,
                                                               LatXform X, float *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int64_t u = q[p];
    if (u < 0 || u >= (int64_t)A.nx * A.ny * A.nz) {   // not a lattice point
        out[p * 3] = out[p * 3 + 1] = out[p * 3 + 2] = __builtin_nanf("");
        return;
    }
    lat_point(A, X, (int)(u / A.nz / A.ny), (int)(u / A.nz % A.ny), (int)(u % A.nz), out + p * 3);
}

// one workgroup per listed brick: its cell block's (up to) 9^3 points
__global__ __launch_bounds__(256) void mcs_status_kernel(const int32_t *__restrict__ bricks, BrickVol V, float level,
                                                         int32_t *__restrict__ status) {
    __shared__ int red[4][256 / 64];
    const int64_t b = bricks[blockIdx.x];
    if (b < 0 || b >= (int64_t)V.bx * V.by * V.bz) {
        if (threadIdx.x == 0) status[blockIdx.x] = HM_MCS_UNDECIDED;
        return;
    }
    const int bi = (int)(b / V.bz / V.by), bj = (int)(b / V.bz % V.by), bk = (int)(b % V.bz);
    const int ex = min(kB + 1, V.nx - bi * kB), ey = min(kB + 1, V.ny - bj * kB), ez = min(kB + 1, V.nz - bk * kB);
    int below = 0, above = 0, nan = 0, missing = 0;   // bit 0 the block, bits 1-6 its faces -x +x -y +y -z +z
    for (int t = threadIdx.x; t < (kB + 1) * (kB + 1) * (kB + 1); t += 256) {
        const int li = t / 81, lj = t / 9 % 9, lk = t % 9;
        if (li >= ex || lj >= ey || lk >= ez) continue;
        const int i = bi * kB + li, j = bj * kB + lj, k = bk * kB + lk;
        if (!V.has(i, j, k)) {
            missing = 1;
            continue;
        }
        const float v = V.at(i, j, k);
        nan |= v != v;
        const int where = 1 | (li == 0) << 1 | (li == kB) << 2 | (lj == 0) << 3 | (lj == kB) << 4 | (lk == 0) << 5 |
                          (lk == kB) << 6;
        if (v < level) below |= where;
        else above |= where;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        below |= __shfl_xor(below, o, 64);
        above |= __shfl_xor(above, o, 64);
        nan |= __shfl_xor(nan, o, 64);
        missing |= __shfl_xor(missing, o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = below;
        red[1][wave] = above;
        red[2][wave] = nan;
        red[3][wave] = missing;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int r[4] = {0, 0, 0, 0};
        for (int w = 0; w < 256 / 64; ++w)
            for (int m = 0; m < 4; ++m) r[m] |= red[m][w];
        int both = r[0] & r[1];
        // a low face of the lattice border has no brick across it (an upper one has no points in the block)
        if (bi == 0) both &= ~HM_MCS_FACE(0);
        if (bj == 0) both &= ~HM_MCS_FACE(2);
        if (bk == 0) both &= ~HM_MCS_FACE(4);
        status[blockIdx.x] = both | (r[2] ? HM_MCS_NAN : 0) | (r[3] ? HM_MCS_UNDECIDED : 0);
    }
}

// mc_classify of hm_mesh.hip over the points of the listed bricks
__global__ __launch_bounds__(kMT) void mcs_classify_kernel(const int32_t *__restrict__ bricks, BrickVol V, float level,
                                                           int64_t n, uint16_t *__restrict__ code,
                                                           int32_t *__restrict__ bsum, int64_t nb) {
    const int64_t beg = (int64_t)blockIdx.x * kMBlock;
    int nv = 0, nt = 0, nan = 0;
    for (int r = 0; r < kMRounds; ++r) {
        const int64_t q = beg + (int64_t)r * kMT + threadIdx.x;
        if (q >= n) break;
        int i, j, k;
        if (!mcs_point(q, bricks, V, i, j, k) || !V.has(i, j, k)) {
            code[q] = 0;
            continue;
        }
        const float c0 = V.at(i, j, k);
        nan |= c0 != c0;
        const bool in0 = c0 < level;
        const bool hx = i + 1 < V.nx && V.has(i + 1, j, k), hy = j + 1 < V.ny && V.has(i, j + 1, k),
                   hz = k + 1 < V.nz && V.has(i, j, k + 1);
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

__global__ __launch_bounds__(kMT) void mcs_verts_kernel(const int32_t *__restrict__ bricks, BrickVol V, float level,
                                                        float spx, float spy, float spz, int64_t n,
                                                        const uint16_t *__restrict__ code, int32_t *__restrict__ vbase,
                                                        const int64_t *__restrict__ boff, int64_t cap_v,
                                                        float *__restrict__ verts, float *__restrict__ normals,
                                                        int64_t *__restrict__ vkeys) {
    __shared__ int lds_waves[kMT / 64];
    const float sp[3] = {spx, spy, spz};
    const int64_t beg = (int64_t)blockIdx.x * kMBlock;
    int64_t base = boff[blockIdx.x];
    for (int r = 0; r < kMRounds; ++r) {
        if (beg + (int64_t)r * kMT >= n) break;  // uniform over the workgroup
        const int64_t q = beg + (int64_t)r * kMT + threadIdx.x;
        const int mask = q < n ? code[q] >> 8 : 0;
        int total;
        const int pre = block_excl_scan(__popc(mask), lds_waves, total);
        if (q < n) {
            int64_t vi = base + pre;
            vbase[q] = (int32_t)vi;
            if (mask) {
                int i, j, k;
                mcs_point(q, bricks, V, i, j, k);   // true: the point has a code
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
                        vkeys[vi] = (((int64_t)i * V.ny + j) * V.nz + k) * 3 + ax;
                    }
                    ++vi;
                }
            }
        }
        base += total;
    }
}

// smap: brick -> its position in the brick list (or -1), for the vertex ids of the neighbour bricks' points
__global__ __launch_bounds__(kMT) void mcs_faces_kernel(const int32_t *__restrict__ bricks, BrickVol V,
                                                        const int32_t *__restrict__ smap, int64_t n,
                                                        const uint16_t *__restrict__ code,
                                                        const int32_t *__restrict__ vbase,
                                                        const int64_t *__restrict__ boff, int64_t cap_f,
                                                        int32_t *__restrict__ faces, int64_t *__restrict__ fkeys) {
    __shared__ int lds_waves[kMT / 64];
    const int64_t beg = (int64_t)blockIdx.x * kMBlock;
    int64_t base = boff[blockIdx.x];
    for (int r = 0; r < kMRounds; ++r) {
        if (beg + (int64_t)r * kMT >= n) break;
        const int64_t q = beg + (int64_t)r * kMT + threadIdx.x;
        const int cs = q < n ? code[q] & 255 : 0;
        const int nt = hm_mc_tris[cs][0];
        int total;
        const int pre = block_excl_scan(nt, lds_waves, total);
        int64_t f = base + pre;
        int i = 0, j = 0, k = 0;
        if (nt) mcs_point(q, bricks, V, i, j, k);
        for (int t = 0; t < nt; ++t, ++f) {
            if (f >= cap_f) break;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const int e = hm_mc_tris[cs][1 + 3 * t + m];
                const int c = hm_mc_edge_corner[e], ax = hm_mc_edge_axis[e];
                const int ci = i + (c & 1), cj = j + ((c >> 1) & 1), ck = k + ((c >> 2) & 1);
                const int64_t s = smap[V.brick_of(ci, cj, ck)];
                int32_t id = -1;   // the corner's brick is not listed: the caller's closure is broken
                if (s >= 0 && s * kB3 < n) {
                    const int64_t p = s * kB3 + ((ci & 7) << 6 | (cj & 7) << 3 | (ck & 7));
                    const int pmask = code[p] >> 8;
                    id = vbase[p] + __popc(pmask & ((1 << ax) - 1));
                }
                faces[f * 3 + m] = id;
            }
            fkeys[f] = (((int64_t)i * V.ny + j) * V.nz + k) * 8 + t;
        }
        base += total;
    }
}

int mcs_check_dims(int64_t nx, int64_t ny, int64_t nz, const std::string &w) {
    HM_CHECK_ARG(nx >= 2 && ny >= 2 && nz >= 2, w + ": every lattice dimension must be >= 2");
    HM_CHECK_ARG(nx <= HM_MCS_MAX_DIM && ny <= HM_MCS_MAX_DIM && nz <= HM_MCS_MAX_DIM,
                 w + ": every lattice dimension must be <= 65536");
    return HM_OK;
}

int64_t bricks_along(int64_t n) { return (n + kB - 1) / kB; }

int mcs_check_lattice(const hm_mcs_lattice *lat, const std::string &w) {
    HM_CHECK_ARG(lat != nullptr, w + ": lattice is NULL");
    if (int rc = mcs_check_dims(lat->nx, lat->ny, lat->nz, w)) return rc;
    HM_CHECK_ARG(lat->map != nullptr, w + ": brick map is NULL");
    HM_CHECK_ARG(lat->n_slots >= 0 && lat->n_slots <= INT32_MAX, w + ": n_slots must be in [0, 2^31)");
    HM_CHECK_ARG(lat->n_slots == 0 || lat->pool != nullptr, w + ": value pool is NULL");
    return HM_OK;
}

BrickVol brick_vol(const hm_mcs_lattice *lat) {
    return BrickVol{lat->pool, lat->map, lat->n_slots, (int32_t)lat->nx, (int32_t)lat->ny, (int32_t)lat->nz,
                    (int32_t)bricks_along(lat->nx), (int32_t)bricks_along(lat->ny), (int32_t)bricks_along(lat->nz)};
}

int mcs_check_list(const int32_t *bricks, int64_t n_bricks, const std::string &w) {
    HM_CHECK_ARG(n_bricks >= 0 && n_bricks <= HM_MCS_MAX_LIST, w + ": n_bricks must be in [0, 2^22]");
    HM_CHECK_ARG(n_bricks == 0 || bricks != nullptr, w + ": brick list is NULL");
    return HM_OK;
}

int mcs_points_args(const float *ax, const float *ay, const float *az, int64_t nx, int64_t ny, int64_t nz,
                    const float *xform, float *out, const std::string &w, LatAxes &A, LatXform &X) {
    if (int rc = mcs_check_dims(nx, ny, nz, w)) return rc;
    HM_CHECK_ARG(ax && ay && az, w + ": NULL axis");
    HM_CHECK_ARG(out != nullptr, w + ": NULL output");
    A = LatAxes{ax, ay, az, (int32_t)nx, (int32_t)ny, (int32_t)nz};
    X.on = xform != nullptr;
    for (int m = 0; m < 9; ++m) X.r[m] = xform ? xform[m] : 0.0f;
    for (int m = 0; m < 3; ++m) X.s[m] = xform ? xform[9 + m] : 0.0f;
    return HM_OK;
}

}  // namespace

extern "C" {

int hm_mcs_points_bricks(const int32_t *bricks, int64_t n_bricks, const float *ax, const float *ay, const float *az,
                         int64_t nx, int64_t ny, int64_t nz, const float *xform, float *points, void *stream) {
    LatAxes A;
    LatXform X;
    if (int rc = mcs_check_list(bricks, n_bricks, "hm_mcs_points_bricks")) return rc;
    if (n_bricks == 0) return HM_OK;
    if (int rc = mcs_points_args(ax, ay, az, nx, ny, nz, xform, points, "hm_mcs_points_bricks", A, X)) return rc;
    const int64_t n = n_bricks * kB3;
    hipLaunchKernelGGL(mcs_points_bricks_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream),
                       bricks, n, A, X, (int32_t)bricks_along(ny), (int32_t)bricks_along(nz), points);
    HM_CHECK_LAUNCH("hm_mcs_points_bricks");
    return HM_OK;
}

int hm_mcs_points_index(const int64_t *index, int64_t n, const float *ax, const float *ay, const float *az, int64_t nx,
                        int64_t ny, int64_t nz, const float *xform, float *points, void *stream) {
    LatAxes A;
    LatXform X;
    HM_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "hm_mcs_points_index: n must be in [0, 2^31)");
    if (n == 0) return HM_OK;
    HM_CHECK_ARG(index != nullptr, "hm_mcs_points_index: NULL index");
    if (int rc = mcs_points_args(ax, ay, az, nx, ny, nz, xform, points, "hm_mcs_points_index", A, X)) return rc;
    hipLaunchKernelGGL(mcs_points_index_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream),
                       index, n, A, X, points);
    HM_CHECK_LAUNCH("hm_mcs_points_index");
    return HM_OK;
}

int hm_mcs_status(const int32_t *bricks, int64_t n_bricks, const hm_mcs_lattice *lat, float level, int32_t *status,
                  void *stream) {
    if (int rc = mcs_check_list(bricks, n_bricks, "hm_mcs_status")) return rc;
    if (int rc = mcs_check_lattice(lat, "hm_mcs_status")) return rc;
    HM_CHECK_ARG(level == level, "hm_mcs_status: level is NaN");
    if (n_bricks == 0) return HM_OK;
    HM_CHECK_ARG(status != nullptr, "hm_mcs_status: NULL status");
    hipLaunchKernelGGL(mcs_status_kernel, dim3((unsigned)n_bricks), dim3(256), 0, as_stream(stream), bricks,
                       brick_vol(lat), level, status);
    HM_CHECK_LAUNCH("hm_mcs_status");
    return HM_OK;
}

int64_t hm_mcs_workspace_bytes(int64_t n_bricks) {
    if (n_bricks < 1 || n_bricks > HM_MCS_MAX_LIST)
        return hm_fail(HM_ERR_INVALID, "hm_mcs_workspace_bytes: n_bricks must be in [1, 2^22]");
    return mc_ws_bytes(n_bricks * kB3);
}

int hm_mcs_count(const int32_t *bricks, int64_t n_bricks, const hm_mcs_lattice *lat, float level, void *workspace,
                 int64_t workspace_bytes, int64_t *counts, void *stream) {
    if (int rc = mcs_check_list(bricks, n_bricks, "hm_mcs_count")) return rc;
    HM_CHECK_ARG(n_bricks >= 1, "hm_mcs_count: empty brick list");
    if (int rc = mcs_check_lattice(lat, "hm_mcs_count")) return rc;
    HM_CHECK_ARG(workspace && counts, "hm_mcs_count: NULL workspace or counts");
    HM_CHECK_ARG(workspace_bytes >= hm_mcs_workspace_bytes(n_bricks), "hm_mcs_count: workspace too small");
    HM_CHECK_ARG(level == level, "hm_mcs_count: level is NaN");
    const int64_t n = n_bricks * kB3, nb = (n + kMBlock - 1) / kMBlock;
    const McWs w = mc_carve(workspace, n);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(mcs_classify_kernel, dim3((unsigned)nb), dim3(kMT), 0, st, bricks, brick_vol(lat), level, n,
                       w.code, w.bsum, nb);
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(kScanT), 0, st, static_cast<const int32_t *>(w.bsum), nb, w.boff,
                       counts);
    HM_CHECK_LAUNCH("hm_mcs_count");
    return HM_OK;
}

int hm_mcs_emit(const int32_t *bricks, int64_t n_bricks, const hm_mcs_lattice *lat, const int32_t *list_pos,
                float level, const float *spacing, void *workspace, int64_t workspace_bytes, int64_t n_verts,
                int64_t n_faces, float *verts, float *normals, int32_t *faces, int64_t *vert_keys, int64_t *face_keys,
                void *stream) {
    if (int rc = mcs_check_list(bricks, n_bricks, "hm_mcs_emit")) return rc;
    HM_CHECK_ARG(n_bricks >= 1, "hm_mcs_emit: empty brick list");
    if (int rc = mcs_check_lattice(lat, "hm_mcs_emit")) return rc;
    HM_CHECK_ARG(workspace && spacing && list_pos, "hm_mcs_emit: NULL workspace, spacing or list_pos");
    HM_CHECK_ARG(workspace_bytes >= hm_mcs_workspace_bytes(n_bricks), "hm_mcs_emit: workspace too small");
    HM_CHECK_ARG(n_verts >= 0 && n_faces >= 0, "hm_mcs_emit: negative count");
    HM_CHECK_ARG(n_verts <= INT32_MAX && n_faces <= INT32_MAX,
                 "hm_mcs_emit: " + std::to_string(n_verts) + " vertices / " + std::to_string(n_faces) +
                     " faces do not fit int32 indices");
    HM_CHECK_ARG(n_verts == 0 || (verts && normals && vert_keys), "hm_mcs_emit: NULL verts, normals or vert_keys");
    HM_CHECK_ARG(n_faces == 0 || (faces && face_keys), "hm_mcs_emit: NULL faces or face_keys");
    const int64_t n = n_bricks * kB3, nb = (n + kMBlock - 1) / kMBlock;
    const McWs w = mc_carve(workspace, n);
    const BrickVol V = brick_vol(lat);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(mcs_verts_kernel, dim3((unsigned)nb), dim3(kMT), 0, st, bricks, V, level, spacing[0],
                       spacing[1], spacing[2], n, static_cast<const uint16_t *>(w.code), w.vbase,
                       static_cast<const int64_t *>(w.boff), n_verts, verts, normals, vert_keys);
    if (n_faces > 0)
        hipLaunchKernelGGL(mcs_faces_kernel, dim3((unsigned)nb), dim3(kMT), 0, st, bricks, V, list_pos, n,
                           static_cast<const uint16_t *>(w.code), static_cast<const int32_t *>(w.vbase),
                           static_cast<const int64_t *>(w.boff + nb), n_faces, faces, face_keys);
    HM_CHECK_LAUNCH("hm_mcs_emit");
    return HM_OK;
}

}  // extern "C"
