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
//   hm_mcs_count / hm_mcs_emit      the two phases of hm_mesh.hip over the points of the listed (surface) bricks: the
//                                   kernels of hm_mesh_dev.h, the ones the dense volume runs, over the lattice BrickLat
//                                   (values through the brick map, work items through the brick list and its position
//                                   map).  A cell or an edge with a corner that is not evaluated emits nothing.
//                                   Outputs come in list order with an int64 key each; sorted by key they are the dense
//                                   kernels' outputs.
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
    below = hm_wave_reduce(below, HmOr{});
    above = hm_wave_reduce(above, HmOr{});
    nan = hm_wave_reduce(nan, HmOr{});
    missing = hm_wave_reduce(missing, HmOr{});
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

// the brick lattice: work item q is point q & 511 of listed brick q >> 9.  smap: brick -> its position in the brick list
// (or -1), for the work items of the neighbour bricks' points; vkeys / fkeys: the dense linear order of each output
struct BrickLat : BrickVol {
    const int32_t *bricks, *smap;
    int64_t n;   // work items: listed bricks * 512
    int64_t *vkeys, *fkeys;
    __device__ __forceinline__ bool point(int64_t q, int &i, int &j, int &k) const {
        return mcs_point(q, bricks, *this, i, j, k);
    }
    // false: the corner's brick is not listed, the caller's closure is broken
    __device__ __forceinline__ bool corner(int64_t, int i, int j, int k, int c, int64_t &p) const {
        const int ci = i + (c & 1), cj = j + ((c >> 1) & 1), ck = k + ((c >> 2) & 1);
        const int64_t s = smap[brick_of(ci, cj, ck)];
        p = s * kB3 + ((ci & 7) << 6 | (cj & 7) << 3 | (ck & 7));
        return s >= 0 && s * kB3 < n;
    }
    __device__ __forceinline__ void vert_key(int64_t vi, int i, int j, int k, int ax) const {
        vkeys[vi] = (((int64_t)i * ny + j) * nz + k) * 3 + ax;
    }
    __device__ __forceinline__ void face_key(int64_t f, int i, int j, int k, int t) const {
        fkeys[f] = (((int64_t)i * ny + j) * nz + k) * 8 + t;
    }
};

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

// the lattice of hm_mcs_count / hm_mcs_emit; the count phase uses neither the position map nor the keys
BrickLat brick_lat(const hm_mcs_lattice *lat, const int32_t *bricks, int64_t n_bricks, const int32_t *list_pos = nullptr,
                   int64_t *vert_keys = nullptr, int64_t *face_keys = nullptr) {
    return BrickLat{brick_vol(lat), bricks, list_pos, n_bricks * kB3, vert_keys, face_keys};
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
    return mc_layout(nullptr, n_bricks * kB3).bytes;
}

int hm_mcs_count(const int32_t *bricks, int64_t n_bricks, const hm_mcs_lattice *lat, float level, void *workspace,
                 int64_t workspace_bytes, int64_t *counts, void *stream) {
    if (int rc = mcs_check_list(bricks, n_bricks, "hm_mcs_count")) return rc;
    HM_CHECK_ARG(n_bricks >= 1, "hm_mcs_count: empty brick list");
    if (int rc = mcs_check_lattice(lat, "hm_mcs_count")) return rc;
    HM_CHECK_ARG(workspace && counts, "hm_mcs_count: NULL workspace or counts");
    HM_CHECK_ARG(workspace_bytes >= hm_mcs_workspace_bytes(n_bricks), "hm_mcs_count: workspace too small");
    HM_CHECK_ARG(level == level, "hm_mcs_count: level is NaN");
    const BrickLat V = brick_lat(lat, bricks, n_bricks);
    const McWs w = mc_layout(workspace, V.n);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(mc_classify_kernel<BrickLat>, dim3((unsigned)w.nb), dim3(kMT), 0, st, V, level, V.n, w.code,
                       w.bsum, w.nb);
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(kScanT), 0, st, static_cast<const int32_t *>(w.bsum), w.nb, w.boff,
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
    const BrickLat V = brick_lat(lat, bricks, n_bricks, list_pos, vert_keys, face_keys);
    const McWs w = mc_layout(workspace, V.n);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(mc_verts_kernel<BrickLat>, dim3((unsigned)w.nb), dim3(kMT), 0, st, V, level, spacing[0],
                       spacing[1], spacing[2], V.n, static_cast<const uint16_t *>(w.code), w.vbase,
                       static_cast<const int64_t *>(w.boff), n_verts, verts, normals);
    if (n_faces > 0)
        hipLaunchKernelGGL(mc_faces_kernel<BrickLat>, dim3((unsigned)w.nb), dim3(kMT), 0, st, V, V.n,
                           static_cast<const uint16_t *>(w.code), static_cast<const int32_t *>(w.vbase),
                           static_cast<const int64_t *>(w.boff + w.nb), n_faces, faces);
    HM_CHECK_LAUNCH("hm_mcs_emit");
    return HM_OK;
}

}  // extern "C"
