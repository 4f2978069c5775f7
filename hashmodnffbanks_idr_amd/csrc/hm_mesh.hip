// hm_mesh.hip - marching cubes of a device fp32 volume (reference: skimage.measure.marching_cubes as plots.py:122-128
// calls it; topology from the generated case table hm_mc_table.h, see scripts/gen_mc_table.py).
//
// The output size depends on the data, so there are two phases around one host read of the totals:
//   hm_mc_count  mc_classify   per lattice point: the sign-changing lattice edges it owns (+x, +y, +z) and the case of
//                              the cell it is the lowest corner of -> a uint16 code; per 4096-point block: vertex and
//                              triangle sums and a NaN bit
//                mc_scan       one workgroup: exclusive prefix of the block sums, the int64 totals and the NaN flag
//   hm_mc_emit   mc_verts      per point: vertex base = block offset + in-block prefix (-> vbase, int32), its vertices
//                              (linear interpolation on the edge) and normals (interpolated central differences)
//                mc_faces      per cell: face base likewise; each edge of a table triangle is the vertex
//                              vbase[q] + (its axis' rank among q's crossing axes) of one of the cell's 8 points q
// Order of the outputs: vertices by owning point (linear index (i*ny + j)*nz + k), then axis x < y < z; faces by cell
// linear index, then table order - independent of the volume's strides.  No atomics: two calls give the same bits.
// Workspace: 2 B (code) + 4 B (vbase) per lattice point + 32 B per block.
// The scans, the gradient and the vertex arithmetic are in hm_mesh_dev.h, shared with hm_mesh_sparse.hip.
#include "hm_mc_table.h"
#include "hm_mesh_dev.h"

namespace {

struct McVol {
    const float *v;
    int32_t nx, ny, nz;
    int64_t sx, sy, sz;
    __device__ __forceinline__ float at(int i, int j, int k) const {
        return v[(int64_t)i * sx + (int64_t)j * sy + (int64_t)k * sz];
    }
};

__device__ __forceinline__ void mc_point(int64_t q, const McVol &V, int &i, int &j, int &k) {
    const uint32_t u = (uint32_t)q;
    k = (int)(u % (uint32_t)V.nz);
    const uint32_t r = u / (uint32_t)V.nz;
    j = (int)(r % (uint32_t)V.ny);
    i = (int)(r / (uint32_t)V.ny);
}

__global__ __launch_bounds__(kMT) void mc_classify_kernel(McVol V, float level, int64_t n, uint16_t *__restrict__ code,
                                                          int32_t *__restrict__ bsum, int64_t nb) {
    const int64_t beg = (int64_t)blockIdx.x * kMBlock;
    int nv = 0, nt = 0, nan = 0;
    for (int r = 0; r < kMRounds; ++r) {
        const int64_t q = beg + (int64_t)r * kMT + threadIdx.x;
        if (q >= n) break;
        int i, j, k;
        mc_point(q, V, i, j, k);
        const float c0 = V.at(i, j, k);
        nan |= c0 != c0;
        const bool in0 = c0 < level;
        const bool hx = i + 1 < V.nx, hy = j + 1 < V.ny, hz = k + 1 < V.nz;
        // corner values of the cell (i, j, k) .. (i+1, j+1, k+1); only the ones that exist are read
        const float c1 = hx ? V.at(i + 1, j, k) : c0;
        const float c2 = hy ? V.at(i, j + 1, k) : c0;
        const float c4 = hz ? V.at(i, j, k + 1) : c0;
        const int mask = ((hx && (c1 < level) != in0) ? 1 : 0) | ((hy && (c2 < level) != in0) ? 2 : 0) |
                         ((hz && (c4 < level) != in0) ? 4 : 0);
        int cs = 0;
        if (hx && hy && hz) {
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

__global__ __launch_bounds__(kMT) void mc_verts_kernel(McVol V, float level, float spx, float spy, float spz, int64_t n,
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
        int total;
        const int pre = block_excl_scan(__popc(mask), lds_waves, total);
        if (q < n) {
            int64_t vi = base + pre;
            vbase[q] = (int32_t)vi;
            if (mask) {
                int i, j, k;
                mc_point(q, V, i, j, k);
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
                    }
                    ++vi;
                }
            }
        }
        base += total;
    }
}

__global__ __launch_bounds__(kMT) void mc_faces_kernel(McVol V, int64_t n, const uint16_t *__restrict__ code,
                                                       const int32_t *__restrict__ vbase,
                                                       const int64_t *__restrict__ boff, int64_t cap_f,
                                                       int32_t *__restrict__ faces) {
    __shared__ int lds_waves[kMT / 64];
    const int64_t beg = (int64_t)blockIdx.x * kMBlock;
    const int64_t sj = V.nz, si = (int64_t)V.ny * V.nz;
    int64_t base = boff[blockIdx.x];
    for (int r = 0; r < kMRounds; ++r) {
        if (beg + (int64_t)r * kMT >= n) break;
        const int64_t q = beg + (int64_t)r * kMT + threadIdx.x;
        const int cs = q < n ? code[q] & 255 : 0;
        const int nt = hm_mc_tris[cs][0];
        int total;
        const int pre = block_excl_scan(nt, lds_waves, total);
        int64_t f = base + pre;
        for (int t = 0; t < nt; ++t, ++f) {
            if (f >= cap_f) break;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const int e = hm_mc_tris[cs][1 + 3 * t + m];
                const int c = hm_mc_edge_corner[e], ax = hm_mc_edge_axis[e];
                const int64_t p = q + (c & 1) * si + ((c >> 1) & 1) * sj + ((c >> 2) & 1);
                const int pmask = code[p] >> 8;
                faces[f * 3 + m] = vbase[p] + __popc(pmask & ((1 << ax) - 1));
            }
        }
        base += total;
    }
}

int mc_check_volume(const float *vol, int64_t nx, int64_t ny, int64_t nz, int64_t sx, int64_t sy, int64_t sz,
                    const char *what) {
    const std::string w(what);
    HM_CHECK_ARG(nx >= 2 && ny >= 2 && nz >= 2, w + ": every volume dimension must be >= 2");
    HM_CHECK_ARG(nx * ny * nz < ((int64_t)1 << 31), w + ": nx*ny*nz must be < 2^31");
    HM_CHECK_ARG(sx >= 0 && sy >= 0 && sz >= 0, w + ": negative stride");
    HM_CHECK_ARG(vol != nullptr, w + ": volume is NULL");
    return HM_OK;
}

}  // namespace

extern "C" {

int64_t hm_mc_workspace_bytes(int64_t nx, int64_t ny, int64_t nz) {
    if (nx < 2 || ny < 2 || nz < 2 || nx * ny * nz >= ((int64_t)1 << 31))
        return hm_fail(HM_ERR_INVALID, "hm_mc_workspace_bytes: dimensions must be >= 2 and nx*ny*nz < 2^31");
    return mc_ws_bytes(nx * ny * nz);
}

int hm_mc_count(const float *vol, int64_t nx, int64_t ny, int64_t nz, int64_t sx, int64_t sy, int64_t sz, float level,
                void *workspace, int64_t workspace_bytes, int64_t *counts, void *stream) {
    if (int rc = mc_check_volume(vol, nx, ny, nz, sx, sy, sz, "hm_mc_count")) return rc;
    HM_CHECK_ARG(workspace && counts, "hm_mc_count: NULL workspace or counts");
    HM_CHECK_ARG(workspace_bytes >= hm_mc_workspace_bytes(nx, ny, nz), "hm_mc_count: workspace too small");
    HM_CHECK_ARG(level == level, "hm_mc_count: level is NaN");
    const int64_t n = nx * ny * nz, nb = (n + kMBlock - 1) / kMBlock;
    const McVol V{vol, (int32_t)nx, (int32_t)ny, (int32_t)nz, sx, sy, sz};
    const McWs w = mc_carve(workspace, n);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(mc_classify_kernel, dim3((unsigned)nb), dim3(kMT), 0, st, V, level, n, w.code, w.bsum, nb);
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(kScanT), 0, st, static_cast<const int32_t *>(w.bsum), nb, w.boff,
                       counts);
    HM_CHECK_LAUNCH("hm_mc_count");
    return HM_OK;
}

int hm_mc_emit(const float *vol, int64_t nx, int64_t ny, int64_t nz, int64_t sx, int64_t sy, int64_t sz, float level,
               const float *spacing, void *workspace, int64_t workspace_bytes, int64_t n_verts, int64_t n_faces,
               float *verts, float *normals, int32_t *faces, void *stream) {
    if (int rc = mc_check_volume(vol, nx, ny, nz, sx, sy, sz, "hm_mc_emit")) return rc;
    HM_CHECK_ARG(workspace && spacing, "hm_mc_emit: NULL workspace or spacing");
    HM_CHECK_ARG(workspace_bytes >= hm_mc_workspace_bytes(nx, ny, nz), "hm_mc_emit: workspace too small");
    HM_CHECK_ARG(n_verts >= 0 && n_faces >= 0, "hm_mc_emit: negative count");
    HM_CHECK_ARG(n_verts <= INT32_MAX && n_faces <= INT32_MAX,
                 "hm_mc_emit: " + std::to_string(n_verts) + " vertices / " + std::to_string(n_faces) +
                     " faces do not fit int32 indices");
    HM_CHECK_ARG(n_verts == 0 || (verts && normals), "hm_mc_emit: NULL verts or normals");
    HM_CHECK_ARG(n_faces == 0 || faces, "hm_mc_emit: NULL faces");
    const int64_t n = nx * ny * nz, nb = (n + kMBlock - 1) / kMBlock;
    const McVol V{vol, (int32_t)nx, (int32_t)ny, (int32_t)nz, sx, sy, sz};
    const McWs w = mc_carve(workspace, n);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(mc_verts_kernel, dim3((unsigned)nb), dim3(kMT), 0, st, V, level, spacing[0], spacing[1],
                       spacing[2], n, static_cast<const uint16_t *>(w.code), w.vbase,
                       static_cast<const int64_t *>(w.boff), n_verts, verts, normals);
    if (n_faces > 0)
        hipLaunchKernelGGL(mc_faces_kernel, dim3((unsigned)nb), dim3(kMT), 0, st, V, n,
                           static_cast<const uint16_t *>(w.code), static_cast<const int32_t *>(w.vbase),
                           static_cast<const int64_t *>(w.boff + nb), n_faces, faces);
    HM_CHECK_LAUNCH("hm_mc_emit");
    return HM_OK;
}

}  // extern "C"
