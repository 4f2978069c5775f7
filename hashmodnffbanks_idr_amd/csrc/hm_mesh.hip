// hm_mesh.hip - marching cubes of a device fp32 volume (reference: skimage.measure.marching_cubes as plots.py:122-128
// calls it; topology from the generated case table hm_mc_table.h, see scripts/gen_mc_table.py).  The kernels are
// hm_mesh_dev.h's, written over a lattice type; this file supplies the dense lattice McVol, the checks and the launches.
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
// hm_mesh_sparse.hip runs the same kernels over the listed bricks of a value pool.
#include "hm_mesh_dev.h"

namespace {

// the dense lattice: work item q is the point of linear index q = (i*ny + j)*nz + k
struct McVol {
    const float *v;
    int32_t nx, ny, nz;
    int64_t sx, sy, sz;
    __device__ __forceinline__ float at(int i, int j, int k) const {
        return v[(int64_t)i * sx + (int64_t)j * sy + (int64_t)k * sz];
    }
    __device__ __forceinline__ bool has(int, int, int) const { return true; }
    __device__ __forceinline__ bool point(int64_t q, int &i, int &j, int &k) const {
        const uint32_t u = (uint32_t)q;
        k = (int)(u % (uint32_t)nz);
        const uint32_t r = u / (uint32_t)nz;
        j = (int)(r % (uint32_t)ny);
        i = (int)(r / (uint32_t)ny);
        return true;
    }
    __device__ __forceinline__ bool corner(int64_t q, int, int, int, int c, int64_t &p) const {
        p = q + (c & 1) * ((int64_t)ny * nz) + ((c >> 1) & 1) * (int64_t)nz + ((c >> 2) & 1);
        return true;
    }
    __device__ __forceinline__ void vert_key(int64_t, int, int, int, int) const {}
    __device__ __forceinline__ void face_key(int64_t, int, int, int, int) const {}
};

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
    return mc_layout(nullptr, nx * ny * nz).bytes;
}

int hm_mc_count(const float *vol, int64_t nx, int64_t ny, int64_t nz, int64_t sx, int64_t sy, int64_t sz, float level,
                void *workspace, int64_t workspace_bytes, int64_t *counts, void *stream) {
    if (int rc = mc_check_volume(vol, nx, ny, nz, sx, sy, sz, "hm_mc_count")) return rc;
    HM_CHECK_ARG(workspace && counts, "hm_mc_count: NULL workspace or counts");
    HM_CHECK_ARG(workspace_bytes >= hm_mc_workspace_bytes(nx, ny, nz), "hm_mc_count: workspace too small");
    HM_CHECK_ARG(level == level, "hm_mc_count: level is NaN");
    const int64_t n = nx * ny * nz;
    const McVol V{vol, (int32_t)nx, (int32_t)ny, (int32_t)nz, sx, sy, sz};
    const McWs w = mc_layout(workspace, n);
    const int64_t nb = w.nb;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(mc_classify_kernel<McVol>, dim3((unsigned)nb), dim3(kMT), 0, st, V, level, n, w.code, w.bsum, nb);
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
    const int64_t n = nx * ny * nz;
    const McVol V{vol, (int32_t)nx, (int32_t)ny, (int32_t)nz, sx, sy, sz};
    const McWs w = mc_layout(workspace, n);
    const int64_t nb = w.nb;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(mc_verts_kernel<McVol>, dim3((unsigned)nb), dim3(kMT), 0, st, V, level, spacing[0], spacing[1],
                       spacing[2], n, static_cast<const uint16_t *>(w.code), w.vbase,
                       static_cast<const int64_t *>(w.boff), n_verts, verts, normals);
    if (n_faces > 0)
        hipLaunchKernelGGL(mc_faces_kernel<McVol>, dim3((unsigned)nb), dim3(kMT), 0, st, V, n,
                           static_cast<const uint16_t *>(w.code), static_cast<const int32_t *>(w.vbase),
                           static_cast<const int64_t *>(w.boff + nb), n_faces, faces);
    HM_CHECK_LAUNCH("hm_mc_emit");
    return HM_OK;
}

}  // extern "C"
