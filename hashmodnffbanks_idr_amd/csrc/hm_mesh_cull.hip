// hm_mesh_cull.hip - culling an extracted mesh by what the cameras saw (contract: include/hashmod.h; driver:
// ops.mesh_mask_votes, ops.mesh_depth_maps, ops.mesh_visible_votes, ops.mesh_keep_vertices, evaluation/cull.py):
//
//   hm_mesh_mask_votes     one lane per vertex, a loop over the views: is the vertex in the image, and is a mask pixel
//                          set within `dilate` pixels of it (four reads of the masks' summed-area table)
//   hm_mesh_depth_maps     per view: cull_project (one lane per vertex: fixed-point position and 1/w into a buffer),
//                          cull_raster (one lane per face: the pixel centres of its bounding box; a box of more than
//                          big_face pixels goes to a list), cull_raster_big (one wave per listed face)
//   hm_mesh_visible_votes  one lane per vertex, a loop over the views: w against the largest depth around its pixel
//   hm_mesh_keep_mark      the face and vertex flags of "all three vertices kept", for hm_mesh_select_emit
//
// The projection, the pixel, the fixed-point position and the visibility rule are hm_view_dev.h's (the rule is also the
// colours': hm_mesh_color.hip); the projection kernel, the face set-up, the coverage test and the depth of a covered
// pixel are hm_raster_dev.h's, shared with the renderer (hm_mesh_render.hip).  Coverage is decided by int64 edge
// functions of the fixed-point positions, the depth by fp64 operations rounded once, and a pixel keeps the minimum through an unsigned atomicMin on the float's bits (positive floats order like their bits): the
// depth maps do not depend on the order of the faces and two calls give the same bits.  The votes are written once per
// vertex, without atomics.  No index is dereferenced before its range check.
#include "hm_raster_dev.h"

namespace {

constexpr int kVT = kRasterVT;
constexpr int kBigBlocks = kRasterBigBlocks;
constexpr uint32_t kInfBits = 0x7f800000u;

CullWs cull_layout(void *ws, int64_t n_verts, int64_t n_faces) {
    HmCarve c(ws);
    return cull_layout(c, n_verts, n_faces);
}

__global__ __launch_bounds__(kVT) void cull_fill_kernel(uint32_t *__restrict__ p, int64_t n, uint32_t value) {
    const int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x;
    if (i < n) p[i] = value;
}

// sat: [n_views, H + 1, W + 1] int32, sat[v][r][c] = the number of set mask pixels in rows < r and columns < c
__global__ __launch_bounds__(kVT) void cull_mask_votes_kernel(const float *__restrict__ verts, int64_t n_verts,
                                                              const double *__restrict__ proj, int n_views,
                                                              const int32_t *__restrict__ sat, int H, int W, int dilate,
                                                              int accumulate, int32_t *__restrict__ n_in_image,
                                                              int32_t *__restrict__ n_in_mask) {
    const int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x;
    if (i >= n_verts) return;
    const float x = verts[i * 3], y = verts[i * 3 + 1], z = verts[i * 3 + 2];
    int n_img = 0, n_msk = 0;
    const int64_t pitch = (int64_t)W + 1, plane = ((int64_t)H + 1) * pitch;
    for (int v = 0; v < n_views; ++v) {
        int32_t col, row;
        if (!hm_view_pixel(hm_view_project(proj + (int64_t)v * 12, x, y, z), H, W, col, row)) continue;
        ++n_img;
        const int c0 = max(col - dilate, 0), c1 = min(col + dilate, W - 1) + 1;
        const int r0 = max(row - dilate, 0), r1 = min(row + dilate, H - 1) + 1;
        const int32_t *s = sat + (int64_t)v * plane;
        const int32_t set = (s[r1 * pitch + c1] - s[r0 * pitch + c1]) - (s[r1 * pitch + c0] - s[r0 * pitch + c0]);
        n_msk += set > 0;
    }
    n_in_image[i] = (accumulate ? n_in_image[i] : 0) + n_img;
    n_in_mask[i] = (accumulate ? n_in_mask[i] : 0) + n_msk;
}

// the pixel (col, row) of the box: covered iff E_0, E_1, E_2 are all >= 0 or all <= 0; then depth = min(depth, z)
__device__ __forceinline__ void cull_pixel(const Tri &t, int col, int row, int W, uint32_t *__restrict__ depth) {
    raster_pixel(t, col, row, [&](float z) { atomicMin(depth + (int64_t)row * W + col, __float_as_uint(z)); });
}

__global__ __launch_bounds__(kVT) void cull_raster_kernel(const ViewVert *__restrict__ pv,
                                                          const int32_t *__restrict__ faces, int64_t n_faces,
                                                          int64_t n_verts, int H, int W, int64_t big_face,
                                                          uint32_t *__restrict__ depth, int32_t *__restrict__ n_skipped,
                                                          int32_t *__restrict__ list, uint32_t *__restrict__ count,
                                                          int32_t *status) {
    const int64_t f = (int64_t)blockIdx.x * kVT + threadIdx.x;
    if (f >= n_faces) return;
    int32_t id[3];
    if (!hm_face_ids(faces, f, n_verts, id, status)) return;
    Tri t;
    const int kind = cull_tri(pv, id, H, W, t);
    if (kind == kTriSkipped) atomicAdd(n_skipped, 1);
    if (kind != kTriDraw) return;
    if ((int64_t)(t.c1 - t.c0 + 1) * (t.r1 - t.r0 + 1) > big_face) {
        const uint32_t slot = atomicAdd(count, 1u);
        if (slot < (uint64_t)n_faces) list[slot] = (int32_t)f;
        return;
    }
    for (int row = t.r0; row <= t.r1; ++row)
        for (int col = t.c0; col <= t.c1; ++col) cull_pixel(t, col, row, W, depth);
}

// one wave per listed face, 64 pixels of its box per round (H*W < 2^31: the box fits uint32)
__global__ __launch_bounds__(kVT) void cull_raster_big_kernel(const ViewVert *__restrict__ pv,
                                                              const int32_t *__restrict__ faces, int64_t n_faces,
                                                              int64_t n_verts, int H, int W,
                                                              uint32_t *__restrict__ depth,
                                                              const int32_t *__restrict__ list,
                                                              const uint32_t *__restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * kVT + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * (kVT / 64);
    const int64_t n = min((int64_t)*count, n_faces);
    for (int64_t i = wave; i < n; i += n_waves) {
        const int64_t f = list[i];
        int32_t id[3];
        if (f < 0 || f >= n_faces || !hm_face_ids(faces, f, n_verts, id)) continue;
        Tri t;
        if (cull_tri(pv, id, H, W, t) != kTriDraw) continue;
        const uint32_t bw = (uint32_t)(t.c1 - t.c0 + 1), total = bw * (uint32_t)(t.r1 - t.r0 + 1);
        for (uint32_t p = lane; p < total; p += 64) cull_pixel(t, t.c0 + (int)(p % bw), t.r0 + (int)(p / bw), W, depth);
    }
}

__global__ __launch_bounds__(kVT) void cull_visible_votes_kernel(const float *__restrict__ verts, int64_t n_verts,
                                                                 const double *__restrict__ proj, int n_views,
                                                                 const float *__restrict__ depth, int H, int W, int pad,
                                                                 float tol, int accumulate,
                                                                 int32_t *__restrict__ n_visible) {
    const int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x;
    if (i >= n_verts) return;
    const float x = verts[i * 3], y = verts[i * 3 + 1], z = verts[i * 3 + 2];
    int n_vis = 0;
    for (int v = 0; v < n_views; ++v) {
        const HmViewPoint q = hm_view_project(proj + (int64_t)v * 12, x, y, z);
        int32_t col, row;
        if (!hm_view_pixel(q, H, W, col, row)) continue;
        n_vis += hm_view_visible(q, depth + (int64_t)v * H * W, H, W, col, row, pad, tol);
    }
    n_visible[i] = (accumulate ? n_visible[i] : 0) + n_vis;
}

__global__ __launch_bounds__(kVT) void cull_keep_mark_kernel(const int32_t *__restrict__ faces, int64_t n_faces,
                                                             int64_t n_verts, const uint8_t *__restrict__ keep,
                                                             int32_t *__restrict__ vflag, int32_t *__restrict__ fflag,
                                                             int32_t *status) {
    const int64_t f = (int64_t)blockIdx.x * kVT + threadIdx.x;
    if (f >= n_faces) return;
    int32_t v[3];
    const bool in = hm_face_ids(faces, f, n_verts, v, status) && keep[v[0]] && keep[v[1]] && keep[v[2]];
    fflag[f] = in ? 1 : 0;
    if (in) {
#pragma unroll
        for (int m = 0; m < 3; ++m) vflag[v[m]] = 1;
    }
}

}  // namespace

extern "C" {

int hm_mesh_mask_votes(const float *verts, int64_t n_verts, const double *proj, int64_t n_views, const int32_t *sat,
                       int64_t H, int64_t W, int64_t dilate, int accumulate, int32_t *n_in_image, int32_t *n_in_mask,
                       void *stream) {
    if (int rc = hm_check_mesh(0, n_verts, nullptr, "hm_mesh_mask_votes")) return rc;
    if (int rc = hm_view_check_image(n_views, H, W, "hm_mesh_mask_votes")) return rc;
    HM_CHECK_ARG(dilate >= 0, "hm_mesh_mask_votes: dilate must be >= 0");
    if (n_verts == 0) return HM_OK;
    HM_CHECK_ARG(verts && n_in_image && n_in_mask && (n_views == 0 || (proj && sat)), "hm_mesh_mask_votes: NULL pointer");
    const int r = (int)(dilate < 65536 ? dilate : 65536);   // a radius beyond the image is the whole image
    hipLaunchKernelGGL(cull_mask_votes_kernel, dim3(hm_grid(n_verts, kVT)), dim3(kVT), 0, as_stream(stream), verts,
                       n_verts, proj, (int)n_views, sat, (int)H, (int)W, r, accumulate, n_in_image, n_in_mask);
    HM_CHECK_LAUNCH("hm_mesh_mask_votes");
    return HM_OK;
}

int64_t hm_mesh_depth_workspace_bytes(int64_t n_verts, int64_t n_faces) {
    if (n_verts < 0 || n_verts >= ((int64_t)1 << 31) || n_faces < 0 || n_faces >= ((int64_t)1 << 31))
        return hm_fail(HM_ERR_INVALID, "hm_mesh_depth_workspace_bytes: n_verts and n_faces must be in [0, 2^31)");
    return cull_layout(nullptr, n_verts, n_faces).bytes;
}

int hm_mesh_depth_maps(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const double *proj,
                       int64_t n_views, int64_t H, int64_t W, int64_t big_face, float *depth, int32_t *n_skipped,
                       void *workspace, int64_t workspace_bytes, int32_t *status, void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_depth_maps")) return rc;
    if (int rc = hm_view_check_image(n_views, H, W, "hm_mesh_depth_maps")) return rc;
    HM_CHECK_ARG(big_face >= 1, "hm_mesh_depth_maps: big_face must be >= 1");
    if (n_views == 0) return HM_OK;
    HM_CHECK_ARG(proj && depth && n_skipped && status && workspace && (n_verts == 0 || verts),
                 "hm_mesh_depth_maps: NULL pointer");
    HM_CHECK_ARG(workspace_bytes >= cull_layout(nullptr, n_verts, n_faces).bytes,
                 "hm_mesh_depth_maps: workspace too small");
    const CullWs w = cull_layout(workspace, n_verts, n_faces);
    hipStream_t st = as_stream(stream);
    uint32_t *bits = reinterpret_cast<uint32_t *>(depth);
    const int64_t pixels = H * W;
    hm_zero_u32_async(n_skipped, n_views, st);
    for (int64_t v = 0; v < n_views; ++v) {
        hipLaunchKernelGGL(cull_fill_kernel, dim3(hm_grid(pixels, kVT)), dim3(kVT), 0, st, bits + v * pixels, pixels,
                           kInfBits);
        if (n_faces == 0) continue;
        hipLaunchKernelGGL(cull_project_kernel, dim3(hm_grid(n_verts > 0 ? n_verts : 1, kVT)), dim3(kVT), 0, st, verts,
                           n_verts, proj + v * 12, w.pv, w.count);
        hipLaunchKernelGGL(cull_raster_kernel, dim3(hm_grid(n_faces, kVT)), dim3(kVT), 0, st,
                           static_cast<const ViewVert *>(w.pv), faces, n_faces, n_verts, (int)H, (int)W, big_face,
                           bits + v * pixels, n_skipped + v, w.list, w.count, status);
        hipLaunchKernelGGL(cull_raster_big_kernel, dim3((unsigned)min((int64_t)kBigBlocks, (n_faces + 3) / 4)),
                           dim3(kVT), 0, st, static_cast<const ViewVert *>(w.pv), faces, n_faces, n_verts, (int)H,
                           (int)W, bits + v * pixels, static_cast<const int32_t *>(w.list),
                           static_cast<const uint32_t *>(w.count));
    }
    HM_CHECK_LAUNCH("hm_mesh_depth_maps");
    return HM_OK;
}

int hm_mesh_visible_votes(const float *verts, int64_t n_verts, const double *proj, int64_t n_views, const float *depth,
                          int64_t H, int64_t W, int64_t pad, float tol, int accumulate, int32_t *n_visible,
                          void *stream) {
    if (int rc = hm_check_mesh(0, n_verts, nullptr, "hm_mesh_visible_votes")) return rc;
    if (int rc = hm_view_check_image(n_views, H, W, "hm_mesh_visible_votes")) return rc;
    HM_CHECK_ARG(pad >= 0 && pad <= 64, "hm_mesh_visible_votes: pad must be in [0, 64]");
    HM_CHECK_ARG(tol == tol, "hm_mesh_visible_votes: tol is NaN");
    if (n_verts == 0) return HM_OK;
    HM_CHECK_ARG(verts && n_visible && (n_views == 0 || (proj && depth)), "hm_mesh_visible_votes: NULL pointer");
    hipLaunchKernelGGL(cull_visible_votes_kernel, dim3(hm_grid(n_verts, kVT)), dim3(kVT), 0, as_stream(stream), verts,
                       n_verts, proj, (int)n_views, depth, (int)H, (int)W, (int)pad, tol, accumulate, n_visible);
    HM_CHECK_LAUNCH("hm_mesh_visible_votes");
    return HM_OK;
}

int hm_mesh_keep_mark(const int32_t *faces, int64_t n_faces, int64_t n_verts, const uint8_t *keep, int32_t *vflag,
                      int32_t *fflag, int32_t *status, void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_keep_mark")) return rc;
    if (n_faces == 0) return HM_OK;
    HM_CHECK_ARG(vflag && fflag && status && (n_verts == 0 || keep), "hm_mesh_keep_mark: NULL pointer");
    hipLaunchKernelGGL(cull_keep_mark_kernel, dim3(hm_grid(n_faces, kVT)), dim3(kVT), 0, as_stream(stream), faces,
                       n_faces, n_verts, keep, vflag, fflag, status);
    HM_CHECK_LAUNCH("hm_mesh_keep_mark");
    return HM_OK;
}

}  // extern "C"
