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
// colours': hm_mesh_color.hip).  Coverage is decided by int64 edge functions of the fixed-point positions (|X|, |Y| <
// 2^24 and pixel centres below 2^24: every product is below 2^50), the depth by fp64 operations rounded once, and a
// pixel keeps the minimum through an unsigned atomicMin on the float's bits (positive floats order like their bits): the
// depth maps do not depend on the order of the faces and two calls give the same bits.  The votes are written once per
// vertex, without atomics.  No index is dereferenced before its range check.
#include "hm_block_dev.h"
#include "hm_view_dev.h"

namespace {

constexpr int kVT = 256;
constexpr int kBigBlocks = 1024;          // workgroups of cull_raster_big: 4096 waves stride over the list
constexpr uint32_t kInfBits = 0x7f800000u;

// a vertex as one view sees it: 16 bytes, one load per face corner.  X == kBadX: the face is skipped
struct __align__(16) ViewVert {
    int32_t X, Y;
    double iw;
};
constexpr int32_t kBadX = INT32_MIN;

struct CullWs {
    ViewVert *pv;        // [n_verts]
    int32_t *list;       // [n_faces] the faces of the current view whose box exceeds big_face
    uint32_t *count;     // [1]
    int64_t bytes;
};

CullWs cull_layout(void *ws, int64_t n_verts, int64_t n_faces) {
    HmCarve c(ws);
    CullWs w;
    w.pv = c.take<ViewVert>(n_verts > 0 ? n_verts : 1);
    w.list = c.take<int32_t>(n_faces > 0 ? n_faces : 1);
    w.count = c.take<uint32_t>(1);
    w.bytes = c.bytes;
    return w;
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

__global__ __launch_bounds__(kVT) void cull_project_kernel(const float *__restrict__ verts, int64_t n_verts,
                                                           const double *__restrict__ P, ViewVert *__restrict__ pv,
                                                           uint32_t *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x;
    if (i == 0) *count = 0u;   // the list of the view before this one has been consumed: the stream orders the launches
    if (i >= n_verts) return;
    const HmViewPoint q = hm_view_project(P, verts[i * 3], verts[i * 3 + 1], verts[i * 3 + 2]);
    ViewVert o;
    if (!hm_view_fixed(q, o.X, o.Y)) o.X = kBadX;
    o.iw = __ddiv_rn(1.0, q.w);
    pv[i] = o;
}

// a face of one view, ready to be drawn: its corners, its doubled area and the pixels of its clamped bounding box
struct Tri {
    int64_t X[3], Y[3], area;
    double iw[3];
    int c0, c1, r0, r1;   // columns c0..c1 and rows r0..r1, inclusive
};

enum { kTriNone = 0, kTriDraw = 1, kTriSkipped = 2 };

// kTriSkipped: a corner is unprojectable or out of the fixed-point range; kTriNone: zero area or no pixel centre in the box
__device__ __forceinline__ int cull_tri(const ViewVert *__restrict__ pv, const int32_t (&id)[3], int H, int W, Tri &t) {
    bool ok = true;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const ViewVert q = pv[id[m]];
        ok = ok && q.X != kBadX;
        t.X[m] = q.X;
        t.Y[m] = q.Y;
        t.iw[m] = q.iw;
    }
    if (!ok) return kTriSkipped;
    t.area = (t.X[1] - t.X[0]) * (t.Y[2] - t.Y[0]) - (t.Y[1] - t.Y[0]) * (t.X[2] - t.X[0]);
    if (t.area == 0) return kTriNone;
    const int64_t xlo = min(t.X[0], min(t.X[1], t.X[2])), xhi = max(t.X[0], max(t.X[1], t.X[2]));
    const int64_t ylo = min(t.Y[0], min(t.Y[1], t.Y[2])), yhi = max(t.Y[0], max(t.Y[1], t.Y[2]));
    // the centres 256*col inside [xlo, xhi]: ceil and floor by arithmetic shifts (exact for negative values too)
    t.c0 = (int)max((xlo + (kViewSub - 1)) >> 8, (int64_t)0);
    t.c1 = (int)min(xhi >> 8, (int64_t)W - 1);
    t.r0 = (int)max((ylo + (kViewSub - 1)) >> 8, (int64_t)0);
    t.r1 = (int)min(yhi >> 8, (int64_t)H - 1);
    return (t.c0 <= t.c1 && t.r0 <= t.r1) ? kTriDraw : kTriNone;
}

// the pixel (col, row) of the box: covered iff E_0, E_1, E_2 are all >= 0 or all <= 0; then depth = min(depth, z)
__device__ __forceinline__ void cull_pixel(const Tri &t, int col, int row, int W, uint32_t *__restrict__ depth) {
    const int64_t Xp = (int64_t)col * kViewSub, Yp = (int64_t)row * kViewSub;
    int64_t E[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        E[a] = (t.X[c] - t.X[b]) * (Yp - t.Y[b]) - (t.Y[c] - t.Y[b]) * (Xp - t.X[b]);
    }
    const bool covered = (E[0] >= 0 && E[1] >= 0 && E[2] >= 0) || (E[0] <= 0 && E[1] <= 0 && E[2] <= 0);
    if (!covered) return;
    const double area = (double)t.area;
    const double b0 = __ddiv_rn((double)E[0], area), b1 = __ddiv_rn((double)E[1], area),
                 b2 = __ddiv_rn((double)E[2], area);
    const double s = __dadd_rn(__dadd_rn(__dmul_rn(b0, t.iw[0]), __dmul_rn(b1, t.iw[1])), __dmul_rn(b2, t.iw[2]));
    const float z = __double2float_rn(__ddiv_rn(1.0, s));
    if (isfinite(z) && z > 0.0f) atomicMin(depth + (int64_t)row * W + col, __float_as_uint(z));
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
