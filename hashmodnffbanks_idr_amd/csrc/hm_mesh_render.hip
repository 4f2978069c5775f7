// hm_mesh_render.hip - an extracted mesh seen through the cameras: a visibility buffer and its resolve (contract:
// include/hashmod.h; driver: ops.mesh_render, evaluation/mesh_views.py).  Per view, on the caller's stream:
//
//   cull_project         one lane per vertex: fixed-point position and 1/w into the workspace (hm_raster_dev.h)
//   render_fill          one 64-bit key per pixel, all ones
//   render_raster        one lane per face: the pixel centres of its bounding box; a box of more than big_face pixels
//                        goes to a list.  A covered pixel with a depth z that is finite and > 0 takes
//                        key = min(key, float_bits(z) << 32 | face) by a 64-bit unsigned atomicMin whose result is
//                        not used (global_atomic_umin_x2 without a return on gfx950)
//   render_raster_big    one wave per listed face
//   render_resolve       one lane per pixel: the face and the depth out of the key, the perspective-correct weights and
//                        the interpolated attributes recomputed from the face's projected corners; no atomics
//
// Coverage and depth are the depth maps' (hm_raster_dev.h: the same functions), so `depth` has hm_mesh_depth_maps' bits.
// Positive floats order like their bits and the face sits in the low word: a pixel keeps the nearest sample and, among
// equal depths, the smallest face index, whatever the order in which the faces are drawn.  No face or vertex index is
// dereferenced before its range check.
#include "hm_raster_dev.h"

namespace {

constexpr int kMaxAttr = 16;
constexpr unsigned long long kNoKey = ~0ull;

struct RenderWs {
    CullWs cull;
    unsigned long long *keys;   // [H * W] of the current view
    int64_t bytes;
};

RenderWs render_layout(void *ws, int64_t n_verts, int64_t n_faces, int64_t pixels) {
    HmCarve c(ws);
    RenderWs w;
    w.cull = cull_layout(c, n_verts, n_faces);
    w.keys = c.take<unsigned long long>(pixels);
    w.bytes = c.bytes;
    return w;
}

struct Background {
    float v[kMaxAttr];
};

__global__ __launch_bounds__(kRasterVT) void render_fill_kernel(unsigned long long *__restrict__ keys, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kRasterVT + threadIdx.x;
    if (i < n) keys[i] = kNoKey;
}

__device__ __forceinline__ void render_pixel(const Tri &t, int64_t f, int col, int row, int W,
                                             unsigned long long *__restrict__ keys) {
    raster_pixel(t, col, row, [&](float z) {
        atomicMin(keys + (int64_t)row * W + col, ((unsigned long long)__float_as_uint(z) << 32) | (uint32_t)f);
    });
}

__global__ __launch_bounds__(kRasterVT) void render_raster_kernel(const ViewVert *__restrict__ pv,
                                                                  const int32_t *__restrict__ faces, int64_t n_faces,
                                                                  int64_t n_verts, int H, int W, int64_t big_face,
                                                                  unsigned long long *__restrict__ keys,
                                                                  int32_t *__restrict__ n_skipped,
                                                                  int32_t *__restrict__ list,
                                                                  uint32_t *__restrict__ count, int32_t *status) {
    const int64_t f = (int64_t)blockIdx.x * kRasterVT + threadIdx.x;
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
        for (int col = t.c0; col <= t.c1; ++col) render_pixel(t, f, col, row, W, keys);
}

// one wave per listed face, 64 pixels of its box per round (H*W < 2^31: the box fits uint32)
__global__ __launch_bounds__(kRasterVT) void render_raster_big_kernel(const ViewVert *__restrict__ pv,
                                                                      const int32_t *__restrict__ faces,
                                                                      int64_t n_faces, int64_t n_verts, int H, int W,
                                                                      unsigned long long *__restrict__ keys,
                                                                      const int32_t *__restrict__ list,
                                                                      const uint32_t *__restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * kRasterVT + threadIdx.x) >> 6,
                  n_waves = (int64_t)gridDim.x * (kRasterVT / 64);
    const int64_t n = min((int64_t)*count, n_faces);
    for (int64_t i = wave; i < n; i += n_waves) {
        const int64_t f = list[i];
        int32_t id[3];
        if (f < 0 || f >= n_faces || !hm_face_ids(faces, f, n_verts, id)) continue;
        Tri t;
        if (cull_tri(pv, id, H, W, t) != kTriDraw) continue;
        const uint32_t bw = (uint32_t)(t.c1 - t.c0 + 1), total = bw * (uint32_t)(t.r1 - t.r0 + 1);
        for (uint32_t p = lane; p < total; p += 64)
            render_pixel(t, f, t.c0 + (int)(p % bw), t.r0 + (int)(p / bw), W, keys);
    }
}

// One lane per pixel.  The key's face is one that covered this pixel in the raster of this view, so its indices are in
// range and cull_tri draws it; both are tested again all the same, and a key that fails them resolves to "nothing drawn".
__global__ __launch_bounds__(kRasterVT) void render_resolve_kernel(const unsigned long long *__restrict__ keys,
                                                                   const ViewVert *__restrict__ pv,
                                                                   const int32_t *__restrict__ faces, int64_t n_faces,
                                                                   int64_t n_verts, int H, int W,
                                                                   const float *__restrict__ attrs, int n_attr,
                                                                   Background bg, int32_t *__restrict__ face_id,
                                                                   float *__restrict__ depth,
                                                                   float *__restrict__ weights,
                                                                   float *__restrict__ image) {
    const int64_t p = (int64_t)blockIdx.x * kRasterVT + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const unsigned long long key = keys[p];
    const int64_t f = (int64_t)(key & 0xffffffffull);
    int32_t id[3];
    Tri t;
    const bool drawn = key != kNoKey && f < n_faces && hm_face_ids(faces, f, n_verts, id) &&
                       cull_tri(pv, id, H, W, t) == kTriDraw;
    if (!drawn) {
        face_id[p] = -1;
        depth[p] = __uint_as_float(0x7f800000u);
        if (weights) weights[p * 3] = weights[p * 3 + 1] = weights[p * 3 + 2] = 0.0f;
        for (int c = 0; c < n_attr; ++c) image[p * n_attr + c] = bg.v[c];
        return;
    }
    face_id[p] = (int32_t)f;
    depth[p] = __uint_as_float((uint32_t)(key >> 32));
    if (!weights && n_attr == 0) return;
    int64_t E[3];
    raster_edges(t, (int)(p % W), (int)(p / W), E);
    const RasterTerms r = raster_terms(t, E);
    if (weights) {
        weights[p * 3] = __double2float_rn(__ddiv_rn(r.t0, r.s));
        weights[p * 3 + 1] = __double2float_rn(__ddiv_rn(r.t1, r.s));
        weights[p * 3 + 2] = __double2float_rn(__ddiv_rn(r.t2, r.s));
    }
    const float *a0 = attrs + (int64_t)id[0] * n_attr, *a1 = attrs + (int64_t)id[1] * n_attr,
                *a2 = attrs + (int64_t)id[2] * n_attr;
    for (int c = 0; c < n_attr; ++c) {
        const double num = __dadd_rn(__dadd_rn(__dmul_rn(r.t0, (double)a0[c]), __dmul_rn(r.t1, (double)a1[c])),
                                     __dmul_rn(r.t2, (double)a2[c]));
        image[p * n_attr + c] = __double2float_rn(__ddiv_rn(num, r.s));
    }
}

}  // namespace

extern "C" {

int64_t hm_mesh_render_workspace_bytes(int64_t n_verts, int64_t n_faces, int64_t H, int64_t W) {
    if (n_verts < 0 || n_verts >= ((int64_t)1 << 31) || n_faces < 0 || n_faces >= ((int64_t)1 << 31))
        return hm_fail(HM_ERR_INVALID, "hm_mesh_render_workspace_bytes: n_verts and n_faces must be in [0, 2^31)");
    if (int rc = hm_view_check_image(0, H, W, "hm_mesh_render_workspace_bytes")) return rc;
    return render_layout(nullptr, n_verts, n_faces, H * W).bytes;
}

int hm_mesh_render(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const double *proj,
                   int64_t n_views, int64_t H, int64_t W, int64_t big_face, const float *attrs, int64_t n_attr,
                   const float *background, int32_t *face_id, float *depth, float *weights, float *image,
                   int32_t *n_skipped, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_render")) return rc;
    if (int rc = hm_view_check_image(n_views, H, W, "hm_mesh_render")) return rc;
    HM_CHECK_ARG(big_face >= 1, "hm_mesh_render: big_face must be >= 1");
    HM_CHECK_ARG(n_attr >= 0 && n_attr <= kMaxAttr, "hm_mesh_render: n_attr must be in [0, 16]");
    HM_CHECK_ARG((attrs != nullptr) == (image != nullptr), "hm_mesh_render: attrs and image go together");
    HM_CHECK_ARG(n_attr == 0 || attrs, "hm_mesh_render: NULL attrs with n_attr > 0");
    if (n_views == 0) return HM_OK;
    HM_CHECK_ARG(proj && face_id && depth && n_skipped && status && workspace && (n_verts == 0 || verts),
                 "hm_mesh_render: NULL pointer");
    HM_CHECK_ARG(workspace_bytes >= render_layout(nullptr, n_verts, n_faces, H * W).bytes,
                 "hm_mesh_render: workspace too small");
    Background bg;
    for (int c = 0; c < kMaxAttr; ++c) bg.v[c] = (background && c < n_attr) ? background[c] : 0.0f;
    const int n_image = image ? (int)n_attr : 0;
    const RenderWs w = render_layout(workspace, n_verts, n_faces, H * W);
    hipStream_t st = as_stream(stream);
    const int64_t pixels = H * W;
    hm_zero_u32_async(n_skipped, n_views, st);
    for (int64_t v = 0; v < n_views; ++v) {
        hipLaunchKernelGGL(render_fill_kernel, dim3(hm_grid(pixels, kRasterVT)), dim3(kRasterVT), 0, st, w.keys, pixels);
        if (n_faces > 0) {
            hipLaunchKernelGGL(cull_project_kernel, dim3(hm_grid(n_verts > 0 ? n_verts : 1, kRasterVT)),
                               dim3(kRasterVT), 0, st, verts, n_verts, proj + v * 12, w.cull.pv, w.cull.count);
            hipLaunchKernelGGL(render_raster_kernel, dim3(hm_grid(n_faces, kRasterVT)), dim3(kRasterVT), 0, st,
                               static_cast<const ViewVert *>(w.cull.pv), faces, n_faces, n_verts, (int)H, (int)W,
                               big_face, w.keys, n_skipped + v, w.cull.list, w.cull.count, status);
            hipLaunchKernelGGL(render_raster_big_kernel,
                               dim3((unsigned)min((int64_t)kRasterBigBlocks, (n_faces + 3) / 4)), dim3(kRasterVT), 0,
                               st, static_cast<const ViewVert *>(w.cull.pv), faces, n_faces, n_verts, (int)H, (int)W,
                               w.keys, static_cast<const int32_t *>(w.cull.list),
                               static_cast<const uint32_t *>(w.cull.count));
        }
        hipLaunchKernelGGL(render_resolve_kernel, dim3(hm_grid(pixels, kRasterVT)), dim3(kRasterVT), 0, st,
                           static_cast<const unsigned long long *>(w.keys), static_cast<const ViewVert *>(w.cull.pv),
                           faces, n_faces, n_verts, (int)H, (int)W, attrs, n_image, bg, face_id + v * pixels,
                           depth + v * pixels, weights ? weights + v * pixels * 3 : nullptr,
                           image ? image + v * pixels * n_image : nullptr);
    }
    HM_CHECK_LAUNCH("hm_mesh_render");
    return HM_OK;
}

}  // extern "C"
