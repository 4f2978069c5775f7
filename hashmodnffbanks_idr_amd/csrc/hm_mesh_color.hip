// hm_mesh_color.hip - colouring the vertices of an extracted mesh from the photographs (contract: include/hashmod.h;
// driver: ops.mesh_vertex_colors, ops.mesh_colors_finish, evaluation/color.py):
//
//   hm_mesh_vertex_colors  one lane per vertex, a loop over the views in ascending order: is the vertex in the image,
//                          visible against the mesh's depth map (hm_view_visible, the rule of hm_mesh_visible_votes),
//                          inside the eroded mask (four reads of the masks' summed-area table) and facing the camera;
//                          then four image taps per channel, blended by cos^power or kept from the best view
//
// The projection, the pixel and the visibility rule are hm_view_dev.h's.  Every operation is fp64 and rounded once, the
// views are visited in order and a vertex belongs to one lane: no atomics, no workspace, two calls give the same bits,
// and a call over the views [0, n) equals calls over [0, k) and [k, n) with accumulate.  No index is formed before its
// range check: the taps come from floor(u), floor(v) of a vertex whose pixel rint(u), rint(v) is in the image, so they
// are in [-1, W - 1] x [-1, H - 1] before the clamp.
#include "hm_block_dev.h"
#include "hm_color_dev.h"
#include "hm_view_dev.h"

namespace {

constexpr int kVT = 256;
constexpr int kColorMaxPower = 8;

// MODE 0 blends the views by their weights, MODE 1 keeps the view of the largest weight (the first of equals)
template <int MODE, bool FACING, bool MASKED>
__global__ __launch_bounds__(kVT) void color_vertex_kernel(const float *__restrict__ verts,
                                                           const float *__restrict__ normals, int64_t n_verts,
                                                           const double *__restrict__ proj,
                                                           const double *__restrict__ centers, int n_views,
                                                           const float *__restrict__ images,
                                                           const float *__restrict__ depth,
                                                           const int32_t *__restrict__ sat, int H, int W, int pad,
                                                           float tol, int erode, double min_cos, int power,
                                                           int accumulate, double *__restrict__ acc,
                                                           int32_t *__restrict__ n_used) {
    const int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x;
    if (i >= n_verts) return;
    const float x = verts[i * 3], y = verts[i * 3 + 1], z = verts[i * 3 + 2];
    double nx = 0.0, ny = 0.0, nz = 0.0, nn = 0.0;
    if (FACING) {
        nx = normals[i * 3], ny = normals[i * 3 + 1], nz = normals[i * 3 + 2];
        nn = color_dot(nx, ny, nz, nx, ny, nz);
    }
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    int used = 0;
    if (accumulate) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = acc[i * 4 + k];
        used = n_used[i];
    }
    const int64_t pixels = (int64_t)H * W, pitch = (int64_t)W + 1, plane = ((int64_t)H + 1) * pitch;
    for (int v = 0; v < n_views; ++v) {
        const HmViewPoint q = hm_view_project(proj + (int64_t)v * 12, x, y, z);
        int32_t col, row;
        if (!hm_view_pixel(q, H, W, col, row)) continue;
        if (!hm_view_visible(q, depth + (int64_t)v * pixels, H, W, col, row, pad, tol)) continue;
        if (MASKED) {
            // every pixel of the clamped (2 erode + 1)^2 window is set: its count equals its area
            const int64_t c0 = max(col - erode, 0), c1 = min(col + erode, W - 1) + 1;
            const int64_t r0 = max(row - erode, 0), r1 = min(row + erode, H - 1) + 1;
            const int32_t *s = sat + (int64_t)v * plane;
            const int32_t set = (s[r1 * pitch + c1] - s[r0 * pitch + c1]) - (s[r1 * pitch + c0] - s[r0 * pitch + c0]);
            if ((int64_t)set != (c1 - c0) * (r1 - r0)) continue;
        }
        double w = 1.0;
        if (FACING) {
            const double *c = centers + (int64_t)v * 3;
            const double dx = __dsub_rn(c[0], (double)x), dy = __dsub_rn(c[1], (double)y),
                         dz = __dsub_rn(c[2], (double)z);
            const double den = __dsqrt_rn(__dmul_rn(nn, color_dot(dx, dy, dz, dx, dy, dz)));
            const double cs = __ddiv_rn(color_dot(nx, ny, nz, dx, dy, dz), den);
            if (!(den > 0.0 && isfinite(cs) && cs > min_cos)) continue;
            for (int p = 0; p < power; ++p) w = __dmul_rn(w, cs);
        }
        // the pixel is in the image: floor(u) in [-1, W - 1], floor(v) in [-1, H - 1]
        const double fc = floor(q.u), fr = floor(q.v);
        const double fu = __dsub_rn(q.u, fc), fv = __dsub_rn(q.v, fr);
        const int ic = (int)fc, ir = (int)fr;
        const int64_t ca = min(max(ic, 0), W - 1), cb = min(max(ic + 1, 0), W - 1);
        const int64_t ra = min(max(ir, 0), H - 1), rb = min(max(ir + 1, 0), H - 1);
        const float *img = images + (int64_t)v * pixels * 3;
        const float *taa = img + (ra * W + ca) * 3, *tab = img + (ra * W + cb) * 3;
        const float *tba = img + (rb * W + ca) * 3, *tbb = img + (rb * W + cb) * 3;
        double val[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            val[k] = color_lerp(color_lerp((double)taa[k], (double)tab[k], fu),
                                color_lerp((double)tba[k], (double)tbb[k], fu), fv);
        ++used;
        if (MODE == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a[k] = __dadd_rn(a[k], __dmul_rn(w, val[k]));
            a[3] = __dadd_rn(a[3], w);
        } else if (w > a[3]) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a[k] = val[k];
            a[3] = w;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[i * 4 + k] = a[k];
    n_used[i] = used;
}

}  // namespace

extern "C" {

int hm_mesh_vertex_colors(const float *verts, const float *normals, int64_t n_verts, const double *proj,
                          const double *centers, const float *images, const float *depth, const int32_t *sat,
                          int64_t n_views, int64_t H, int64_t W, int64_t pad, float tol, int64_t erode, double min_cos,
                          int power, int mode, int accumulate, double *acc, int32_t *n_used, void *stream) {
    if (int rc = hm_check_mesh(0, n_verts, nullptr, "hm_mesh_vertex_colors")) return rc;
    if (int rc = hm_view_check_image(n_views, H, W, "hm_mesh_vertex_colors")) return rc;
    HM_CHECK_ARG(pad >= 0 && pad <= 64, "hm_mesh_vertex_colors: pad must be in [0, 64]");
    HM_CHECK_ARG(erode >= 0 && erode <= 65536, "hm_mesh_vertex_colors: erode must be in [0, 65536]");
    HM_CHECK_ARG(tol == tol, "hm_mesh_vertex_colors: tol is NaN");
    HM_CHECK_ARG(min_cos >= 0.0 && min_cos < 1.0, "hm_mesh_vertex_colors: min_cos must be in [0, 1)");
    HM_CHECK_ARG(power >= 0 && power <= kColorMaxPower, "hm_mesh_vertex_colors: power must be in [0, 8]");
    HM_CHECK_ARG(mode == 0 || mode == 1, "hm_mesh_vertex_colors: mode must be 0 (blend) or 1 (best)");
    if (n_verts == 0) return HM_OK;
    HM_CHECK_ARG(verts && acc && n_used && (n_views == 0 || (proj && centers && images && depth)),
                 "hm_mesh_vertex_colors: NULL pointer");
    if (n_views == 0 && accumulate) return HM_OK;   // nothing to add; without accumulate the launch writes the zeros
    hm_bool_dispatch(mode == 1, [&](auto best) {
        hm_bool_dispatch(normals != nullptr, [&](auto facing) {
            hm_bool_dispatch(sat != nullptr, [&](auto masked) {
                hipLaunchKernelGGL((color_vertex_kernel<best.value ? 1 : 0, facing.value, masked.value>),
                                   dim3(hm_grid(n_verts, kVT)), dim3(kVT), 0, as_stream(stream), verts, normals,
                                   n_verts, proj, centers, (int)n_views, images, depth, sat, (int)H, (int)W, (int)pad,
                                   tol, (int)erode, min_cos, power, accumulate, acc, n_used);
            });
        });
    });
    HM_CHECK_LAUNCH("hm_mesh_vertex_colors");
    return HM_OK;
}

}  // extern "C"
