// hm_view_dev.h - a vertex seen by a view, written once for the culling and colouring kernels (hm_mesh_cull.hip,
// hm_mesh_color.hip): the projection, the pixel, the fixed-point screen position and the visibility rule.  A view is a
// 3x4 projection P in fp64 (K[:3,:3] @ inv(pose)[:3,:4]); pixel (col, row) has its centre at uv = (col, row).  Every
// operation is fp64 on the fp32 coordinates and rounded once (__dmul_rn and friends: no contraction whatever the build
// flags say), so the numpy restatement (tests/mesh_cull_cases.py) gives the same bits.  Every range test is made on
// doubles BEFORE a value becomes an integer: a NaN, an infinity or a huge value fails it and nothing is read.
#pragma once
#include <math.h>

#include "hm_common.h"

constexpr int kViewSub = 256;                  // fixed-point units per pixel
constexpr double kViewFixedLimit = 16777216.0; // |X|, |Y| < 2^24

#ifdef __HIPCC__
struct HmViewPoint {
    double u, v, w;   // u = p0/w, v = p1/w, w = p2; meaningful only when ok
    bool ok;          // projectable: finite coordinates, w finite and > 0
};

// p_a = ((P[a,0]*x + P[a,1]*y) + P[a,2]*z) + P[a,3]; P: 12 doubles, row-major
__device__ __forceinline__ HmViewPoint hm_view_project(const double *__restrict__ P, float fx, float fy, float fz) {
    HmViewPoint q;
    const double x = fx, y = fy, z = fz;
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        p[a] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(P[a * 4], x), __dmul_rn(P[a * 4 + 1], y)),
                                   __dmul_rn(P[a * 4 + 2], z)), P[a * 4 + 3]);
    q.w = p[2];
    q.ok = isfinite(fx) && isfinite(fy) && isfinite(fz) && isfinite(q.w) && q.w > 0.0;
    q.u = __ddiv_rn(p[0], q.w);
    q.v = __ddiv_rn(p[1], q.w);
    return q;
}

// the pixel (col, row) = (rint(u), rint(v)), half to even; false unless the vertex is projectable and in the W x H image
__device__ __forceinline__ bool hm_view_pixel(const HmViewPoint &q, int64_t H, int64_t W, int32_t &col, int32_t &row) {
    const double c = rint(q.u), r = rint(q.v);
    const bool in = q.ok && c >= 0.0 && c < (double)W && r >= 0.0 && r < (double)H;
    col = in ? (int32_t)c : 0;
    row = in ? (int32_t)r : 0;
    return in;
}

// the fixed-point position (X, Y) = (rint(256 u), rint(256 v)); false unless projectable and |X|, |Y| < 2^24
__device__ __forceinline__ bool hm_view_fixed(const HmViewPoint &q, int32_t &X, int32_t &Y) {
    const double x = rint(__dmul_rn(q.u, (double)kViewSub)), y = rint(__dmul_rn(q.v, (double)kViewSub));
    const bool in = q.ok && fabs(x) < kViewFixedLimit && fabs(y) < kViewFixedLimit;
    X = in ? (int32_t)x : 0;
    Y = in ? (int32_t)y : 0;
    return in;
}

// the visibility rule of the votes and of the colours: float32(w) <= m + tol, m = the maximum of the view's depth map d
// [H, W] over the (2 pad + 1)^2 pixels around the vertex' pixel (col, row), indices clamped to the image.  (col, row)
// is hm_view_pixel's and in the image.
__device__ __forceinline__ bool hm_view_visible(const HmViewPoint &q, const float *__restrict__ d, int H, int W,
                                                int32_t col, int32_t row, int pad, float tol) {
    float m = d[(int64_t)row * W + col];
    for (int dr = -pad; dr <= pad; ++dr) {
        const int64_t r = min(max(row + dr, 0), H - 1);
        for (int dc = -pad; dc <= pad; ++dc) m = fmaxf(m, d[r * W + min(max(col + dc, 0), W - 1)]);
    }
    return __double2float_rn(q.w) <= __fadd_rn(m, tol);
}
#endif

// the image sizes the kernels' index arithmetic is written for: pixel centres below 2^24, H*W within int32
inline int hm_view_check_image(int64_t n_views, int64_t H, int64_t W, const char *what) {
    const std::string w(what);
    HM_CHECK_ARG(n_views >= 0 && n_views < ((int64_t)1 << 31), w + ": n_views must be in [0, 2^31)");
    HM_CHECK_ARG(H >= 1 && W >= 1 && H <= 65536 && W <= 65536 && H * W < ((int64_t)1 << 31),
                 w + ": H and W must be in [1, 65536] with H*W < 2^31");
    return HM_OK;
}
