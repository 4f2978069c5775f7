// hm_raster_dev.h - a face drawn into one view, written once for the depth maps (hm_mesh_cull.hip) and the renderer
// (hm_mesh_render.hip): the per-view vertex buffer and its projection kernel, the workspace the two share, the face
// set-up, the three edge functions with the coverage test, the barycentric weights and the depth of a covered pixel.
// Coverage is decided by int64 edge functions of the fixed-point positions (|X|, |Y| < 2^24 and pixel centres below
// 2^24: every product is below 2^50), the weights and the depth by fp64 operations rounded once (__ddiv_rn and
// friends), so the numpy restatements (tests/mesh_cull_cases.py, tests/mesh_render_cases.py) give the same bits.
// Everything here sits in an unnamed namespace: each translation unit gets its own copy of the kernel.
#pragma once
#include "hm_block_dev.h"
#include "hm_view_dev.h"

namespace {

constexpr int kRasterVT = 256;            // lanes per workgroup of the projection and raster kernels
constexpr int kRasterBigBlocks = 1024;    // workgroups of the wave-per-face kernels: 4096 waves stride over the list

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

// the parts the depth maps and the renderer share, in this order at the start of either workspace
inline CullWs cull_layout(HmCarve &c, int64_t n_verts, int64_t n_faces) {
    CullWs w;
    w.pv = c.take<ViewVert>(n_verts > 0 ? n_verts : 1);
    w.list = c.take<int32_t>(n_faces > 0 ? n_faces : 1);
    w.count = c.take<uint32_t>(1);
    w.bytes = c.bytes;
    return w;
}

#ifdef __HIPCC__
__global__ __launch_bounds__(kRasterVT) void cull_project_kernel(const float *__restrict__ verts, int64_t n_verts,
                                                                 const double *__restrict__ P,
                                                                 ViewVert *__restrict__ pv,
                                                                 uint32_t *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * kRasterVT + threadIdx.x;
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

// the edge functions E_0, E_1, E_2 of the pixel centre (col, row)
__device__ __forceinline__ void raster_edges(const Tri &t, int col, int row, int64_t (&E)[3]) {
    const int64_t Xp = (int64_t)col * kViewSub, Yp = (int64_t)row * kViewSub;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        E[a] = (t.X[c] - t.X[b]) * (Yp - t.Y[b]) - (t.Y[c] - t.Y[b]) * (Xp - t.X[b]);
    }
}

// t_m = b_m * iw_m with b_m = E_m / area, and s = (t_0 + t_1) + t_2: the depth is 1/s, an attribute sum(t_m a_m) / s.
// The statements keep the order of the nested expression the depth maps had, (b0*iw0 + b1*iw1) + b2*iw2: with it their
// kernels' instruction streams are what they were before this header (scripts/kernel_isa_diff.py).
struct RasterTerms {
    double t0, t1, t2, s;
};
__device__ __forceinline__ RasterTerms raster_terms(const Tri &t, const int64_t (&E)[3]) {
    const double area = (double)t.area;
    const double b0 = __ddiv_rn((double)E[0], area), b1 = __ddiv_rn((double)E[1], area),
                 b2 = __ddiv_rn((double)E[2], area);
    RasterTerms r;
    r.t0 = __dmul_rn(b0, t.iw[0]);
    r.t1 = __dmul_rn(b1, t.iw[1]);
    const double s01 = __dadd_rn(r.t0, r.t1);
    r.t2 = __dmul_rn(b2, t.iw[2]);
    r.s = __dadd_rn(s01, r.t2);
    return r;
}

// the depth of a covered pixel, z = float32(1 / ((b0*iw0 + b1*iw1) + b2*iw2))
__device__ __forceinline__ float raster_depth(const Tri &t, const int64_t (&E)[3]) {
    return __double2float_rn(__ddiv_rn(1.0, raster_terms(t, E).s));
}

// the sample of face t at the pixel centre (col, row): covered iff E_0, E_1, E_2 are all >= 0 or all <= 0 (both windings,
// inclusive edges); sink(z) iff it is covered and z is finite and > 0.  (The test is written out here, not in a function
// of its own: as one the compiler lowers its branches differently and the depth maps take 1 to 6 % longer.)
template <class Sink>
__device__ __forceinline__ void raster_pixel(const Tri &t, int col, int row, Sink sink) {
    int64_t E[3];
    raster_edges(t, col, row, E);
    const bool covered = (E[0] >= 0 && E[1] >= 0 && E[2] >= 0) || (E[0] <= 0 && E[1] <= 0 && E[2] <= 0);
    if (!covered) return;
    const float z = raster_depth(t, E);
    if (isfinite(z) && z > 0.0f) sink(z);
}
#endif

}  // namespace
