// hm_mesh_ray.hip - the first hit of a ray on a triangle mesh, exact in fp32, over the triangle grid that
// hm_mesh_dist.hip builds (contract and the definition of the per-face value: include/hashmod.h; DESIGN.md "Rays
// against the mesh on the device"; numpy restatement: tests/mesh_ray_cases.ray_ref, and walk_ref for the walk below).
//
//   hm_mesh_ray_cast  mr_cast   one ray per lane, 64 rays per workgroup, in the order given: the big-face run staged
//                               through LDS and tested by every lane (as md_query does), then every lane walks the
//                               slabs of the grid along its own ray and tests the records of the cells it crosses,
//                               read from global memory as three float4 each
//
// The result of a ray is the argmin over a superset of the faces that can hold its first hit, under the total order
// (t, face); a face tested twice changes nothing.  So it does not depend on the grid, big_face, the batch or the lane.
//
// WHY THE WALK IS EXACT.  A hit of the definition has its point p = fl(o + fl(t*d)) inside the face's padded box
// [lo, hi] = [fl(min - pad), fl(max + pad)] on every axis.  The index lists a face in every cell of nn_cell(lo) ..
// nn_cell(hi) (or the face is big and was tested up front), and nn_cell is monotone, so the face is listed in the
// cell of its own hit point.  For a fixed ray P_a(t) = fl(o_a + fl(t*d_a)) is monotone in t on every axis (a product
// and a sum with one fixed operand, each rounded once), and p = P(t) by definition - no error analysis is needed.
// Let m be the axis of the largest |d| and s the sign of d_m; c(t) = nn_cell(P_m(t)) is monotone along the ray.  The
// hits with t in [t_min, T], T = min(t_max, FLT_MAX), have c(t) between k0 = c(t_min) and k1 = c(T); the slabs
// k0, k0 + s, .., k1 are visited in that order.  For a slab k, mr_checked returns a time whose slab has been CHECKED
// to lie strictly before k (or strictly after k) in ray order - the crossing time of the slab's plane, nudged by
// doubling steps; by monotonicity every hit whose point lies in slab k has its t between the two, and its cell on
// a minor axis lies between the cells of P_a at the two ends.  Every record of that rectangle of cells is tested.
// Where no checked time is found the end of the ray's own range stands in: a larger rectangle, never a smaller one.
// After slab k every untested hit lies in a later slab, so its t exceeds T_before(k + s): a lane whose best t is <=
// that bound is finished - a later hit can neither beat nor tie it.  nn_cell clamps at the grid's border, so the
// border slabs stand for everything beyond them and origins and hits outside the grid need nothing more.
#include <float.h>
#include <math.h>

#include "hm_block_dev.h"
#include "hm_mesh_rec_dev.h"
#include "hm_nn_dev.h"

namespace {

constexpr int kBigChunk = 256;   // big-face records staged in LDS per pass (12 KiB)

struct MrBest {
    float t;
    int32_t face;
    float u, v;
    MdVec p;
};

// the value of face (a, b, c) for the ray, merged into B under the total order (t, face)
__device__ __forceinline__ void mr_test(MdVec o, MdVec d, float t_min, float t_max, float pad, MdVec a, MdVec b,
                                        MdVec c, int32_t face, MrBest &B) {
    const MdVec e1 = md_sub(b, a), e2 = md_sub(c, a);
    const MdVec pv = md_cross(d, e2);
    const float det = md_dot(e1, pv);
    const MdVec tv = md_sub(o, a);
    const float u = __fdiv_rn(md_dot(tv, pv), det);
    const MdVec qv = md_cross(tv, e1);
    const float v = __fdiv_rn(md_dot(d, qv), det);
    const float t = __fdiv_rn(md_dot(e2, qv), det);
    // a NaN fails every comparison; a t beyond the lane's best cannot win, whatever its point
    if (!(det != 0.0f && u >= 0.0f && v >= 0.0f && __fadd_rn(u, v) <= 1.0f && t >= t_min && t <= t_max && t <= B.t))
        return;
    const MdVec p = md_along(o, t, d);
    const MdVec lo = {__fsub_rn(fminf(fminf(a.x, b.x), c.x), pad), __fsub_rn(fminf(fminf(a.y, b.y), c.y), pad),
                      __fsub_rn(fminf(fminf(a.z, b.z), c.z), pad)};
    const MdVec hi = {__fadd_rn(fmaxf(fmaxf(a.x, b.x), c.x), pad), __fadd_rn(fmaxf(fmaxf(a.y, b.y), c.y), pad),
                      __fadd_rn(fmaxf(fmaxf(a.z, b.z), c.z), pad)};
    const bool inside = p.x >= lo.x && p.x <= hi.x && p.y >= lo.y && p.y <= hi.y && p.z >= lo.z && p.z <= hi.z;
    const bool better = inside && (t < B.t || face < B.face);   // t <= B.t holds here
    B.t = better ? t : B.t;
    B.face = better ? face : B.face;
    B.u = better ? u : B.u;
    B.v = better ? v : B.v;
    B.p.x = better ? p.x : B.p.x;
    B.p.y = better ? p.y : B.p.y;
    B.p.z = better ? p.z : B.p.z;
}

__device__ __forceinline__ void mr_test_record(const float4 r0, const float4 r1, const float4 r2, MdVec o, MdVec d,
                                               float t_min, float t_max, float pad, MrBest &B) {
    mr_test(o, d, t_min, t_max, pad, {r0.x, r0.y, r0.z}, {r0.w, r1.x, r1.y}, {r1.z, r1.w, r2.x}, __float_as_int(r2.y),
            B);
}

// P_a(t) = fl(o_a + fl(t * d_a))
__device__ __forceinline__ float mr_at(float o, float t, float d) { return __fadd_rn(o, __fmul_rn(t, d)); }

// A time whose major-axis cell has been CHECKED to lie strictly before (w = -1) or strictly after (w = +1) slab k in
// ray order; false when none was found.  The guess is the crossing time of the slab's entry (exit) plane, moved
// earlier (later) by doubling steps that start at a few ulp of the operands.
__device__ __forceinline__ bool mr_checked(float om, float dm, float lom, float h, int32_t gm, int32_t s, int32_t w,
                                           int32_t k, float &t) {
    const float plane = __fadd_rn(lom, __fmul_rn((float)(s * w > 0 ? k + 1 : k), h));
    float tg = __fdiv_rn(__fsub_rn(plane, om), dm);
    float step = __fmul_rn(__fadd_rn(__fdiv_rn(fmaxf(fmaxf(fabsf(om), fabsf(plane)), fmaxf(fabsf(lom), h)), fabsf(dm)),
                                     fabsf(tg)),
                           4.7683716e-7f);   // 2^-21
    for (int it = 0; it < 48; ++it) {
        tg = __fadd_rn(tg, w > 0 ? step : -step);
        if (tg == tg && w * s * (nn_cell(mr_at(om, tg, dm), lom, h, gm) - k) > 0) {
            t = tg;
            return true;
        }
        step = __fmul_rn(step, 2.0f);
    }
    return false;
}

__global__ __launch_bounds__(64) void mr_cast_kernel(const float *__restrict__ origins, const float *__restrict__ dirs,
                                                     const float *__restrict__ t_min_in,
                                                     const float *__restrict__ t_max_in, int64_t m,
                                                     const float4 *__restrict__ rec, int64_t n_pairs, int64_t n_big,
                                                     const int32_t *__restrict__ cell_start, NnGrid G, float pad,
                                                     float *__restrict__ t_out, int32_t *__restrict__ face_out,
                                                     float *__restrict__ uv_out, float *__restrict__ point_out,
                                                     int32_t *status, unsigned long long *n_tests) {
    __shared__ float4 stage[kBigChunk * kRecVec];
    const int lane = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * 64;
    const bool live = first + lane < m;
    const int64_t i = live ? first + lane : first;   // first < m: the launch has ceil(m / 64) workgroups
    const MdVec o = {origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2]};
    const MdVec d = {dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]};
    const float t_min = t_min_in ? t_min_in[i] : 0.0f;
    const float t_max = t_max_in ? t_max_in[i] : INFINITY;
    const bool finite = nn_finite3(o.x, o.y, o.z) && nn_finite3(d.x, d.y, d.z) && isfinite(t_min) && t_max == t_max;
    if (live && !finite) atomicOr(status, 4);

    MrBest B = {INFINITY, kNoFace, NAN, NAN, {NAN, NAN, NAN}};
    unsigned long long tests = 0;

    // the big faces: one run behind the pair records, staged in LDS and tested in full by every lane
    for (int64_t t0 = 0; t0 < n_big; t0 += kBigChunk) {
        const int32_t cnt = (int32_t)min((int64_t)kBigChunk, n_big - t0);
#pragma unroll
        for (int u = 0; u < kBigChunk / 64; ++u) {
            const int32_t slot = u * 64 + lane;
            if (slot < cnt) {
#pragma unroll
                for (int k = 0; k < kRecVec; ++k) stage[slot * kRecVec + k] = rec[(n_pairs + t0 + slot) * kRecVec + k];
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int32_t c = 0; c < cnt; ++c)
            mr_test_record(stage[c * kRecVec], stage[c * kRecVec + 1], stage[c * kRecVec + 2], o, d, t_min, t_max, pad,
                           B);
        __syncthreads();
        tests += live ? (unsigned long long)cnt : 0ull;
    }

    // the slab walk of this lane's ray; T is finite: a hit has a finite t, and inf * 0 must not enter the walk
    const float T = fminf(t_max, FLT_MAX);
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    const int32_t maj = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);   // the lowest axis among equal
    const float om = maj == 0 ? o.x : maj == 1 ? o.y : o.z;
    const float dm = maj == 0 ? d.x : maj == 1 ? d.y : d.z;
    const float lom = maj == 0 ? G.lo[0] : maj == 1 ? G.lo[1] : G.lo[2];
    const int32_t gm = maj == 0 ? G.g[0] : maj == 1 ? G.g[1] : G.g[2];
    const int32_t gx = G.g[0], gy = G.g[1], gz = G.g[2];
    if (live && finite && dm != 0.0f && t_min <= T) {
        const int32_t s = dm > 0.0f ? 1 : -1;
        int32_t k = nn_cell(mr_at(om, t_min, dm), lom, G.h, gm);
        const int32_t k1 = nn_cell(mr_at(om, T, dm), lom, G.h, gm);
        float t_lo = t_min;   // no hit whose point lies in slab k has a smaller t
        for (int32_t n = 0; n < gm; ++n) {
            float t_hi = fminf(T, B.t);   // a hit beyond the lane's best neither beats nor ties it
            if (k != k1) {
                float ta;
                if (mr_checked(om, dm, lom, G.h, gm, s, 1, k, ta)) t_hi = fminf(t_hi, ta);
            }
            if (t_lo <= t_hi) {
                const int32_t xa = nn_cell(mr_at(o.x, t_lo, d.x), G.lo[0], G.h, gx),
                              xb = nn_cell(mr_at(o.x, t_hi, d.x), G.lo[0], G.h, gx);
                const int32_t ya = nn_cell(mr_at(o.y, t_lo, d.y), G.lo[1], G.h, gy),
                              yb = nn_cell(mr_at(o.y, t_hi, d.y), G.lo[1], G.h, gy);
                const int32_t za = nn_cell(mr_at(o.z, t_lo, d.z), G.lo[2], G.h, gz),
                              zb = nn_cell(mr_at(o.z, t_hi, d.z), G.lo[2], G.h, gz);
                const int32_t x0 = maj == 0 ? k : min(xa, xb), x1 = maj == 0 ? k : max(xa, xb);
                const int32_t y0 = maj == 1 ? k : min(ya, yb), y1 = maj == 1 ? k : max(ya, yb);
                const int32_t z0 = maj == 2 ? k : min(za, zb), z1 = maj == 2 ? k : max(za, zb);
                for (int32_t x = x0; x <= x1; ++x)
                    for (int32_t y = y0; y <= y1; ++y) {
                        // the cells of one column are one contiguous run of records
                        const int64_t col = ((int64_t)x * gy + y) * gz;
                        int32_t r = cell_start[col + z0], e = cell_start[col + z1 + 1];
                        r = min(max(r, 0), (int32_t)n_pairs);
                        e = min(max(e, r), (int32_t)n_pairs);
                        tests += (unsigned long long)(e - r);
                        for (; r < e; ++r)
                            mr_test_record(rec[(int64_t)r * kRecVec], rec[(int64_t)r * kRecVec + 1],
                                           rec[(int64_t)r * kRecVec + 2], o, d, t_min, t_max, pad, B);
                    }
            }
            if (k == k1) break;
            float tb;
            const bool checked = mr_checked(om, dm, lom, G.h, gm, s, -1, k + s, tb);
            if (checked && B.t <= tb) break;   // the stopping rule
            t_lo = checked ? fmaxf(t_min, tb) : t_min;
            k += s;
        }
    }

    if (n_tests) {   // diagnostic only: an integer count
        const unsigned long long total = hm_wave_reduce(tests, HmSum{});
        if (lane == 0) atomicAdd(n_tests, total);
    }
    if (live) {
        const bool hit = B.face != kNoFace;
        t_out[i] = hit ? B.t : INFINITY;
        face_out[i] = hit ? B.face : -1;
        if (uv_out) {
            uv_out[i * 2] = hit ? B.u : NAN;
            uv_out[i * 2 + 1] = hit ? B.v : NAN;
        }
        if (point_out) {
            point_out[i * 3] = hit ? B.p.x : NAN;
            point_out[i * 3 + 1] = hit ? B.p.y : NAN;
            point_out[i * 3 + 2] = hit ? B.p.z : NAN;
        }
    }
}

}  // namespace

extern "C" {

int hm_mesh_ray_cast(const float *origins, const float *dirs, const float *t_min, const float *t_max, int64_t m,
                     const float *records, int64_t n_pairs, int64_t n_big, const int32_t *cell_start, const float *lo,
                     float h, const int32_t *g, float pad, float *t, int32_t *face, float *uv, float *point,
                     int32_t *status, uint64_t *n_tests, void *stream) {
    HM_CHECK_ARG(m >= 0 && m < ((int64_t)1 << 31), "hm_mesh_ray_cast: m must be in [0, 2^31)");
    if (int rc = md_check_counts(n_pairs, n_big, "hm_mesh_ray_cast")) return rc;
    NnGrid G;
    int64_t cells;
    if (int rc = nn_grid(lo, h, g, "hm_mesh_ray_cast", G, cells)) return rc;
    HM_CHECK_ARG(std::isfinite(pad) && pad >= 0.0f, "hm_mesh_ray_cast: pad must be finite and >= 0");
    if (m == 0) return HM_OK;
    HM_CHECK_ARG(origins && dirs && records && cell_start && t && face && status, "hm_mesh_ray_cast: NULL pointer");
    hipLaunchKernelGGL(mr_cast_kernel, dim3(hm_grid(m, 64)), dim3(64), 0, as_stream(stream), origins, dirs, t_min,
                       t_max, m, reinterpret_cast<const float4 *>(records), n_pairs, n_big, cell_start, G, pad, t, face,
                       uv, point, status, reinterpret_cast<unsigned long long *>(n_tests));
    HM_CHECK_LAUNCH("hm_mesh_ray_cast");
    return HM_OK;
}

}  // extern "C"
