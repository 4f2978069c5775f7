// hm_mesh_dist.hip - exact fp32 point-to-triangle-mesh distance on a uniform grid: for every query the closest point
// of the mesh, the face it lies on, the face's feature (interior or one of its three edges) and the squared distance
// (contract and the definition of the per-face value: include/hashmod.h; DESIGN.md "Point-to-mesh distance on the
// device"; numpy restatement: tests/mesh_dist_cases.closest_ref).
//
//   hm_mesh_dist_count  md_count   one lane per face: its cell box nn_cell(lo) .. nn_cell(hi) per axis; count[f] = the
//                                  cells of the box, or 0 and big[f] = 1 when there are more than big_face of them
//                                  (hm_mesh_index_count / hm_mesh_index_build: the same with the box grown by a pad,
//                                  nn_cell(fl(lo - pad)) .. nn_cell(fl(hi + pad)), the index hm_mesh_ray.hip walks; the
//                                  hm_mesh_dist_* entry points forward with pad = 0.  A padded index lists a superset
//                                  of the cells, which the stopping rule below allows: it needs AT LEAST the box's)
//   (caller)                       exclusive prefix sums of count and big, their totals read by the host
//   hm_mesh_dist_build  md_emit    (cell key, face) pairs, faces ascending, a face's cells in key order; the big faces'
//                                  records, ascending, behind the pair records
//                       hm_sort_pairs_i32 (stable)  ->  the faces of one cell are one run, in ascending face index
//                       md_records record r = the three vertices and the face index of the r-th sorted pair, 48 bytes
//                       nn_cell_start  cell_start[c] = first sorted pair whose key is >= c
//   hm_mesh_dist_query  nn_key + sort  the queries ordered by their (clamped) cell
//                       md_query   one wave per 64 consecutive sorted queries: hm_nn.hip's box walk with a triangle test
//
// md_query.  As nn_query (hm_nn.hip): the wave's box is the cell box of its lanes' cells grown by a ring; the cells of
// a column (cx, cy) are one contiguous run of records; the lanes look the ranges up 64 at a time, a wave prefix sum
// lays them end to end, the records are staged in LDS kChunk at a time, and EVERY lane tests EVERY staged record from
// a wave-uniform LDS address, first against the face's bounding box (md_test, "the box reject") and, when the box is
// not farther than the lane's best, in full.  Before the walk every wave tests the whole big-face run.  A face listed
// in several cells of the box is tested several times; under the total order (d2, face) a repeat changes nothing.  A
// lane's result is the argmin over a superset of the faces it needs, so it does not depend on the wave, the box or
// the grid.
//
// THE STOPPING RULE FOR TRIANGLES.  It is nn_face_low / nn_face_high (hm_nn_dev.h) unchanged; what has to be shown is
// that a face the walk has not tested cannot beat or tie a lane whose best d2 is < b2.  Every candidate point of a
// face is clamped per axis into the face's fp32 bounding box [lo, hi] BEFORE its distance is taken, so the value of a
// face is fl-dot(q - p, q - p) of a point p with lo <= p <= hi on every axis.  A face is listed in every cell of
// [nn_cell(lo), nn_cell(hi)] (or it is big, and then it was tested).  The walk has scanned every cell of the box
// [b0, b1]: the cells of each new box that were not in the box before it.  A face that is in none of them has a cell
// box disjoint from [b0, b1], so on some axis nn_cell(hi) < b0 or nn_cell(lo) > b1.  In the first case, F =
// nn_face_low(b0) has been CHECKED to satisfy nn_cell(F) >= b0 > nn_cell(hi), and nn_cell being monotone, hi < F;
// hence p <= hi < F on that axis.  For q >= F, rounding being monotone: fl(q - p) >= fl(q - F) >= 0, fl(fl(q - p)^2)
// >= fl(fl(q - F)^2), and adding the other two non-negative squares never rounds below the first term (the sum order
// (x + y) + z is covered for each axis: a sum of non-negative terms is >= each of them after rounding).  So the face's
// value, whichever of its four candidates wins, is >= b2 > best: neither a better minimum nor a tie.  The second case
// is the mirror image with nn_face_high.  q < F gives the bound 0, which finishes nothing.  The end conditions are
// nn_query's: best < b2, b2 > max_d2 (nothing to report beyond the box), or the box covers the grid.
#include <math.h>

#include "hm_block_dev.h"
#include "hm_mesh_rec_dev.h"
#include "hm_nn_dev.h"

namespace {

constexpr int kChunk = 256;   // records staged in LDS per pass (12 KiB)

// ---- the face value (include/hashmod.h), every operation rounded once: the vector operations are hm_mesh_rec_dev.h's
// min(max(p, lo), hi) per axis; fmaxf / fminf return the other operand for a NaN, so the result is always in the box
__device__ __forceinline__ MdVec md_clamp(MdVec p, MdVec lo, MdVec hi) {
    return {fminf(fmaxf(p.x, lo.x), hi.x), fminf(fmaxf(p.y, lo.y), hi.y), fminf(fmaxf(p.z, lo.z), hi.z)};
}

struct MdBest {
    float d2;
    int32_t face;
    MdVec p;
    int32_t feature;
};

// candidate k of the face: its point, clamped into the face's box, replaces the face's current one when strictly nearer
__device__ __forceinline__ void md_candidate(MdVec q, MdVec point, MdVec lo, MdVec hi, int32_t k, float &d2, MdVec &p,
                                             int32_t &feature) {
    const MdVec c = md_clamp(point, lo, hi);
    const MdVec w = md_sub(q, c);
    const float d = md_dot(w, w);
    const bool better = d < d2;
    d2 = better ? d : d2;
    feature = better ? k : feature;
    p.x = better ? c.x : p.x;
    p.y = better ? c.y : p.y;
    p.z = better ? c.z : p.z;
}

__device__ __forceinline__ void md_segment(MdVec q, MdVec p0, MdVec p1, MdVec lo, MdVec hi, int32_t k, float &d2,
                                           MdVec &p, int32_t &feature) {
    const MdVec e = md_sub(p1, p0);
    const float ee = md_dot(e, e);
    float t = ee > 0.0f ? __fdiv_rn(md_dot(md_sub(q, p0), e), ee) : 0.0f;
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    md_candidate(q, md_along(p0, t, e), lo, hi, k, d2, p, feature);
}

// the value of face (a, b, c) for q, merged into B under the total order (d2, face)
__device__ __forceinline__ void md_test(MdVec q, MdVec a, MdVec b, MdVec c, int32_t face, MdBest &B) {
    const MdVec lo = {fminf(fminf(a.x, b.x), c.x), fminf(fminf(a.y, b.y), c.y), fminf(fminf(a.z, b.z), c.z)};
    const MdVec hi = {fmaxf(fmaxf(a.x, b.x), c.x), fmaxf(fmaxf(a.y, b.y), c.y), fmaxf(fmaxf(a.z, b.z), c.z)};
    // THE BOX REJECT.  Every candidate point c of this face was clamped into [lo, hi], and g = clamp(q) is the box's
    // nearest point to q per axis: q >= hi gives g = hi >= c, q <= lo gives g = lo <= c, and in between g = q.  So
    // |q - c| >= |q - g| per axis, and by the monotonicity of rounding (the argument at nn_face_low) the face's value
    // in fp32 is >= the box's, computed here by the same expression.  A box farther than the lane's best therefore
    // holds neither a better minimum nor a tie; an equal one is still tested, for the tie.  Most faces of a wave's
    // cell box are far from all of its lanes, which then skip the test together.
    const MdVec wg = md_sub(q, md_clamp(q, lo, hi));
    if (md_dot(wg, wg) > B.d2) return;
    float d2 = INFINITY;
    MdVec p = {NAN, NAN, NAN};
    int32_t feature = -1;
    // candidate 0: the projection onto the plane, when it falls inside the triangle
    const MdVec n = md_cross(md_sub(b, a), md_sub(c, a));
    const float nn = md_dot(n, n);
    const MdVec wa = md_sub(a, q), wb = md_sub(b, q), wc = md_sub(c, q);
    if (nn > 0.0f && md_dot(n, md_cross(wa, wb)) >= 0.0f && md_dot(n, md_cross(wb, wc)) >= 0.0f &&
        md_dot(n, md_cross(wc, wa)) >= 0.0f)
        md_candidate(q, md_along(q, __fdiv_rn(md_dot(wa, n), nn), n), lo, hi, 0, d2, p, feature);
    md_segment(q, a, b, lo, hi, 1, d2, p, feature);
    md_segment(q, b, c, lo, hi, 2, d2, p, feature);
    md_segment(q, c, a, lo, hi, 3, d2, p, feature);
    const bool better = d2 < B.d2 || (d2 == B.d2 && face < B.face);
    B.d2 = better ? d2 : B.d2;
    B.face = better ? face : B.face;
    B.feature = better ? feature : B.feature;
    B.p.x = better ? p.x : B.p.x;
    B.p.y = better ? p.y : B.p.y;
    B.p.z = better ? p.z : B.p.z;
}

// ---- build ---------------------------------------------------------------------------------------------------------
// the vertices of face f and its cell box, the cells of fl(min - pad) .. fl(max + pad) per axis (pad = 0: of the
// bounding box itself, x - 0 being x); false (and a status bit: 1 an index outside [0, n_verts), 2 a non-finite
// vertex) for a face that is not to be listed.  No vertex is read through an index that was not checked.
__device__ __forceinline__ bool md_face(const float *__restrict__ verts, const int32_t *__restrict__ faces, int64_t f,
                                        int64_t n_verts, const NnGrid &G, float pad, int32_t *status, float (&v)[9],
                                        int32_t (&c0)[3], int32_t (&c1)[3]) {
    int32_t id[3];
    const bool in_range = status ? hm_face_ids(faces, f, n_verts, id, status) : hm_face_ids(faces, f, n_verts, id);
    if (!in_range) return false;
    bool finite = true;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
#pragma unroll
        for (int a = 0; a < 3; ++a) v[m * 3 + a] = verts[(int64_t)id[m] * 3 + a];
        finite = finite && nn_finite3(v[m * 3], v[m * 3 + 1], v[m * 3 + 2]);
    }
    if (!finite) {
        if (status) atomicOr(status, 2);
        return false;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c0[a] = nn_cell(__fsub_rn(fminf(fminf(v[a], v[3 + a]), v[6 + a]), pad), G.lo[a], G.h, G.g[a]);
        c1[a] = nn_cell(__fadd_rn(fmaxf(fmaxf(v[a], v[3 + a]), v[6 + a]), pad), G.lo[a], G.h, G.g[a]);
    }
    return true;
}

__global__ __launch_bounds__(kNT) void md_count_kernel(const float *__restrict__ verts,
                                                       const int32_t *__restrict__ faces, int64_t n_faces,
                                                       int64_t n_verts, NnGrid G, float pad, int64_t big_face,
                                                       int32_t *__restrict__ count, int32_t *__restrict__ big,
                                                       int32_t *status) {
    const int64_t f = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (f >= n_faces) return;
    float v[9];
    int32_t c0[3], c1[3];
    int32_t n = 0, is_big = 0;
    if (md_face(verts, faces, f, n_verts, G, pad, status, v, c0, c1)) {
        // at most the cells of the grid: < 2^31
        const int64_t cells = (int64_t)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
        is_big = cells > big_face ? 1 : 0;
        n = is_big ? 0 : (int32_t)cells;
    }
    count[f] = n;
    big[f] = is_big;
}

__device__ __forceinline__ void md_store_record(float4 *__restrict__ rec, int64_t r, const float (&v)[9],
                                                int32_t face) {
    rec[r * kRecVec] = make_float4(v[0], v[1], v[2], v[3]);
    rec[r * kRecVec + 1] = make_float4(v[4], v[5], v[6], v[7]);
    rec[r * kRecVec + 2] = make_float4(v[8], __int_as_float(face), 0.0f, 0.0f);
}

// every write is checked against the totals the host read, so prefix sums that do not belong to these counts cannot
// send a store outside key / pair_face / rec
__global__ __launch_bounds__(kNT) void md_emit_kernel(const float *__restrict__ verts,
                                                      const int32_t *__restrict__ faces, int64_t n_faces,
                                                      int64_t n_verts, NnGrid G, float pad,
                                                      const int32_t *__restrict__ count,
                                                      const int32_t *__restrict__ big,
                                                      const int32_t *__restrict__ prefix, int64_t n_pairs,
                                                      const int32_t *__restrict__ big_prefix, int64_t n_big,
                                                      int32_t *__restrict__ key, int32_t *__restrict__ pair_face,
                                                      float4 *__restrict__ rec) {
    const int64_t f = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (f >= n_faces) return;
    const bool is_big = big[f] != 0;
    if (!is_big && count[f] <= 0) return;
    float v[9];
    int32_t c0[3], c1[3];
    if (!md_face(verts, faces, f, n_verts, G, pad, nullptr, v, c0, c1)) return;
    if (is_big) {
        const int64_t o = big_prefix[f];
        if (o >= 0 && o < n_big) md_store_record(rec, n_pairs + o, v, (int32_t)f);
        return;
    }
    int64_t o = prefix[f];
    const int64_t end = o + count[f];
    if (o < 0 || end > n_pairs) return;
    for (int32_t x = c0[0]; x <= c1[0]; ++x)
        for (int32_t y = c0[1]; y <= c1[1]; ++y)
            for (int32_t z = c0[2]; z <= c1[2]; ++z) {
                if (o >= end) return;
                key[o] = (x * G.g[1] + y) * G.g[2] + z;
                pair_face[o] = (int32_t)f;
                ++o;
            }
}

__global__ __launch_bounds__(kNT) void md_records_kernel(const float *__restrict__ verts,
                                                         const int32_t *__restrict__ faces, int64_t n_faces,
                                                         int64_t n_verts, const int32_t *__restrict__ pair_face,
                                                         const int64_t *__restrict__ perm, int64_t n_pairs,
                                                         float4 *__restrict__ rec) {
    const int64_t r = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (r >= n_pairs) return;
    int64_t i = perm[r];
    if ((uint64_t)i >= (uint64_t)n_pairs) i = 0;
    const int32_t f = pair_face[i];
    float v[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = NAN;   // a record that cannot be read never wins: its d2 is NaN
    int32_t id[3];
    int32_t face = kNoFace;
    if ((uint64_t)(int64_t)f < (uint64_t)n_faces && hm_face_ids(faces, f, n_verts, id)) {
        face = f;
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int a = 0; a < 3; ++a) v[m * 3 + a] = verts[(int64_t)id[m] * 3 + a];
    }
    md_store_record(rec, r, v, face);
}

// ---- query ---------------------------------------------------------------------------------------------------------
// every lane tests the cnt records staged in LDS, each read at a wave-uniform address
__device__ __forceinline__ void md_test_staged(const float4 *stage, int32_t cnt, MdVec q, MdBest &B) {
#pragma unroll 2
    for (int32_t c = 0; c < cnt; ++c) {
        const float4 r0 = stage[c * kRecVec], r1 = stage[c * kRecVec + 1], r2 = stage[c * kRecVec + 2];
        md_test(q, {r0.x, r0.y, r0.z}, {r0.w, r1.x, r1.y}, {r1.z, r1.w, r2.x}, __float_as_int(r2.y), B);
    }
}

__global__ __launch_bounds__(64) void md_query_kernel(const float *__restrict__ query, int64_t m,
                                                      const int64_t *__restrict__ qperm,
                                                      const float4 *__restrict__ rec, int64_t n_pairs, int64_t n_big,
                                                      const int32_t *__restrict__ cell_start, NnGrid G, float max_d2,
                                                      float *__restrict__ d2_out, int32_t *__restrict__ face_out,
                                                      float *__restrict__ point_out, int32_t *__restrict__ feature_out,
                                                      unsigned long long *n_tests) {
    __shared__ float4 stage[kChunk * kRecVec];
    __shared__ int32_t it_beg[64];
    __shared__ int32_t it_off[65];
    const int lane = threadIdx.x;
    const int64_t first_q = (int64_t)blockIdx.x * 64;
    const bool live = first_q + lane < m;
    // a lane past the end repeats the wave's first query, so that it does not widen the box
    int64_t src = qperm[live ? first_q + lane : first_q];
    if ((uint64_t)src >= (uint64_t)m) src = 0;
    const MdVec q = {query[src * 3], query[src * 3 + 1], query[src * 3 + 2]};
    bool done = !live || !nn_finite3(q.x, q.y, q.z);

    MdBest B = {INFINITY, kNoFace, {NAN, NAN, NAN}, -1};
    unsigned long long staged = 0;   // records this wave has tested (every lane tests each of them)

    // the big faces: one run behind the pair records, tested in full
    for (int64_t t0 = 0; t0 < n_big; t0 += kChunk) {
        const int32_t cnt = (int32_t)min((int64_t)kChunk, n_big - t0);
#pragma unroll
        for (int u = 0; u < kChunk / 64; ++u) {
            const int32_t slot = u * 64 + lane;
            if (slot < cnt) {
#pragma unroll
                for (int k = 0; k < kRecVec; ++k) stage[slot * kRecVec + k] = rec[(n_pairs + t0 + slot) * kRecVec + k];
            }
        }
        __syncthreads();
        md_test_staged(stage, cnt, q, B);
        __syncthreads();
        staged += (unsigned long long)cnt;
    }

    const int32_t gx = G.g[0], gy = G.g[1], gz = G.g[2];
    const int32_t cx = nn_cell(q.x, G.lo[0], G.h, gx), cy = nn_cell(q.y, G.lo[1], G.h, gy),
                  cz = nn_cell(q.z, G.lo[2], G.h, gz);
    // the box [b0, b1] per axis (wave-uniform), and the box scanned so far [o0, o1]
    int32_t b0x = max(hm_wave_reduce(cx, HmMin{}) - 1, 0), b1x = min(hm_wave_reduce(cx, HmMax{}) + 1, gx - 1);
    int32_t b0y = max(hm_wave_reduce(cy, HmMin{}) - 1, 0), b1y = min(hm_wave_reduce(cy, HmMax{}) + 1, gy - 1);
    int32_t b0z = max(hm_wave_reduce(cz, HmMin{}) - 1, 0), b1z = min(hm_wave_reduce(cz, HmMax{}) + 1, gz - 1);
    int32_t o0x = 0, o1x = -1, o0y = 0, o1y = -1, o0z = 0, o1z = -1;
    int32_t ring = 1;

    for (;;) {
        const int32_t ny = b1y - b0y + 1;
        const int64_t n_items = (int64_t)(b1x - b0x + 1) * ny * 2;   // two z-ranges per column: below / above the old box
        for (int64_t base = 0; base < n_items; base += 64) {
            const int64_t it = base + lane;
            int32_t s = 0, e = 0;
            if (it < n_items) {
                const int32_t col = (int32_t)(it >> 1), part = (int32_t)(it & 1);
                const int32_t x = b0x + col / ny, y = b0y + col % ny;
                const bool seen = x >= o0x && x <= o1x && y >= o0y && y <= o1y;
                int32_t z0, z1;
                if (!seen) {
                    z0 = part ? 1 : b0z;
                    z1 = part ? 0 : b1z;
                } else {
                    z0 = part ? o1z + 1 : b0z;
                    z1 = part ? b1z : o0z - 1;
                }
                if (z0 <= z1) {
                    const int64_t k = ((int64_t)x * gy + y) * gz;
                    s = cell_start[k + z0];
                    e = cell_start[k + z1 + 1];
                    s = min(max(s, 0), (int32_t)n_pairs);
                    e = min(max(e, s), (int32_t)n_pairs);
                }
            }
            // the ranges of one group are disjoint parts of [0, n_pairs): their lengths sum to < 2^31
            int32_t incl = e - s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int32_t up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            __syncthreads();
            it_beg[lane] = s;
            it_off[lane + 1] = incl;
            if (lane == 0) it_off[0] = 0;
            __syncthreads();
            const int32_t total = it_off[64];
            staged += (unsigned long long)total;
            for (int32_t t0 = 0; t0 < total; t0 += kChunk) {
                const int32_t cnt = min(kChunk, total - t0);
#pragma unroll
                for (int u = 0; u < kChunk / 64; ++u) {
                    const int32_t slot = u * 64 + lane;
                    if (slot < cnt) {
                        const int32_t t = t0 + slot;
                        int a = 0, b = 64;   // the item j with it_off[j] <= t < it_off[j + 1]
                        while (a < b) {
                            const int mid = (a + b) >> 1;
                            if (it_off[mid + 1] <= t) a = mid + 1;
                            else b = mid;
                        }
                        const int64_t r = (int64_t)it_beg[a] + (t - it_off[a]);
#pragma unroll
                        for (int k = 0; k < kRecVec; ++k) stage[slot * kRecVec + k] = rec[r * kRecVec + k];
                    }
                }
                __syncthreads();
                md_test_staged(stage, cnt, q, B);
                __syncthreads();
            }
        }

        // the stopping rule (see the head of the file and nn_face_low)
        float b2 = INFINITY;
        if (b0x > 0) {
            const float b = fmaxf(__fsub_rn(q.x, nn_face_low(G.lo[0], G.h, gx, b0x)), 0.0f);
            b2 = fminf(b2, __fmul_rn(b, b));
        }
        if (b1x < gx - 1) {
            const float b = fmaxf(__fsub_rn(nn_face_high(G.lo[0], G.h, gx, b1x), q.x), 0.0f);
            b2 = fminf(b2, __fmul_rn(b, b));
        }
        if (b0y > 0) {
            const float b = fmaxf(__fsub_rn(q.y, nn_face_low(G.lo[1], G.h, gy, b0y)), 0.0f);
            b2 = fminf(b2, __fmul_rn(b, b));
        }
        if (b1y < gy - 1) {
            const float b = fmaxf(__fsub_rn(nn_face_high(G.lo[1], G.h, gy, b1y), q.y), 0.0f);
            b2 = fminf(b2, __fmul_rn(b, b));
        }
        if (b0z > 0) {
            const float b = fmaxf(__fsub_rn(q.z, nn_face_low(G.lo[2], G.h, gz, b0z)), 0.0f);
            b2 = fminf(b2, __fmul_rn(b, b));
        }
        if (b1z < gz - 1) {
            const float b = fmaxf(__fsub_rn(nn_face_high(G.lo[2], G.h, gz, b1z), q.z), 0.0f);
            b2 = fminf(b2, __fmul_rn(b, b));
        }
        // every face beyond the box is at d2 >= b2: no better minimum and no tie when best < b2, nothing to report
        // when b2 > max_d2
        done = done || B.d2 < b2 || b2 > max_d2;
        const bool covers = b0x == 0 && b0y == 0 && b0z == 0 && b1x == gx - 1 && b1y == gy - 1 && b1z == gz - 1;
        if (covers || __all(done)) break;

        o0x = b0x, o1x = b1x, o0y = b0y, o1y = b1y, o0z = b0z, o1z = b1z;
        b0x = max(b0x - ring, 0), b1x = (int32_t)min((int64_t)b1x + ring, (int64_t)gx - 1);
        b0y = max(b0y - ring, 0), b1y = (int32_t)min((int64_t)b1y + ring, (int64_t)gy - 1);
        b0z = max(b0z - ring, 0), b1z = (int32_t)min((int64_t)b1z + ring, (int64_t)gz - 1);
        ring = min(ring * 2, 1 << 20);
    }

    if (n_tests && lane == 0) atomicAdd(n_tests, staged * 64ull);   // diagnostic only: an integer count
    if (live) {
        const bool hit = B.face != kNoFace && B.d2 <= max_d2;   // false for a NaN distance
        d2_out[src] = hit ? B.d2 : INFINITY;
        face_out[src] = hit ? B.face : -1;
        if (point_out) {
            point_out[src * 3] = hit ? B.p.x : NAN;
            point_out[src * 3 + 1] = hit ? B.p.y : NAN;
            point_out[src * 3 + 2] = hit ? B.p.z : NAN;
        }
        if (feature_out) feature_out[src] = hit ? B.feature : -1;
    }
}

// [hm_keysort_layout(n) | pair_face n i32]
struct MdWs {
    HmKeySortWs sort;
    int32_t *pair_face;
    int64_t bytes;
};

MdWs md_layout(void *ws, int64_t n) {
    MdWs w;
    w.sort = hm_keysort_layout(ws, n);
    HmCarve c(ws);
    c.bytes = w.sort.bytes;
    w.pair_face = c.take<int32_t>(n);
    w.bytes = c.bytes;
    return w;
}

}  // namespace

extern "C" {

int64_t hm_mesh_dist_workspace_bytes(int64_t n) {
    if (n < 0 || n >= ((int64_t)1 << 31))
        return hm_fail(HM_ERR_INVALID, "hm_mesh_dist_workspace_bytes: n must be in [0, 2^31)");
    return md_layout(nullptr, n).bytes;
}

int hm_mesh_index_count(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts, const float *lo,
                        float h, const int32_t *g, float pad, int64_t big_face, int32_t *count, int32_t *big,
                        int32_t *status, void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_index_count")) return rc;
    HM_CHECK_ARG(n_faces >= 1, "hm_mesh_index_count: at least one face is needed");
    NnGrid G;
    int64_t cells;
    if (int rc = nn_grid(lo, h, g, "hm_mesh_index_count", G, cells)) return rc;
    HM_CHECK_ARG(big_face >= 1, "hm_mesh_index_count: big_face must be >= 1");
    HM_CHECK_ARG(std::isfinite(pad) && pad >= 0.0f, "hm_mesh_index_count: pad must be finite and >= 0");
    HM_CHECK_ARG((verts || n_verts == 0) && count && big && status, "hm_mesh_index_count: NULL pointer");
    hipLaunchKernelGGL(md_count_kernel, dim3(hm_grid(n_faces, kNT)), dim3(kNT), 0, as_stream(stream), verts, faces,
                       n_faces, n_verts, G, pad, big_face, count, big, status);
    HM_CHECK_LAUNCH("hm_mesh_index_count");
    return HM_OK;
}

int hm_mesh_index_build(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts, const float *lo,
                        float h, const int32_t *g, float pad, const int32_t *count, const int32_t *big,
                        const int32_t *prefix, int64_t n_pairs, const int32_t *big_prefix, int64_t n_big,
                        int32_t *cell_start, float *records, void *workspace, int64_t workspace_bytes, void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_index_build")) return rc;
    HM_CHECK_ARG(n_faces >= 1, "hm_mesh_index_build: at least one face is needed");
    NnGrid G;
    int64_t cells;
    if (int rc = nn_grid(lo, h, g, "hm_mesh_index_build", G, cells)) return rc;
    if (int rc = md_check_counts(n_pairs, n_big, "hm_mesh_index_build")) return rc;
    HM_CHECK_ARG(std::isfinite(pad) && pad >= 0.0f, "hm_mesh_index_build: pad must be finite and >= 0");
    HM_CHECK_ARG(verts && count && big && prefix && big_prefix && cell_start && records && workspace,
                 "hm_mesh_index_build: NULL pointer");
    HM_CHECK_ARG(workspace_bytes >= hm_mesh_dist_workspace_bytes(n_pairs),
                 "hm_mesh_index_build: workspace too small");
    const MdWs w = md_layout(workspace, n_pairs);
    hipStream_t st = as_stream(stream);
    float4 *rec = reinterpret_cast<float4 *>(records);
    hipLaunchKernelGGL(md_emit_kernel, dim3(hm_grid(n_faces, kNT)), dim3(kNT), 0, st, verts, faces, n_faces, n_verts, G,
                       pad, count, big, prefix, n_pairs, big_prefix, n_big, w.sort.key, w.pair_face, rec);
    if (n_pairs > 0) {
        int key_bits = 1;
        while (key_bits < 31 && ((int64_t)1 << key_bits) < cells) ++key_bits;
        if (int rc = hm_sort_pairs_i32(w.sort.key, n_pairs, key_bits, w.sort.keys_sorted, w.sort.perm, w.sort.sort_ws,
                                       w.sort.sort_bytes, stream))
            return rc;
        hipLaunchKernelGGL(md_records_kernel, dim3(hm_grid(n_pairs, kNT)), dim3(kNT), 0, st, verts, faces, n_faces,
                           n_verts, static_cast<const int32_t *>(w.pair_face),
                           static_cast<const int64_t *>(w.sort.perm), n_pairs, rec);
    }
    hipLaunchKernelGGL(nn_cell_start_kernel, dim3(hm_grid(cells + 1, kNT)), dim3(kNT), 0, st,
                       static_cast<const int32_t *>(w.sort.keys_sorted), n_pairs, cells, cell_start);
    HM_CHECK_LAUNCH("hm_mesh_index_build");
    return HM_OK;
}

// the index without a pad: the cells of the faces' own bounding boxes
int hm_mesh_dist_count(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts, const float *lo,
                       float h, const int32_t *g, int64_t big_face, int32_t *count, int32_t *big, int32_t *status,
                       void *stream) {
    return hm_mesh_index_count(verts, faces, n_faces, n_verts, lo, h, g, 0.0f, big_face, count, big, status, stream);
}

int hm_mesh_dist_build(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts, const float *lo,
                       float h, const int32_t *g, const int32_t *count, const int32_t *big, const int32_t *prefix,
                       int64_t n_pairs, const int32_t *big_prefix, int64_t n_big, int32_t *cell_start, float *records,
                       void *workspace, int64_t workspace_bytes, void *stream) {
    return hm_mesh_index_build(verts, faces, n_faces, n_verts, lo, h, g, 0.0f, count, big, prefix, n_pairs, big_prefix,
                               n_big, cell_start, records, workspace, workspace_bytes, stream);
}

int hm_mesh_dist_query(const float *query, int64_t m, const float *records, int64_t n_pairs, int64_t n_big,
                       const int32_t *cell_start, const float *lo, float h, const int32_t *g, float max_dist2, float *d2,
                       int32_t *face, float *point, int32_t *feature, void *workspace, int64_t workspace_bytes,
                       int32_t *status, uint64_t *n_tests, void *stream) {
    HM_CHECK_ARG(m >= 0 && m < ((int64_t)1 << 31), "hm_mesh_dist_query: m must be in [0, 2^31)");
    if (int rc = md_check_counts(n_pairs, n_big, "hm_mesh_dist_query")) return rc;
    NnGrid G;
    int64_t cells;
    if (int rc = nn_grid(lo, h, g, "hm_mesh_dist_query", G, cells)) return rc;
    HM_CHECK_ARG(!(max_dist2 != max_dist2) && max_dist2 >= 0.0f,
                 "hm_mesh_dist_query: max_dist2 must be >= 0 (inf for none)");
    if (m == 0) return HM_OK;
    HM_CHECK_ARG(query && records && cell_start && d2 && face && workspace && status,
                 "hm_mesh_dist_query: NULL pointer");
    HM_CHECK_ARG(workspace_bytes >= hm_mesh_dist_workspace_bytes(m), "hm_mesh_dist_query: workspace too small");
    const MdWs w = md_layout(workspace, m);
    if (int rc = nn_sorted_keys(query, m, G, cells, w.sort, status, 4, stream)) return rc;
    hipLaunchKernelGGL(md_query_kernel, dim3(hm_grid(m, 64)), dim3(64), 0, as_stream(stream), query, m,
                       static_cast<const int64_t *>(w.sort.perm), reinterpret_cast<const float4 *>(records), n_pairs,
                       n_big, cell_start, G, max_dist2, d2, face, point, feature,
                       reinterpret_cast<unsigned long long *>(n_tests));
    HM_CHECK_LAUNCH("hm_mesh_dist_query");
    return HM_OK;
}

}  // extern "C"
