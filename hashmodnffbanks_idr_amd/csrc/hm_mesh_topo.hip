// hm_mesh_topo.hip - the sign of the point-to-mesh distance: the angle-weighted pseudo-normals of a triangle mesh
// (Baerentzen and Aanaes) as two tables, and the sign of a closest-point result from them (contract and the definition:
// include/hashmod.h; DESIGN.md "Signed distance to the mesh on the device"; numpy restatement:
// tests/mesh_sign_cases.topology_ref / sign_ref).
//
//   hm_mesh_topology_build
//     mt_face     one lane per face: nu = n / |n| (fp64, zero for a face without area) and its three corner angles, the
//                 3 corner keys (vertex id) and the 3 half-edge key pairs (min, max); item i = 3 * face + k throughout
//     hm_sort_pairs_i32 (stable) of the corner keys  ->  the (face, corner) pairs of one vertex are one run, ascending
//     mt_vertex   the lane of every run head walks its run in sorted order and writes VN[v]
//     hm_sort_pairs_i32 by max, mt_regather, hm_sort_pairs_i32 by min: two stable passes order the half-edges by
//                 (min, max), and the members of one run stay in ascending (face, k) order
//     mt_edge     the lane of every run head walks its run, sums nu in sorted order, writes the sum to the slot of
//                 every member, and counts the run as a boundary, non-manifold or flipped edge (integer atomics)
//   hm_mesh_sign  one lane per query: the feature's normal from the tables, the sign of dot(w, N), sd = sign * sqrt(d2)
//
// No floating-point atomic anywhere: every sum is formed by ONE lane in the order the stable sorts fixed, so the tables
// do not depend on the thread order.  A vertex or an edge with a very long run is walked by one lane.  The fp64
// operations are __dadd_rn and friends: rounded once, never contracted, whatever the build flags.
#include <math.h>

#include "hm_block_dev.h"
#include "hm_mesh_rec_dev.h"
#include "hm_nn_dev.h"

namespace {

struct MtVec {
    double x, y, z;
};
__device__ __forceinline__ MtVec mt_wide(MdVec v) { return {(double)v.x, (double)v.y, (double)v.z}; }
__device__ __forceinline__ MtVec mt_sub(MtVec u, MtVec v) {
    return {__dsub_rn(u.x, v.x), __dsub_rn(u.y, v.y), __dsub_rn(u.z, v.z)};
}
__device__ __forceinline__ double mt_dot(MtVec u, MtVec v) {
    return __dadd_rn(__dadd_rn(__dmul_rn(u.x, v.x), __dmul_rn(u.y, v.y)), __dmul_rn(u.z, v.z));
}
__device__ __forceinline__ MtVec mt_cross(MtVec u, MtVec v) {
    return {__dsub_rn(__dmul_rn(u.y, v.z), __dmul_rn(u.z, v.y)), __dsub_rn(__dmul_rn(u.z, v.x), __dmul_rn(u.x, v.z)),
            __dsub_rn(__dmul_rn(u.x, v.y), __dmul_rn(u.y, v.x))};
}
// the angle at corner p between the edges to p1 and p2
__device__ __forceinline__ double mt_angle(MtVec p, MtVec p1, MtVec p2) {
    const MtVec e1 = mt_sub(p1, p), e2 = mt_sub(p2, p);
    const MtVec x = mt_cross(e1, e2);
    return atan2(__dsqrt_rn(mt_dot(x, x)), mt_dot(e1, e2));
}

__device__ __forceinline__ MdVec mt_vertex(const float *__restrict__ verts, int32_t id) {
    return {verts[(int64_t)id * 3], verts[(int64_t)id * 3 + 1], verts[(int64_t)id * 3 + 2]};
}

// ---- build ---------------------------------------------------------------------------------------------------------
// A face that cannot be read (status bit 0: an index outside [0, n_verts); bit 1: a non-finite vertex) gets zero
// quantities and the keys of vertex 0; no vertex is read through an index that was not checked, and the caller rejects
// the whole result.
__global__ __launch_bounds__(kNT) void mt_face_kernel(const float *__restrict__ verts,
                                                      const int32_t *__restrict__ faces, int64_t n_faces,
                                                      int64_t n_verts, double *__restrict__ nu,
                                                      double *__restrict__ angle, int32_t *__restrict__ corner_key,
                                                      int32_t *__restrict__ emin, int32_t *__restrict__ emax,
                                                      int32_t *status) {
    const int64_t f = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (f >= n_faces) return;
    int32_t id[3];
    bool ok = hm_face_ids(faces, f, n_verts, id, status);
    MtVec u = {0.0, 0.0, 0.0};
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
    if (ok) {
        const MdVec a = mt_vertex(verts, id[0]), b = mt_vertex(verts, id[1]), c = mt_vertex(verts, id[2]);
        if (nn_finite3(a.x, a.y, a.z) && nn_finite3(b.x, b.y, b.z) && nn_finite3(c.x, c.y, c.z)) {
            const MtVec A = mt_wide(a), B = mt_wide(b), Cc = mt_wide(c);
            const MtVec n = mt_cross(mt_sub(B, A), mt_sub(Cc, A));
            const double nn = mt_dot(n, n);
            if (nn != 0.0) {
                const double len = __dsqrt_rn(nn);
                u = {__ddiv_rn(n.x, len), __ddiv_rn(n.y, len), __ddiv_rn(n.z, len)};
            }
            g0 = mt_angle(A, B, Cc);
            g1 = mt_angle(B, Cc, A);
            g2 = mt_angle(Cc, A, B);
        } else {
            atomicOr(status, 2);
            ok = false;
        }
    }
    const int32_t v0 = ok ? id[0] : 0, v1 = ok ? id[1] : 0, v2 = ok ? id[2] : 0;
    nu[f * 3] = u.x;
    nu[f * 3 + 1] = u.y;
    nu[f * 3 + 2] = u.z;
    angle[f * 3] = g0;
    angle[f * 3 + 1] = g1;
    angle[f * 3 + 2] = g2;
    corner_key[f * 3] = v0;
    corner_key[f * 3 + 1] = v1;
    corner_key[f * 3 + 2] = v2;
    emin[f * 3] = min(v0, v1);
    emax[f * 3] = max(v0, v1);
    emin[f * 3 + 1] = min(v1, v2);
    emax[f * 3 + 1] = max(v1, v2);
    emin[f * 3 + 2] = min(v2, v0);
    emax[f * 3 + 2] = max(v2, v0);
}

// an entry of a sorting permutation as an item, whatever the permutation holds
__device__ __forceinline__ int64_t mt_item(int64_t i, int64_t n) { return (uint64_t)i < (uint64_t)n ? i : 0; }

__global__ __launch_bounds__(kNT) void mt_vertex_kernel(const int32_t *__restrict__ keys_sorted,
                                                        const int64_t *__restrict__ perm, int64_t n, int64_t n_verts,
                                                        const double *__restrict__ nu,
                                                        const double *__restrict__ angle, double *__restrict__ vn) {
    const int64_t j = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (j >= n) return;
    const int32_t v = keys_sorted[j];
    if (j > 0 && keys_sorted[j - 1] == v) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int64_t r = j; r < n && keys_sorted[r] == v; ++r) {
        const int64_t item = mt_item(perm[r], n);
        const int64_t f = item / 3;
        const double g = angle[item];
        sx = __dadd_rn(sx, __dmul_rn(g, nu[f * 3]));
        sy = __dadd_rn(sy, __dmul_rn(g, nu[f * 3 + 1]));
        sz = __dadd_rn(sz, __dmul_rn(g, nu[f * 3 + 2]));
    }
    if ((uint64_t)(int64_t)v < (uint64_t)n_verts) {
        vn[(int64_t)v * 3] = sx;
        vn[(int64_t)v * 3 + 1] = sy;
        vn[(int64_t)v * 3 + 2] = sz;
    }
}

// between the two passes: the order after the first one, kept as items, and the second pass's keys in that order
__global__ __launch_bounds__(kNT) void mt_regather_kernel(const int64_t *__restrict__ perm, int64_t n,
                                                          const int32_t *__restrict__ emin,
                                                          int32_t *__restrict__ item1, int32_t *__restrict__ key) {
    const int64_t j = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (j >= n) return;
    const int64_t item = mt_item(perm[j], n);
    item1[j] = (int32_t)item;
    key[j] = emin[item];
}

// the item at sorted position r of the half-edges
__device__ __forceinline__ int64_t mt_edge_item(const int64_t *__restrict__ perm, const int32_t *__restrict__ item1,
                                                int64_t r, int64_t n) {
    return mt_item(item1[mt_item(perm[r], n)], n);
}

// true when half-edge `item` runs from its larger vertex to its smaller one
__device__ __forceinline__ bool mt_downward(const int32_t *__restrict__ faces, int64_t item) {
    const int64_t f = item / 3;
    const int k = (int)(item - f * 3);
    return faces[f * 3 + k] > faces[f * 3 + (k == 2 ? 0 : k + 1)];
}

__global__ __launch_bounds__(kNT) void mt_edge_kernel(const int32_t *__restrict__ min_sorted,
                                                      const int64_t *__restrict__ perm,
                                                      const int32_t *__restrict__ item1,
                                                      const int32_t *__restrict__ emax,
                                                      const int32_t *__restrict__ faces, int64_t n,
                                                      const double *__restrict__ nu, double *__restrict__ en,
                                                      unsigned long long *__restrict__ counts) {
    const int64_t j = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (j >= n) return;
    const int32_t lo = min_sorted[j];
    const int64_t head = mt_edge_item(perm, item1, j, n);
    const int32_t hi = emax[head];
    if (j > 0 && min_sorted[j - 1] == lo && emax[mt_edge_item(perm, item1, j - 1, n)] == hi) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int64_t end = j;
    int64_t second = head;
    for (; end < n && min_sorted[end] == lo; ++end) {
        const int64_t item = mt_edge_item(perm, item1, end, n);
        if (emax[item] != hi) break;
        if (end == j + 1) second = item;
        const int64_t f = item / 3;
        sx = __dadd_rn(sx, nu[f * 3]);
        sy = __dadd_rn(sy, nu[f * 3 + 1]);
        sz = __dadd_rn(sz, nu[f * 3 + 2]);
    }
    for (int64_t r = j; r < end; ++r) {
        const int64_t item = mt_edge_item(perm, item1, r, n);
        en[item * 3] = sx;
        en[item * 3 + 1] = sy;
        en[item * 3 + 2] = sz;
    }
    const int64_t len = end - j;
    if (len == 1) atomicAdd(counts, 1ull);
    else if (len > 2) atomicAdd(counts + 1, 1ull);
    else if (mt_downward(faces, head) == mt_downward(faces, second)) atomicAdd(counts + 2, 1ull);
}

// ---- the sign ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNT) void mt_sign_kernel(const float *__restrict__ query, int64_t m,
                                                      const int32_t *__restrict__ face_in,
                                                      const int32_t *__restrict__ feature_in,
                                                      const float *__restrict__ point, const float *__restrict__ d2,
                                                      const float *__restrict__ verts,
                                                      const int32_t *__restrict__ faces, int64_t n_faces,
                                                      int64_t n_verts, const double *__restrict__ vn,
                                                      const double *__restrict__ en, float *__restrict__ sd,
                                                      int32_t *__restrict__ sign_out) {
    const int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (i >= m) return;
    const int32_t face = face_in[i], feature = feature_in[i];
    int32_t id[3];
    // a cut query, and a face or a feature that cannot be one of this mesh: no sign
    const bool hit = (uint64_t)(int64_t)face < (uint64_t)n_faces && (uint32_t)feature <= 3u &&
                     hm_face_ids(faces, face, n_verts, id);
    float out = INFINITY;
    int32_t sg = 0;
    if (hit) {
        const MdVec q = {query[i * 3], query[i * 3 + 1], query[i * 3 + 2]};
        const MdVec a = mt_vertex(verts, id[0]), b = mt_vertex(verts, id[1]), c = mt_vertex(verts, id[2]);
        MdVec w;
        MtVec N;
        if (feature == 0) {
            w = md_sub(q, a);
            const MtVec A = mt_wide(a);
            N = mt_cross(mt_sub(mt_wide(b), A), mt_sub(mt_wide(c), A));
        } else {
            // the segment's end points and their indices, selected as scalars
            const MdVec p0 = feature == 1 ? a : feature == 2 ? b : c;
            const MdVec p1 = feature == 1 ? b : feature == 2 ? c : a;
            const int32_t i0 = feature == 1 ? id[0] : feature == 2 ? id[1] : id[2];
            const int32_t i1 = feature == 1 ? id[1] : feature == 2 ? id[2] : id[0];
            const MdVec e = md_sub(p1, p0);
            const float ee = md_dot(e, e);
            const float t = ee > 0.0f ? __fdiv_rn(md_dot(md_sub(q, p0), e), ee) : 0.0f;
            const double *__restrict__ src = t <= 0.0f   ? vn + (int64_t)i0 * 3
                                             : t >= 1.0f ? vn + (int64_t)i1 * 3
                                                         : en + ((int64_t)face * 3 + (feature - 1)) * 3;
            N = {src[0], src[1], src[2]};
            w = md_sub(q, {point[i * 3], point[i * 3 + 1], point[i * 3 + 2]});
        }
        const double s = mt_dot(mt_wide(w), N);
        sg = s < 0.0 ? -1 : 1;   // zero, and a NaN, are outside
        // sqrtf is the correctly rounded root here; __fsqrt_rn lowers to the approximate v_sqrt_f32 in this toolchain
        const float d = sqrtf(d2[i]);
        out = s < 0.0 ? -d : d;
    }
    sd[i] = out;
    if (sign_out) sign_out[i] = sg;
}

// [hm_keysort_layout(n) | nu F*3 f64 | angle n f64 | emin n i32 | emax n i32 | item1 n i32], n = 3 F
struct MtWs {
    HmKeySortWs sort;
    double *nu, *angle;
    int32_t *emin, *emax, *item1;
    int64_t bytes;
};

MtWs mt_layout(void *ws, int64_t n_faces) {
    const int64_t n = n_faces * 3;
    MtWs w;
    w.sort = hm_keysort_layout(ws, n);
    HmCarve c(ws);
    c.bytes = w.sort.bytes;
    w.nu = c.take<double>(n);
    w.angle = c.take<double>(n);
    w.emin = c.take<int32_t>(n);
    w.emax = c.take<int32_t>(n);
    w.item1 = c.take<int32_t>(n);
    w.bytes = c.bytes;
    return w;
}

constexpr int64_t kMaxTopoFaces = (((int64_t)1 << 31) - 1) / 3;   // 3 F items are sorted: 3 F < 2^31

}  // namespace

extern "C" {

int64_t hm_mesh_topology_workspace_bytes(int64_t n_faces) {
    if (n_faces < 0 || n_faces > kMaxTopoFaces)
        return hm_fail(HM_ERR_INVALID, "hm_mesh_topology_workspace_bytes: 3 * n_faces must be in [0, 2^31)");
    return mt_layout(nullptr, n_faces).bytes;
}

int hm_mesh_topology_build(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts,
                           double *vertex_normals, double *edge_normals, int64_t *counts, void *workspace,
                           int64_t workspace_bytes, int32_t *status, void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_topology_build")) return rc;
    HM_CHECK_ARG(n_faces >= 1 && n_faces <= kMaxTopoFaces,
                 "hm_mesh_topology_build: n_faces must be >= 1 and 3 * n_faces < 2^31");
    HM_CHECK_ARG((verts || n_verts == 0) && (vertex_normals || n_verts == 0) && edge_normals && counts && workspace &&
                     status,
                 "hm_mesh_topology_build: NULL pointer");
    HM_CHECK_ARG(workspace_bytes >= hm_mesh_topology_workspace_bytes(n_faces),
                 "hm_mesh_topology_build: workspace too small");
    const MtWs w = mt_layout(workspace, n_faces);
    const int64_t n = n_faces * 3;
    hipStream_t st = as_stream(stream);
    int key_bits = 1;   // the bit length of n_verts - 1
    while (key_bits < 31 && ((int64_t)1 << key_bits) < n_verts) ++key_bits;
    hm_zero_u32_async(vertex_normals, n_verts * 6, st);
    hm_zero_u32_async(counts, 6, st);
    hipLaunchKernelGGL(mt_face_kernel, dim3(hm_grid(n_faces, kNT)), dim3(kNT), 0, st, verts, faces, n_faces, n_verts,
                       w.nu, w.angle, w.sort.key, w.emin, w.emax, status);
    // the corners by vertex
    if (int rc = hm_sort_pairs_i32(w.sort.key, n, key_bits, w.sort.keys_sorted, w.sort.perm, w.sort.sort_ws,
                                   w.sort.sort_bytes, stream))
        return rc;
    hipLaunchKernelGGL(mt_vertex_kernel, dim3(hm_grid(n, kNT)), dim3(kNT), 0, st,
                       static_cast<const int32_t *>(w.sort.keys_sorted), static_cast<const int64_t *>(w.sort.perm), n,
                       n_verts, static_cast<const double *>(w.nu), static_cast<const double *>(w.angle),
                       vertex_normals);
    // the half-edges by (min, max): stable by max, then stable by min
    if (int rc = hm_sort_pairs_i32(w.emax, n, key_bits, w.sort.keys_sorted, w.sort.perm, w.sort.sort_ws,
                                   w.sort.sort_bytes, stream))
        return rc;
    hipLaunchKernelGGL(mt_regather_kernel, dim3(hm_grid(n, kNT)), dim3(kNT), 0, st,
                       static_cast<const int64_t *>(w.sort.perm), n, static_cast<const int32_t *>(w.emin), w.item1,
                       w.sort.key);
    if (int rc = hm_sort_pairs_i32(w.sort.key, n, key_bits, w.sort.keys_sorted, w.sort.perm, w.sort.sort_ws,
                                   w.sort.sort_bytes, stream))
        return rc;
    hipLaunchKernelGGL(mt_edge_kernel, dim3(hm_grid(n, kNT)), dim3(kNT), 0, st,
                       static_cast<const int32_t *>(w.sort.keys_sorted), static_cast<const int64_t *>(w.sort.perm),
                       static_cast<const int32_t *>(w.item1), static_cast<const int32_t *>(w.emax), faces, n,
                       static_cast<const double *>(w.nu), edge_normals,
                       reinterpret_cast<unsigned long long *>(counts));
    HM_CHECK_LAUNCH("hm_mesh_topology_build");
    return HM_OK;
}

int hm_mesh_sign(const float *query, int64_t m, const int32_t *face, const int32_t *feature, const float *point,
                 const float *d2, const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts,
                 const double *vertex_normals, const double *edge_normals, float *sd, int32_t *sign, void *stream) {
    HM_CHECK_ARG(m >= 0 && m < ((int64_t)1 << 31), "hm_mesh_sign: m must be in [0, 2^31)");
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_sign")) return rc;
    HM_CHECK_ARG(n_faces >= 1 && n_faces <= kMaxTopoFaces, "hm_mesh_sign: n_faces must be >= 1 and 3 * n_faces < 2^31");
    if (m == 0) return HM_OK;
    HM_CHECK_ARG(query && face && feature && point && d2 && verts && vertex_normals && edge_normals && sd,
                 "hm_mesh_sign: NULL pointer");
    hipLaunchKernelGGL(mt_sign_kernel, dim3(hm_grid(m, kNT)), dim3(kNT), 0, as_stream(stream), query, m, face, feature,
                       point, d2, verts, faces, n_faces, n_verts, vertex_normals, edge_normals, sd, sign);
    HM_CHECK_LAUNCH("hm_mesh_sign");
    return HM_OK;
}

}  // extern "C"
