// hm_mesh_simplify.hip - vertex clustering of a triangle mesh on the uniform grid of hm_nn_dev.h (DESIGN.md "Mesh
// simplification"; tests/mesh_simplify_cases.py restates it in numpy).  Driver: ops.mesh_simplify.
//
//   hm_mesh_simplify_keys       ms_mark      per face: range check, used[v] = 1 for its three vertices
//                               ms_key       per vertex: the key of its cell (nn_cell), or the sentinel `cells` when unused
//                               hm_sort_pairs_i32 (stable)  ->  a cluster is one run, its members in ascending vertex id
//                               ms_head      head[i] = 1 at the first position of every run below the sentinel
//   hm_mesh_simplify_clusters   one wave per run: lane l takes the run's members l, l + 64, ... in order, the lanes'
//                               sums meet in the wave butterfly; mean, point-normal quadric, 3x3 solve, clamp, normal
//   hm_mesh_simplify_face_flags per face: 1 when its three clusters differ
//   hm_mesh_simplify_dedupe     ms_compact   the kept faces' cluster triples, rotated to smallest-first, in face order
//                               three stable sorts by third, second and first id (the permutations composed in between)
//                               ms_first     a triple equal to its predecessor in that order is a repeat; the others
//                                            are kept and mark their clusters
//   hm_mesh_simplify_emit       the marked clusters' representatives, the kept triples renumbered, the vertex map
//
// Every sum is fp64 over the fp32 inputs in an order fixed by the run alone (no atomics), and a result is rounded to
// fp32 once: two calls give the same bits.  The prefix sums between the entry points are the caller's.  A face index
// outside [0, n_verts) is never dereferenced (hm_face_ids): hm_mesh_simplify_keys reports it in the status word and
// the later launches leave the face out.
#include "hm_block_dev.h"
#include "hm_nn_dev.h"

namespace {

constexpr int kMT = 256;            // threads per workgroup
constexpr int kMWaves = kMT / 64;   // runs per workgroup of the cluster kernel

__global__ __launch_bounds__(kMT) void ms_mark_kernel(const int32_t *__restrict__ faces, int64_t n_faces,
                                                      int64_t n_verts, int32_t *__restrict__ used, int32_t *status) {
    const int64_t f = (int64_t)blockIdx.x * kMT + threadIdx.x;
    if (f >= n_faces) return;
    int32_t v[3];
    if (!hm_face_ids(faces, f, n_verts, v, status)) return;
#pragma unroll
    for (int m = 0; m < 3; ++m) used[v[m]] = 1;
}

__global__ __launch_bounds__(kMT) void ms_key_kernel(const float *__restrict__ verts,
                                                     const int32_t *__restrict__ used, int64_t n_verts, NnGrid G,
                                                     int32_t sentinel, int32_t *__restrict__ key) {
    const int64_t v = (int64_t)blockIdx.x * kMT + threadIdx.x;
    if (v >= n_verts) return;
    int32_t k = sentinel;
    if (used[v]) {
        int64_t c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = nn_cell(verts[v * 3 + a], G.lo[a], G.h, G.g[a]);
        k = (int32_t)((c[0] * G.g[1] + c[1]) * G.g[2] + c[2]);
    }
    key[v] = k;
}

__global__ __launch_bounds__(kMT) void ms_head_kernel(const int32_t *__restrict__ keys_sorted, int64_t n_verts,
                                                      int32_t sentinel, int32_t *__restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * kMT + threadIdx.x;
    if (i >= n_verts) return;
    const int32_t k = keys_sorted[i];
    head[i] = (k < sentinel && (i == 0 || keys_sorted[i - 1] != k)) ? 1 : 0;
}

// n / |n| in fp64, or 0 for a zero or non-finite normal
__device__ __forceinline__ void ms_unit_normal(const float *__restrict__ normals, int64_t v, double (&n)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) n[a] = (double)normals[v * 3 + a];
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const bool ok = len > 0.0 && isfinite(len);
#pragma unroll
    for (int a = 0; a < 3; ++a) n[a] = ok ? n[a] / len : 0.0;
}

// One wave per run [start[c], start[c + 1]) of the sorted vertices.  QUADRIC: x = m + A^-1 b with A = sum n n^T +
// reg k I (symmetric positive definite, condition <= (1 + reg) / reg: the adjugate solve is enough), clamped per axis
// to the cell's box widened to hold m.
template <bool QUADRIC>
__global__ __launch_bounds__(kMT) void ms_cluster_kernel(const float *__restrict__ verts,
                                                         const float *__restrict__ normals, int64_t n_verts,
                                                         const int32_t *__restrict__ keys_sorted,
                                                         const int64_t *__restrict__ perm,
                                                         const int64_t *__restrict__ start, int64_t n_clusters,
                                                         NnGrid G, double reg, float *__restrict__ rep,
                                                         float *__restrict__ normals_out,
                                                         int32_t *__restrict__ cluster_of) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * kMWaves + (threadIdx.x >> 6);
    if (c >= n_clusters) return;                       // wave-uniform
    const int64_t beg = start[c], end = start[c + 1];
    if (beg < 0 || end > n_verts || beg >= end) return;
    double sp[3] = {0.0, 0.0, 0.0}, sn[3] = {0.0, 0.0, 0.0};
    for (int64_t i = beg + lane; i < end; i += 64) {
        const int64_t v = perm[i];
        cluster_of[v] = (int32_t)c;
#pragma unroll
        for (int a = 0; a < 3; ++a) sp[a] += (double)verts[v * 3 + a];
        if (normals) {
            double n[3];
            ms_unit_normal(normals, v, n);
#pragma unroll
            for (int a = 0; a < 3; ++a) sn[a] += n[a];
        }
    }
    const double k = (double)(end - beg);
    double m[3], x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        m[a] = hm_wave_reduce(sp[a], HmSum()) / k;
        sn[a] = hm_wave_reduce(sn[a], HmSum());
        x[a] = m[a];
    }
    if (QUADRIC) {
        double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};   // A: xx xy xz yy yz zz
        for (int64_t i = beg + lane; i < end; i += 64) {
            const int64_t v = perm[i];
            double n[3];
            ms_unit_normal(normals, v, n);
            double d = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) d += n[a] * ((double)verts[v * 3 + a] - m[a]);
            int q = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                b[a] += n[a] * d;
#pragma unroll
                for (int e = a; e < 3; ++e, ++q) A[q] += n[a] * n[e];
            }
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) A[q] = hm_wave_reduce(A[q], HmSum());
#pragma unroll
        for (int a = 0; a < 3; ++a) b[a] = hm_wave_reduce(b[a], HmSum());
        const double rk = reg * k;
        const double a00 = A[0] + rk, a01 = A[1], a02 = A[2], a11 = A[3] + rk, a12 = A[4], a22 = A[5] + rk;
        const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
        const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
        const double det = (a00 * c00 + a01 * c01) + a02 * c02;
        x[0] = m[0] + ((c00 * b[0] + c01 * b[1]) + c02 * b[2]) / det;
        x[1] = m[1] + ((c01 * b[0] + c11 * b[1]) + c12 * b[2]) / det;
        x[2] = m[2] + ((c02 * b[0] + c12 * b[1]) + c22 * b[2]) / det;
        const int32_t key = keys_sorted[beg];
        const int32_t cell[3] = {key / G.g[2] / G.g[1], key / G.g[2] % G.g[1], key % G.g[2]};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double blo = (double)G.lo[a] + (double)cell[a] * (double)G.h, bhi = blo + (double)G.h;
            x[a] = fmin(fmax(x[a], fmin(blo, m[a])), fmax(bhi, m[a]));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) rep[c * 3 + a] = (float)x[a];
        if (normals) {
            const double len = sqrt((sn[0] * sn[0] + sn[1] * sn[1]) + sn[2] * sn[2]);
#pragma unroll
            for (int a = 0; a < 3; ++a) normals_out[c * 3 + a] = len > 0.0 ? (float)(sn[a] / len) : 0.0f;
        }
    }
}

// the clusters of face f's vertices; false for a face out of range, of an unclustered vertex or with two equal clusters
__device__ __forceinline__ bool ms_face_clusters(const int32_t *__restrict__ faces, int64_t f, int64_t n_verts,
                                                 const int32_t *__restrict__ cluster_of, int64_t n_clusters,
                                                 int32_t (&c)[3]) {
    int32_t v[3];
    if (!hm_face_ids(faces, f, n_verts, v)) return false;
#pragma unroll
    for (int m = 0; m < 3; ++m) c[m] = cluster_of[v[m]];
    const bool in = (uint64_t)(int64_t)c[0] < (uint64_t)n_clusters && (uint64_t)(int64_t)c[1] < (uint64_t)n_clusters &&
                    (uint64_t)(int64_t)c[2] < (uint64_t)n_clusters;
    return in && c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
}

__global__ __launch_bounds__(kMT) void ms_face_flags_kernel(const int32_t *__restrict__ faces, int64_t n_faces,
                                                            int64_t n_verts, const int32_t *__restrict__ cluster_of,
                                                            int64_t n_clusters, int32_t *__restrict__ fkeep) {
    const int64_t f = (int64_t)blockIdx.x * kMT + threadIdx.x;
    if (f >= n_faces) return;
    int32_t c[3];
    fkeep[f] = ms_face_clusters(faces, f, n_verts, cluster_of, n_clusters, c) ? 1 : 0;
}

// tri[0..2][o]: the triple of kept face number o = fpre[f], rotated cyclically so that its smallest id comes first
__global__ __launch_bounds__(kMT) void ms_compact_kernel(const int32_t *__restrict__ faces, int64_t n_faces,
                                                         int64_t n_verts, const int32_t *__restrict__ cluster_of,
                                                         int64_t n_clusters, const int32_t *__restrict__ fkeep,
                                                         const int32_t *__restrict__ fpre, int64_t n_tri,
                                                         int32_t *__restrict__ tri) {
    const int64_t f = (int64_t)blockIdx.x * kMT + threadIdx.x;
    if (f >= n_faces || !fkeep[f]) return;
    const int64_t o = fpre[f];
    int32_t c[3];
    if (o < 0 || o >= n_tri || !ms_face_clusters(faces, f, n_verts, cluster_of, n_clusters, c)) return;
    const int r = (c[0] < c[1] && c[0] < c[2]) ? 0 : (c[1] < c[2] ? 1 : 2);
    tri[o] = c[r];
    tri[n_tri + o] = c[(r + 1) % 3];
    tri[2 * n_tri + o] = c[(r + 2) % 3];
}

// order_out[i] = order_in[perm[i]] (perm itself without order_in), key[i] = column[order_out[i]]
__global__ __launch_bounds__(kMT) void ms_next_key_kernel(const int32_t *__restrict__ column,
                                                          const int64_t *__restrict__ order_in,
                                                          const int64_t *__restrict__ perm, int64_t n_tri,
                                                          int64_t *__restrict__ order_out, int32_t *__restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * kMT + threadIdx.x;
    if (i >= n_tri) return;
    int64_t o = perm[i];
    if (order_in) {
        o = order_in[o];
        order_out[i] = o;
    }
    key[i] = column[o];
}

// position i of the order by (first, second, third id; original order among equals): its triple is a repeat when the
// predecessor holds the same one.  The others are kept and mark their clusters (plain stores of 1).
__global__ __launch_bounds__(kMT) void ms_first_kernel(const int32_t *__restrict__ tri,
                                                       const int64_t *__restrict__ order,
                                                       const int64_t *__restrict__ perm, int64_t n_tri,
                                                       int64_t n_clusters, int32_t *__restrict__ tkeep,
                                                       int32_t *__restrict__ cused) {
    const int64_t i = (int64_t)blockIdx.x * kMT + threadIdx.x;
    if (i >= n_tri) return;
    const int64_t o = order[perm[i]];
    int32_t t[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) t[m] = tri[m * n_tri + o];
    bool repeat = false;
    if (i > 0) {
        const int64_t p = order[perm[i - 1]];
        repeat = tri[p] == t[0] && tri[n_tri + p] == t[1] && tri[2 * n_tri + p] == t[2];
    }
    tkeep[o] = repeat ? 0 : 1;
    if (!repeat) {
#pragma unroll
        for (int m = 0; m < 3; ++m)
            if ((uint64_t)(int64_t)t[m] < (uint64_t)n_clusters) cused[t[m]] = 1;
    }
}

__global__ __launch_bounds__(kMT) void ms_emit_clusters_kernel(const float *__restrict__ rep,
                                                               const float *__restrict__ rep_normals,
                                                               int64_t n_clusters, const int32_t *__restrict__ cused,
                                                               const int32_t *__restrict__ cpre, int64_t n_verts_out,
                                                               float *__restrict__ verts_out,
                                                               float *__restrict__ normals_out) {
    const int64_t c = (int64_t)blockIdx.x * kMT + threadIdx.x;
    if (c >= n_clusters || !cused[c]) return;
    const int64_t o = cpre[c];
    if (o < 0 || o >= n_verts_out) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        verts_out[o * 3 + a] = rep[c * 3 + a];
        if (rep_normals) normals_out[o * 3 + a] = rep_normals[c * 3 + a];
    }
}

__global__ __launch_bounds__(kMT) void ms_emit_faces_kernel(const int32_t *__restrict__ tri, int64_t n_tri,
                                                            const int32_t *__restrict__ tkeep,
                                                            const int32_t *__restrict__ tpre, int64_t n_faces_out,
                                                            const int32_t *__restrict__ cpre, int64_t n_clusters,
                                                            int32_t *__restrict__ faces_out) {
    const int64_t o = (int64_t)blockIdx.x * kMT + threadIdx.x;
    if (o >= n_tri || !tkeep[o]) return;
    const int64_t r = tpre[o];
    if (r < 0 || r >= n_faces_out) return;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int32_t c = tri[m * n_tri + o];
        faces_out[r * 3 + m] = (uint64_t)(int64_t)c < (uint64_t)n_clusters ? cpre[c] : -1;
    }
}

__global__ __launch_bounds__(kMT) void ms_emit_map_kernel(const int32_t *__restrict__ cluster_of, int64_t n_verts,
                                                          const int32_t *__restrict__ cused,
                                                          const int32_t *__restrict__ cpre, int64_t n_clusters,
                                                          int32_t *__restrict__ vertex_map) {
    const int64_t v = (int64_t)blockIdx.x * kMT + threadIdx.x;
    if (v >= n_verts) return;
    const int32_t c = cluster_of[v];
    vertex_map[v] = ((uint64_t)(int64_t)c < (uint64_t)n_clusters && cused[c]) ? cpre[c] : -1;
}

// smallest b in [1, 31] with 2^b > max_key
int ms_key_bits(int64_t max_key) {
    int bits = 1;
    while (bits < 31 && ((int64_t)1 << bits) <= max_key) ++bits;
    return bits;
}

// [key n i32 | hm_sort_pairs_i32's own workspace]
struct KeysWs {
    int32_t *key;
    void *sort_ws;
    int64_t sort_bytes, bytes;
};

KeysWs keys_layout(void *ws, int64_t n) {
    HmCarve c(ws);
    KeysWs w;
    w.key = c.take<int32_t>(n);
    w.sort_bytes = hm_sort_workspace_bytes(n);
    w.sort_ws = c.take<char>(w.sort_bytes);
    w.bytes = c.bytes;
    return w;
}

// [key n i32 | keys_sorted n i32 | three orders n i64 | hm_sort_pairs_i32's own workspace]
struct DedupeWs {
    int32_t *key, *keys_sorted;
    int64_t *order[3];
    void *sort_ws;
    int64_t sort_bytes, bytes;
};

DedupeWs dedupe_layout(void *ws, int64_t n) {
    HmCarve c(ws);
    DedupeWs w;
    w.key = c.take<int32_t>(n);
    w.keys_sorted = c.take<int32_t>(n);
    for (int i = 0; i < 3; ++i) w.order[i] = c.take<int64_t>(n);
    w.sort_bytes = hm_sort_workspace_bytes(n);
    w.sort_ws = c.take<char>(w.sort_bytes);
    w.bytes = c.bytes;
    return w;
}

}  // namespace

extern "C" {

int64_t hm_mesh_simplify_keys_workspace_bytes(int64_t n_verts) {
    if (n_verts < 0 || n_verts >= ((int64_t)1 << 31))
        return hm_fail(HM_ERR_INVALID, "hm_mesh_simplify_keys_workspace_bytes: n_verts must be in [0, 2^31)");
    return keys_layout(nullptr, n_verts).bytes;
}

int hm_mesh_simplify_keys(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts, const float *lo,
                          float h, const int32_t *g, int32_t *used, int32_t *keys_sorted, int64_t *perm, int32_t *head,
                          void *workspace, int64_t workspace_bytes, int32_t *status, void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_simplify_keys")) return rc;
    NnGrid G;
    int64_t cells;
    if (int rc = nn_grid(lo, h, g, "hm_mesh_simplify_keys", G, cells)) return rc;
    if (n_verts == 0) return HM_OK;
    HM_CHECK_ARG(verts && used && keys_sorted && perm && head && workspace && status && (n_faces == 0 || faces),
                 "hm_mesh_simplify_keys: NULL pointer");
    HM_CHECK_ARG(workspace_bytes >= hm_mesh_simplify_keys_workspace_bytes(n_verts),
                 "hm_mesh_simplify_keys: workspace too small");
    const KeysWs w = keys_layout(workspace, n_verts);
    const int32_t sentinel = (int32_t)cells;      // above every key, and cells < 2^31
    hipStream_t st = as_stream(stream);
    if (n_faces > 0)
        hipLaunchKernelGGL(ms_mark_kernel, dim3(hm_grid(n_faces, kMT)), dim3(kMT), 0, st, faces, n_faces, n_verts, used,
                           status);
    hipLaunchKernelGGL(ms_key_kernel, dim3(hm_grid(n_verts, kMT)), dim3(kMT), 0, st, verts,
                       static_cast<const int32_t *>(used), n_verts, G, sentinel, w.key);
    if (int rc = hm_sort_pairs_i32(w.key, n_verts, ms_key_bits(cells), keys_sorted, perm, w.sort_ws, w.sort_bytes,
                                   stream))
        return rc;
    hipLaunchKernelGGL(ms_head_kernel, dim3(hm_grid(n_verts, kMT)), dim3(kMT), 0, st,
                       static_cast<const int32_t *>(keys_sorted), n_verts, sentinel, head);
    HM_CHECK_LAUNCH("hm_mesh_simplify_keys");
    return HM_OK;
}

int hm_mesh_simplify_clusters(const float *verts, const float *normals, int64_t n_verts, const int32_t *keys_sorted,
                              const int64_t *perm, const int64_t *start, int64_t n_clusters, const float *lo, float h,
                              const int32_t *g, int quadric, double reg, float *rep, float *rep_normals,
                              int32_t *cluster_of, void *stream) {
    if (int rc = hm_check_mesh(0, n_verts, nullptr, "hm_mesh_simplify_clusters")) return rc;
    NnGrid G;
    int64_t cells;
    if (int rc = nn_grid(lo, h, g, "hm_mesh_simplify_clusters", G, cells)) return rc;
    HM_CHECK_ARG(n_clusters >= 0 && n_clusters <= n_verts, "hm_mesh_simplify_clusters: n_clusters must be in [0, n_verts]");
    HM_CHECK_ARG(!quadric || (normals && std::isfinite(reg) && reg > 0.0),
                 "hm_mesh_simplify_clusters: the quadric placement needs normals and a positive finite reg");
    if (n_clusters == 0) return HM_OK;
    HM_CHECK_ARG(verts && keys_sorted && perm && start && rep && cluster_of && (!normals || rep_normals),
                 "hm_mesh_simplify_clusters: NULL pointer");
    hm_bool_dispatch(quadric != 0, [&](auto q) {
        hipLaunchKernelGGL(ms_cluster_kernel<decltype(q)::value>, dim3(hm_grid(n_clusters, kMWaves)), dim3(kMT), 0,
                           as_stream(stream), verts, normals, n_verts, keys_sorted, perm, start, n_clusters, G, reg, rep,
                           rep_normals, cluster_of);
    });
    HM_CHECK_LAUNCH("hm_mesh_simplify_clusters");
    return HM_OK;
}

int hm_mesh_simplify_face_flags(const int32_t *faces, int64_t n_faces, int64_t n_verts, const int32_t *cluster_of,
                                int64_t n_clusters, int32_t *fkeep, void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_simplify_face_flags")) return rc;
    HM_CHECK_ARG(n_clusters >= 0 && n_clusters <= n_verts,
                 "hm_mesh_simplify_face_flags: n_clusters must be in [0, n_verts]");
    if (n_faces == 0) return HM_OK;
    HM_CHECK_ARG(faces && cluster_of && fkeep, "hm_mesh_simplify_face_flags: NULL pointer");
    hipLaunchKernelGGL(ms_face_flags_kernel, dim3(hm_grid(n_faces, kMT)), dim3(kMT), 0, as_stream(stream), faces,
                       n_faces, n_verts, cluster_of, n_clusters, fkeep);
    HM_CHECK_LAUNCH("hm_mesh_simplify_face_flags");
    return HM_OK;
}

int64_t hm_mesh_simplify_dedupe_workspace_bytes(int64_t n_tri) {
    if (n_tri < 0 || n_tri >= ((int64_t)1 << 31))
        return hm_fail(HM_ERR_INVALID, "hm_mesh_simplify_dedupe_workspace_bytes: n_tri must be in [0, 2^31)");
    return dedupe_layout(nullptr, n_tri).bytes;
}

int hm_mesh_simplify_dedupe(const int32_t *faces, int64_t n_faces, int64_t n_verts, const int32_t *cluster_of,
                            int64_t n_clusters, const int32_t *fkeep, const int32_t *fpre, int64_t n_tri, int32_t *tri,
                            int32_t *tkeep, int32_t *cused, void *workspace, int64_t workspace_bytes, void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_simplify_dedupe")) return rc;
    HM_CHECK_ARG(n_clusters >= 0 && n_clusters <= n_verts, "hm_mesh_simplify_dedupe: n_clusters must be in [0, n_verts]");
    HM_CHECK_ARG(n_tri >= 0 && n_tri <= n_faces, "hm_mesh_simplify_dedupe: n_tri must be in [0, n_faces]");
    if (n_tri == 0) return HM_OK;
    HM_CHECK_ARG(faces && cluster_of && fkeep && fpre && tri && tkeep && cused && workspace,
                 "hm_mesh_simplify_dedupe: NULL pointer");
    HM_CHECK_ARG(workspace_bytes >= hm_mesh_simplify_dedupe_workspace_bytes(n_tri),
                 "hm_mesh_simplify_dedupe: workspace too small");
    const DedupeWs w = dedupe_layout(workspace, n_tri);
    const int bits = ms_key_bits(n_clusters - 1);
    const dim3 grid(hm_grid(n_tri, kMT)), block(kMT);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(ms_compact_kernel, dim3(hm_grid(n_faces, kMT)), block, 0, st, faces, n_faces, n_verts, cluster_of,
                       n_clusters, fkeep, fpre, n_tri, tri);
    const int32_t *ctri = tri;
    // by the third id; then by the second in that order; then by the first: order[2] composes the first two sorts
    if (int rc = hm_sort_pairs_i32(ctri + 2 * n_tri, n_tri, bits, w.keys_sorted, w.order[0], w.sort_ws, w.sort_bytes,
                                   stream))
        return rc;
    hipLaunchKernelGGL(ms_next_key_kernel, grid, block, 0, st, ctri + n_tri, static_cast<const int64_t *>(nullptr),
                       static_cast<const int64_t *>(w.order[0]), n_tri, static_cast<int64_t *>(nullptr), w.key);
    if (int rc = hm_sort_pairs_i32(w.key, n_tri, bits, w.keys_sorted, w.order[1], w.sort_ws, w.sort_bytes, stream))
        return rc;
    hipLaunchKernelGGL(ms_next_key_kernel, grid, block, 0, st, ctri, static_cast<const int64_t *>(w.order[0]),
                       static_cast<const int64_t *>(w.order[1]), n_tri, w.order[2], w.key);
    if (int rc = hm_sort_pairs_i32(w.key, n_tri, bits, w.keys_sorted, w.order[1], w.sort_ws, w.sort_bytes, stream))
        return rc;
    hipLaunchKernelGGL(ms_first_kernel, grid, block, 0, st, ctri, static_cast<const int64_t *>(w.order[2]),
                       static_cast<const int64_t *>(w.order[1]), n_tri, n_clusters, tkeep, cused);
    HM_CHECK_LAUNCH("hm_mesh_simplify_dedupe");
    return HM_OK;
}

int hm_mesh_simplify_emit(const float *rep, const float *rep_normals, int64_t n_clusters, const int32_t *cused,
                          const int32_t *cpre, int64_t n_verts_out, const int32_t *tri, int64_t n_tri,
                          const int32_t *tkeep, const int32_t *tpre, int64_t n_faces_out, const int32_t *cluster_of,
                          int64_t n_verts, float *verts_out, float *normals_out, int32_t *faces_out,
                          int32_t *vertex_map, void *stream) {
    if (int rc = hm_check_mesh(n_tri, n_verts, tri, "hm_mesh_simplify_emit")) return rc;
    HM_CHECK_ARG(n_clusters >= 0 && n_clusters <= n_verts && n_verts_out >= 0 && n_verts_out <= n_clusters &&
                     n_faces_out >= 0 && n_faces_out <= n_tri,
                 "hm_mesh_simplify_emit: counts out of range");
    HM_CHECK_ARG(n_clusters == 0 || (cused && cpre), "hm_mesh_simplify_emit: NULL cluster flags");
    HM_CHECK_ARG(n_verts_out == 0 || (rep && verts_out && (!rep_normals || normals_out)),
                 "hm_mesh_simplify_emit: NULL vertex pointer");
    HM_CHECK_ARG(n_faces_out == 0 || (tri && tkeep && tpre && faces_out), "hm_mesh_simplify_emit: NULL face pointer");
    HM_CHECK_ARG(n_verts == 0 || (cluster_of && vertex_map), "hm_mesh_simplify_emit: NULL vertex map");
    hipStream_t st = as_stream(stream);
    if (n_verts_out > 0)
        hipLaunchKernelGGL(ms_emit_clusters_kernel, dim3(hm_grid(n_clusters, kMT)), dim3(kMT), 0, st, rep, rep_normals,
                           n_clusters, cused, cpre, n_verts_out, verts_out, normals_out);
    if (n_faces_out > 0)
        hipLaunchKernelGGL(ms_emit_faces_kernel, dim3(hm_grid(n_tri, kMT)), dim3(kMT), 0, st, tri, n_tri, tkeep, tpre,
                           n_faces_out, cpre, n_clusters, faces_out);
    if (n_verts > 0)
        hipLaunchKernelGGL(ms_emit_map_kernel, dim3(hm_grid(n_verts, kMT)), dim3(kMT), 0, st, cluster_of, n_verts, cused,
                           cpre, n_clusters, vertex_map);
    HM_CHECK_LAUNCH("hm_mesh_simplify_emit");
    return HM_OK;
}

}  // extern "C"
