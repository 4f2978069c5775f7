// hm_mesh_cc.hip - connected components of a welded triangle mesh, per-component areas, surface moments and the
// submesh of one component (reference: evaluation/eval.py's cleanup of every fine mesh - mesh.split(only_watertight=
// False), one area per part, the part at argmax; utils/plots.TriMesh.split and plots._surface_moments restate it on
// the host).
//
//   hm_mesh_cc_labels      cc_init      parent[v] = v
//                          cc_union     per face: union (f0, f1), (f1, f2) - lock-free union-find, see below
//                          cc_flatten   (next launch) label[v] = the root of v = the smallest vertex id of its component
//   hm_mesh_cc_face_stats  per face: fp64 area from the fp32 vertices, used[v] = 1 for its three vertices
//   hm_mesh_cc_sums        cc_key       key[f] = rank of the face's component among the components that own faces
//                          hm_sort_pairs_i32 (stable)  ->  the faces of one component are one run, in face order
//                          cc_segment   one workgroup per component: fixed-order sum of its run, and the run's length
//   hm_mesh_moments        mom_partial  per 4096-face block: the 10 fp64 sums of plots._surface_moments, fixed order
//                          mom_final    one workgroup: the block partials in order -> area, mean, covariance
//   hm_mesh_select_mark    per face of the component: fflag[f] = 1, vflag[its vertices] = 1
//   hm_mesh_select_emit    vertices / normals of the flagged vertices in ascending order, flagged faces in order,
//                          renumbered by the exclusive prefix sums of the flags (np.unique(..., return_inverse=True))
//
// Union-find.  parent[v] <= v at every moment: a root is hooked under a SMALLER root by atomicCAS(parent + hi, hi, lo),
// and path halving only lowers a non-root's parent to one of its ancestors (atomicMin).  Every pointer chase is
// therefore strictly decreasing and finite, a tree's root is its smallest vertex, and the set of trees only ever
// coarsens.  No thread waits for another: no locks, no polled flags, no inter-workgroup barrier; the only retry loop is
// the CAS of the union, continued from the value the CAS returned (< hi).  parent[] is read with relaxed agent-scope
// atomic loads (served by L2, not by the CU's L1), but nothing depends on their freshness: a stale value is an older
// parent, which is a smaller vertex of the same tree, and the CAS decides on the true value.  After a union returns
// its two vertices are in one tree, so one pass over the faces is complete; the flatten is a later launch and reads
// what the kernel boundary made visible.
//
// A face index outside [0, n_verts) is never dereferenced: the face is skipped and bit 0 of the status word is set.
// Floating-point sums use no atomics and a fixed order: two calls give the same bits.  The face-index loader, the tree
// sum, the grid size and the mesh size check are hm_block_dev.h's.
#include "hm_block_dev.h"

namespace {

constexpr int kCT = 256;                 // threads per workgroup
constexpr int kCRounds = 16;             // faces per thread of a moments block
constexpr int kCBlock = kCT * kCRounds;  // 4096 faces per moments block
constexpr int kSegT = 512;               // threads of a segment-sum workgroup
constexpr int kMom = 10;                 // area, 3 first moments, 6 second moments (xx xy xz yy yz zz)

__device__ __forceinline__ int32_t cc_load(const int32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x as far as this thread can see, halving the path on the way (parent[x] only ever decreases)
__device__ __forceinline__ int32_t cc_find(int32_t *parent, int32_t x) {
    for (;;) {
        const int32_t p = cc_load(parent + x);
        if (p == x) return x;
        const int32_t g = cc_load(parent + p);
        if (g != p) atomicMin(parent + x, g);
        x = g;
    }
}

__device__ __forceinline__ void cc_union(int32_t *parent, int32_t a, int32_t b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old;   // hi was hooked by another thread meanwhile: old < hi is its parent
        b = lo;
    }
}

__global__ __launch_bounds__(kCT) void cc_init_kernel(int32_t *__restrict__ parent, int64_t n_verts) {
    const int64_t v = (int64_t)blockIdx.x * kCT + threadIdx.x;
    if (v < n_verts) parent[v] = (int32_t)v;
}

__global__ __launch_bounds__(kCT) void cc_union_kernel(const int32_t *__restrict__ faces, int64_t n_faces,
                                                       int64_t n_verts, int32_t *parent, int32_t *status) {
    const int64_t f = (int64_t)blockIdx.x * kCT + threadIdx.x;
    if (f >= n_faces) return;
    int32_t v[3];
    if (!hm_face_ids(faces, f, n_verts, v, status)) return;
    cc_union(parent, v[0], v[1]);
    cc_union(parent, v[1], v[2]);
}

// the roots never change here and every store writes a vertex' root over one of its ancestors
__global__ __launch_bounds__(kCT) void cc_flatten_kernel(int32_t *parent, int64_t n_verts) {
    const int64_t v = (int64_t)blockIdx.x * kCT + threadIdx.x;
    if (v >= n_verts) return;
    int32_t r = (int32_t)v;
    for (;;) {
        const int32_t p = cc_load(parent + r);
        if (p == r) break;
        r = p;
    }
    if (r != (int32_t)v) __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct Tri {
    double p[3][3];
};

__device__ __forceinline__ Tri cc_tri(const float *__restrict__ verts, const int32_t (&v)[3]) {
    Tri t;
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int i = 0; i < 3; ++i) t.p[m][i] = (double)verts[(int64_t)v[m] * 3 + i];
    return t;
}

// 0.5 |(v1 - v0) x (v2 - v0)| in fp64 (TriMesh.area_faces)
__device__ __forceinline__ double cc_area(const Tri &t) {
    double a[3], b[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a[i] = t.p[1][i] - t.p[0][i];
        b[i] = t.p[2][i] - t.p[0][i];
    }
    const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
    return 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
}

__global__ __launch_bounds__(kCT) void cc_face_stats_kernel(const float *__restrict__ verts,
                                                            const int32_t *__restrict__ faces, int64_t n_faces,
                                                            int64_t n_verts, double *__restrict__ face_area,
                                                            int32_t *__restrict__ used, int32_t *status) {
    const int64_t f = (int64_t)blockIdx.x * kCT + threadIdx.x;
    if (f >= n_faces) return;
    int32_t v[3];
    if (!hm_face_ids(faces, f, n_verts, v, status)) {
        face_area[f] = 0.0;
        return;
    }
    face_area[f] = cc_area(cc_tri(verts, v));
#pragma unroll
    for (int m = 0; m < 3; ++m) used[v[m]] = 1;
}

// key[f] = rank[label[f0]]; a face, label or rank out of range -> key 0 and the status bit
__global__ __launch_bounds__(kCT) void cc_key_kernel(const int32_t *__restrict__ faces, int64_t n_faces,
                                                     int64_t n_verts, const int32_t *__restrict__ label,
                                                     const int32_t *__restrict__ rank, int64_t n_comp,
                                                     int32_t *__restrict__ key, int32_t *status) {
    const int64_t f = (int64_t)blockIdx.x * kCT + threadIdx.x;
    if (f >= n_faces) return;
    int32_t v[3];
    int32_t k = 0;
    if (hm_face_ids(faces, f, n_verts, v, status)) {
        const int32_t l = label[v[0]];
        if ((uint64_t)(int64_t)l < (uint64_t)n_verts) k = rank[l];
        if ((uint64_t)(int64_t)l >= (uint64_t)n_verts || (uint64_t)(int64_t)k >= (uint64_t)n_comp) {
            atomicOr(status, 1);
            k = 0;
        }
    }
    key[f] = k;
}

// first position of keys_sorted[0..n) that is >= c
__device__ __forceinline__ int64_t cc_lower_bound(const int32_t *__restrict__ keys, int64_t n, int32_t c) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// workgroup c sums the run of key c: thread t takes the run's elements t, t + kSegT, ... in order (four independent
// partial sums, so that four gathers are in flight), then the threads' sums meet in a fixed tree
__global__ __launch_bounds__(kSegT) void cc_segment_kernel(const int32_t *__restrict__ keys_sorted,
                                                           const int64_t *__restrict__ perm, int64_t n_faces,
                                                           const double *__restrict__ face_area,
                                                           double *__restrict__ area, int64_t *__restrict__ count) {
    __shared__ double red[1][kSegT];
    __shared__ int64_t range[2];
    const int32_t c = (int32_t)blockIdx.x;
    if (threadIdx.x < 2) range[threadIdx.x] = cc_lower_bound(keys_sorted, n_faces, c + (int32_t)threadIdx.x);
    __syncthreads();
    const int64_t beg = range[0], end = range[1];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t i = beg + threadIdx.x;
    for (; i + 3 * (int64_t)kSegT < end; i += 4 * (int64_t)kSegT) {
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] += face_area[perm[i + u * (int64_t)kSegT]];
    }
    for (int u = 0; i < end; i += kSegT, ++u) s[u] += face_area[perm[i]];
    red[0][threadIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
    hm_block_tree_sum(red);
    if (threadIdx.x == 0) {
        area[c] = red[0][0];
        count[c] = end - beg;
    }
}

// the sums of plots._surface_moments over one block of faces: a, a*s_i, a*(sum_m v_mi v_mj + s_i s_j)
__global__ __launch_bounds__(kCT) void mom_partial_kernel(const float *__restrict__ verts,
                                                          const int32_t *__restrict__ faces, int64_t n_faces,
                                                          int64_t n_verts, double *__restrict__ partial,
                                                          int32_t *status) {
    __shared__ double red[kMom][kCT];
    double acc[kMom];
#pragma unroll
    for (int k = 0; k < kMom; ++k) acc[k] = 0.0;
    const int64_t beg = (int64_t)blockIdx.x * kCBlock;
    for (int r = 0; r < kCRounds; ++r) {
        const int64_t f = beg + (int64_t)r * kCT + threadIdx.x;
        if (f >= n_faces) break;
        int32_t v[3];
        if (!hm_face_ids(faces, f, n_verts, v, status)) continue;
        const Tri t = cc_tri(verts, v);
        const double a = cc_area(t);
        double s[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) s[i] = (t.p[0][i] + t.p[1][i]) + t.p[2][i];
        acc[0] += a;
#pragma unroll
        for (int i = 0; i < 3; ++i) acc[1 + i] += a * s[i];
        int k = 4;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j, ++k) {
                const double vv = (t.p[0][i] * t.p[0][j] + t.p[1][i] * t.p[1][j]) + t.p[2][i] * t.p[2][j];
                acc[k] += a * (vv + s[i] * s[j]);
            }
    }
#pragma unroll
    for (int k = 0; k < kMom; ++k) red[k][threadIdx.x] = acc[k];
    hm_block_tree_sum(red);
    if (threadIdx.x < kMom) partial[(int64_t)blockIdx.x * kMom + threadIdx.x] = red[threadIdx.x][0];
}

// out[0] = area, out[1..3] = mean, out[4..12] = covariance (row-major); 0/0 = NaN mean and covariance without area
__global__ __launch_bounds__(kCT) void mom_final_kernel(const double *__restrict__ partial, int64_t n_blocks,
                                                        double *__restrict__ out) {
    __shared__ double red[kMom][kCT];
    double acc[kMom];
#pragma unroll
    for (int k = 0; k < kMom; ++k) acc[k] = 0.0;
    for (int64_t b = threadIdx.x; b < n_blocks; b += kCT)
#pragma unroll
        for (int k = 0; k < kMom; ++k) acc[k] += partial[b * kMom + k];
#pragma unroll
    for (int k = 0; k < kMom; ++k) red[k][threadIdx.x] = acc[k];
    hm_block_tree_sum(red);
    if (threadIdx.x == 0) {
        const double A = red[0][0];
        double mean[3];
        out[0] = A;
        for (int i = 0; i < 3; ++i) out[1 + i] = mean[i] = red[1 + i][0] / (3.0 * A);
        int k = 4;
        for (int i = 0; i < 3; ++i)
            for (int j = i; j < 3; ++j, ++k) {
                const double c = red[k][0] / (12.0 * A) - mean[i] * mean[j];
                out[4 + i * 3 + j] = c;
                out[4 + j * 3 + i] = c;
            }
    }
}

__global__ __launch_bounds__(kCT) void sel_mark_kernel(const int32_t *__restrict__ faces, int64_t n_faces,
                                                       int64_t n_verts, const int32_t *__restrict__ label,
                                                       int32_t component, int32_t *__restrict__ vflag,
                                                       int32_t *__restrict__ fflag, int32_t *status) {
    const int64_t f = (int64_t)blockIdx.x * kCT + threadIdx.x;
    if (f >= n_faces) return;
    int32_t v[3];
    const bool in = hm_face_ids(faces, f, n_verts, v, status) && label[v[0]] == component;
    fflag[f] = in ? 1 : 0;
    if (in) {
#pragma unroll
        for (int m = 0; m < 3; ++m) vflag[v[m]] = 1;
    }
}

__global__ __launch_bounds__(kCT) void sel_verts_kernel(const float *__restrict__ verts,
                                                        const float *__restrict__ normals, int64_t n_verts,
                                                        const int32_t *__restrict__ vflag,
                                                        const int32_t *__restrict__ vpre, int64_t cap_v,
                                                        float *__restrict__ verts_out, float *__restrict__ normals_out) {
    const int64_t v = (int64_t)blockIdx.x * kCT + threadIdx.x;
    if (v >= n_verts || !vflag[v]) return;
    const int64_t o = vpre[v];
    if (o < 0 || o >= cap_v) return;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        verts_out[o * 3 + i] = verts[v * 3 + i];
        if (normals) normals_out[o * 3 + i] = normals[v * 3 + i];
    }
}

// a flagged face passed sel_mark's range check and flagged its vertices, so vpre of its indices is their new id
__global__ __launch_bounds__(kCT) void sel_faces_kernel(const int32_t *__restrict__ faces, int64_t n_faces,
                                                        int64_t n_verts, const int32_t *__restrict__ vpre,
                                                        const int32_t *__restrict__ fflag,
                                                        const int32_t *__restrict__ fpre, int64_t cap_f,
                                                        int32_t *__restrict__ faces_out) {
    const int64_t f = (int64_t)blockIdx.x * kCT + threadIdx.x;
    if (f >= n_faces || !fflag[f]) return;
    const int64_t o = fpre[f];
    if (o < 0 || o >= cap_f) return;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int32_t v = faces[f * 3 + m];
        faces_out[o * 3 + m] = (uint64_t)(int64_t)v < (uint64_t)n_verts ? vpre[v] : -1;
    }
}

int64_t mom_blocks(int64_t n_faces) { return (n_faces + kCBlock - 1) / kCBlock; }

// the block partials of hm_mesh_moments (one block's worth for an empty mesh)
struct MomWs {
    double *partial;
    int64_t bytes;
};

MomWs mom_layout(void *ws, int64_t n_faces) {
    const int64_t nb = mom_blocks(n_faces);
    HmCarve c(ws);
    MomWs w;
    w.partial = c.take<double>(kMom * (nb > 0 ? nb : 1));
    w.bytes = c.bytes;
    return w;
}

}  // namespace

extern "C" {

int hm_mesh_cc_labels(const int32_t *faces, int64_t n_faces, int64_t n_verts, int32_t *label, int32_t *status,
                      void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_cc_labels")) return rc;
    if (n_verts == 0 && n_faces == 0) return HM_OK;
    HM_CHECK_ARG(status && (n_verts == 0 || label), "hm_mesh_cc_labels: NULL label or status");
    hipStream_t st = as_stream(stream);
    if (n_verts > 0)
        hipLaunchKernelGGL(cc_init_kernel, dim3(hm_grid(n_verts, kCT)), dim3(kCT), 0, st, label, n_verts);
    if (n_faces > 0)
        hipLaunchKernelGGL(cc_union_kernel, dim3(hm_grid(n_faces, kCT)), dim3(kCT), 0, st, faces, n_faces, n_verts,
                           label, status);
    if (n_verts > 0 && n_faces > 0)
        hipLaunchKernelGGL(cc_flatten_kernel, dim3(hm_grid(n_verts, kCT)), dim3(kCT), 0, st, label, n_verts);
    HM_CHECK_LAUNCH("hm_mesh_cc_labels");
    return HM_OK;
}

int hm_mesh_cc_face_stats(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts,
                          double *face_area, int32_t *used, int32_t *status, void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_cc_face_stats")) return rc;
    if (n_faces == 0) return HM_OK;
    HM_CHECK_ARG(verts && face_area && used && status, "hm_mesh_cc_face_stats: NULL pointer");
    hipLaunchKernelGGL(cc_face_stats_kernel, dim3(hm_grid(n_faces, kCT)), dim3(kCT), 0, as_stream(stream), verts, faces,
                       n_faces, n_verts, face_area, used, status);
    HM_CHECK_LAUNCH("hm_mesh_cc_face_stats");
    return HM_OK;
}

int64_t hm_mesh_cc_sums_workspace_bytes(int64_t n_faces) {
    if (n_faces < 0 || n_faces >= ((int64_t)1 << 31))
        return hm_fail(HM_ERR_INVALID, "hm_mesh_cc_sums_workspace_bytes: n_faces must be in [0, 2^31)");
    return hm_keysort_layout(nullptr, n_faces).bytes;
}

int hm_mesh_cc_sums(const int32_t *faces, int64_t n_faces, int64_t n_verts, const int32_t *label, const int32_t *rank,
                    const double *face_area, int64_t n_components, double *area, int64_t *count, void *workspace,
                    int64_t workspace_bytes, int32_t *status, void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_cc_sums")) return rc;
    HM_CHECK_ARG(n_components >= 0 && n_components <= n_verts, "hm_mesh_cc_sums: n_components must be in [0, n_verts]");
    if (n_faces == 0 || n_components == 0) return HM_OK;
    HM_CHECK_ARG(label && rank && face_area && area && count && workspace && status, "hm_mesh_cc_sums: NULL pointer");
    HM_CHECK_ARG(workspace_bytes >= hm_mesh_cc_sums_workspace_bytes(n_faces), "hm_mesh_cc_sums: workspace too small");
    const HmKeySortWs w = hm_keysort_layout(workspace, n_faces);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(cc_key_kernel, dim3(hm_grid(n_faces, kCT)), dim3(kCT), 0, st, faces, n_faces, n_verts, label,
                       rank, n_components, w.key, status);
    int key_bits = 1;
    while (key_bits < 31 && ((int64_t)1 << key_bits) < n_components) ++key_bits;
    if (int rc = hm_sort_pairs_i32(w.key, n_faces, key_bits, w.keys_sorted, w.perm, w.sort_ws, w.sort_bytes, stream))
        return rc;
    hipLaunchKernelGGL(cc_segment_kernel, dim3((unsigned)n_components), dim3(kSegT), 0, st,
                       static_cast<const int32_t *>(w.keys_sorted), static_cast<const int64_t *>(w.perm), n_faces,
                       face_area, area, count);
    HM_CHECK_LAUNCH("hm_mesh_cc_sums");
    return HM_OK;
}

int64_t hm_mesh_moments_workspace_bytes(int64_t n_faces) {
    if (n_faces < 0 || n_faces >= ((int64_t)1 << 31))
        return hm_fail(HM_ERR_INVALID, "hm_mesh_moments_workspace_bytes: n_faces must be in [0, 2^31)");
    return mom_layout(nullptr, n_faces).bytes;
}

int hm_mesh_moments(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts, double *out,
                    void *workspace, int64_t workspace_bytes, int32_t *status, void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_moments")) return rc;
    HM_CHECK_ARG(out && workspace && status && (n_faces == 0 || verts), "hm_mesh_moments: NULL pointer");
    HM_CHECK_ARG(workspace_bytes >= hm_mesh_moments_workspace_bytes(n_faces), "hm_mesh_moments: workspace too small");
    const int64_t nb = mom_blocks(n_faces);
    double *partial = mom_layout(workspace, n_faces).partial;
    hipStream_t st = as_stream(stream);
    if (nb > 0)
        hipLaunchKernelGGL(mom_partial_kernel, dim3((unsigned)nb), dim3(kCT), 0, st, verts, faces, n_faces, n_verts,
                           partial, status);
    hipLaunchKernelGGL(mom_final_kernel, dim3(1), dim3(kCT), 0, st, static_cast<const double *>(partial), nb, out);
    HM_CHECK_LAUNCH("hm_mesh_moments");
    return HM_OK;
}

int hm_mesh_select_mark(const int32_t *faces, int64_t n_faces, int64_t n_verts, const int32_t *label,
                        int32_t component, int32_t *vflag, int32_t *fflag, int32_t *status, void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_select_mark")) return rc;
    if (n_faces == 0) return HM_OK;
    HM_CHECK_ARG(label && vflag && fflag && status, "hm_mesh_select_mark: NULL pointer");
    hipLaunchKernelGGL(sel_mark_kernel, dim3(hm_grid(n_faces, kCT)), dim3(kCT), 0, as_stream(stream), faces, n_faces,
                       n_verts, label, component, vflag, fflag, status);
    HM_CHECK_LAUNCH("hm_mesh_select_mark");
    return HM_OK;
}

int hm_mesh_select_emit(const float *verts, const float *normals, const int32_t *faces, int64_t n_faces,
                        int64_t n_verts, const int32_t *vflag, const int32_t *vpre, const int32_t *fflag,
                        const int32_t *fpre, int64_t n_verts_out, int64_t n_faces_out, float *verts_out,
                        float *normals_out, int32_t *faces_out, void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_select_emit")) return rc;
    HM_CHECK_ARG(n_verts_out >= 0 && n_verts_out <= n_verts && n_faces_out >= 0 && n_faces_out <= n_faces,
                 "hm_mesh_select_emit: output counts out of range");
    HM_CHECK_ARG(n_verts_out == 0 || (verts && vflag && vpre && verts_out && (!normals || normals_out)),
                 "hm_mesh_select_emit: NULL vertex pointer");
    HM_CHECK_ARG(n_faces_out == 0 || (vpre && fflag && fpre && faces_out), "hm_mesh_select_emit: NULL face pointer");
    hipStream_t st = as_stream(stream);
    if (n_verts_out > 0)
        hipLaunchKernelGGL(sel_verts_kernel, dim3(hm_grid(n_verts, kCT)), dim3(kCT), 0, st, verts, normals, n_verts,
                           vflag, vpre, n_verts_out, verts_out, normals_out);
    if (n_faces_out > 0)
        hipLaunchKernelGGL(sel_faces_kernel, dim3(hm_grid(n_faces, kCT)), dim3(kCT), 0, st, faces, n_faces, n_verts,
                           vpre, fflag, fpre, n_faces_out, faces_out);
    HM_CHECK_LAUNCH("hm_mesh_select_emit");
    return HM_OK;
}

}  // extern "C"
