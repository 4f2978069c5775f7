// hm_block_dev.h - the wave and workgroup primitives of the mesh and evaluation kernels (hm_mesh_dev.h, hm_mesh_sparse,
// hm_mesh_cc, hm_mesh_sample, hm_nn, hm_nn_radius): the 64-lane reduction, the workgroup prefix sum, the fixed-order
// fp64 tree sum, the face-index loader and the grid size.  Integer results do not depend on an order; the fp64 sum
// fixes its order, so two calls give the same bits.
#pragma once
#include "hm_common.h"

// workgroups of `per` items that cover n items
inline unsigned hm_grid(int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); }

// the size check of the mesh entry points: both counts in [0, 2^31), and faces given unless there are none
inline int hm_check_mesh(int64_t n_faces, int64_t n_verts, const void *faces, const char *what) {
    const std::string w(what);
    HM_CHECK_ARG(n_faces >= 0 && n_faces < ((int64_t)1 << 31), w + ": n_faces must be in [0, 2^31)");
    HM_CHECK_ARG(n_verts >= 0 && n_verts < ((int64_t)1 << 31), w + ": n_verts must be in [0, 2^31)");
    HM_CHECK_ARG(n_faces == 0 || faces, w + ": NULL faces");
    return HM_OK;
}

#ifdef __HIPCC__
struct HmSum {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct HmOr {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a | b; }
};
struct HmMin {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return min(a, b); }
};
struct HmMax {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return max(a, b); }
};

// op over the 64 lanes of the wave (butterfly: every lane gets the result)
template <class T, class Op>
__device__ __forceinline__ T hm_wave_reduce(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}

// The inclusive prefix sum of v over the workgroup's T threads (in thread order) and the workgroup total; the exclusive
// one is the result minus v.  wsum: T / 64 words of LDS.  One barrier after the wave totals are written and one after
// they are read: safe to call again at once, in a loop, and beside other LDS use.
template <int T>
__device__ __forceinline__ int32_t hm_block_scan(int32_t v, int32_t *wsum, int32_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    int32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) {
        const int32_t s = wsum[w];
        before += w < wave ? s : 0;
        total += s;
    }
    __syncthreads();
    return before + v;
}

// red[k][t] = thread t's term of row k  ->  red[k][0] = the row's sum, for K fp64 rows at once.  The order is fixed:
// o = T/2 .. 1, red[k][t] += red[k][t + o].
template <int K, int T>
__device__ __forceinline__ void hm_block_tree_sum(double (&red)[K][T]) {
    __syncthreads();
    for (int o = T / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int k = 0; k < K; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        }
        __syncthreads();
    }
}

// the three vertex indices of face f; false when one of them is outside [0, n_verts): such a face is never
// dereferenced.  With a status word (not NULL), its bit 0 is set then.
__device__ __forceinline__ bool hm_face_ids(const int32_t *__restrict__ faces, int64_t f, int64_t n_verts,
                                            int32_t (&v)[3]) {
#pragma unroll
    for (int m = 0; m < 3; ++m) v[m] = faces[f * 3 + m];
    return (uint64_t)(int64_t)v[0] < (uint64_t)n_verts && (uint64_t)(int64_t)v[1] < (uint64_t)n_verts &&
           (uint64_t)(int64_t)v[2] < (uint64_t)n_verts;
}
__device__ __forceinline__ bool hm_face_ids(const int32_t *__restrict__ faces, int64_t f, int64_t n_verts,
                                            int32_t (&v)[3], int32_t *status) {
    const bool ok = hm_face_ids(faces, f, n_verts, v);
    if (!ok) atomicOr(status, 1);
    return ok;
}
#endif
