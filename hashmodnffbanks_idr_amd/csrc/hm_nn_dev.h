// hm_nn_dev.h - the uniform grid of the Chamfer evaluation as hm_nn.hip (build, nearest neighbour), hm_nn_radius.hip
// (greedy radius thinning) and hm_mesh_dist.hip (point-to-mesh distance) share it: the grid record, the cell function,
// the host-side check, and - for the two box searches - the key and cell-table kernels and the checked cell faces of
// the stopping rule.  All files put a coordinate into its cell with the same fp32 operations, so what one builds the
// other can scan.
#pragma once
#include <math.h>

#include "hm_block_dev.h"
#include "hm_common.h"

constexpr int kNT = 256;      // threads of the elementwise kernels

struct NnGrid {
    float lo[3];
    float h;
    int32_t g[3];
    int32_t pad_;
};

// clamp(floor((p - lo) / h), 0, g - 1) with every operation rounded once; monotone non-decreasing in p.  g <= 2^30.
__device__ __forceinline__ int32_t nn_cell(float p, float lo, float h, int32_t g) {
    const float t = floorf(__fdiv_rn(__fsub_rn(p, lo), h));
    const int32_t c = (int32_t)fminf(fmaxf(t, 0.0f), 1073741824.0f);   // NaN -> 0
    return c < g - 1 ? c : g - 1;
}

__device__ __forceinline__ bool nn_finite3(float x, float y, float z) {
    return isfinite(x) && isfinite(y) && isfinite(z);
}

inline int nn_grid(const float *lo, float h, const int32_t *g, const char *what, NnGrid &G, int64_t &cells) {
    const std::string w(what);
    HM_CHECK_ARG(lo && g, w + ": NULL grid");
    HM_CHECK_ARG(std::isfinite(lo[0]) && std::isfinite(lo[1]) && std::isfinite(lo[2]) && std::isfinite(h) && h > 0.0f,
                 w + ": the grid origin must be finite and the cell edge finite and positive");
    cells = 1;
    for (int a = 0; a < 3; ++a) {
        HM_CHECK_ARG(g[a] >= 1 && g[a] <= (1 << 30), w + ": grid dimensions must be in [1, 2^30]");
        cells *= g[a];
        HM_CHECK_ARG(cells < ((int64_t)1 << 31), w + ": the grid must have fewer than 2^31 cells");
        G.lo[a] = lo[a];
        G.g[a] = g[a];
    }
    G.h = h;
    G.pad_ = 0;
    return HM_OK;
}

#ifdef __HIPCC__
static __global__ __launch_bounds__(kNT) void nn_key_kernel(const float *__restrict__ p, int64_t n, NnGrid G,
                                                            int32_t *__restrict__ key, int32_t *status, int32_t bit) {
    const int64_t i = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (i >= n) return;
    const float x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
    if (!nn_finite3(x, y, z)) {
        atomicOr(status, bit);
        key[i] = 0;
        return;
    }
    const int32_t cx = nn_cell(x, G.lo[0], G.h, G.g[0]), cy = nn_cell(y, G.lo[1], G.h, G.g[1]),
                  cz = nn_cell(z, G.lo[2], G.h, G.g[2]);
    key[i] = (cx * G.g[1] + cy) * G.g[2] + cz;
}

// cell_start[c] for c in [0, cells]: the first position of keys_sorted[0..n) that is >= c (n for c == cells)
static __global__ __launch_bounds__(kNT) void nn_cell_start_kernel(const int32_t *__restrict__ keys_sorted,
                                                                   int64_t n, int64_t cells,
                                                                   int32_t *__restrict__ cell_start) {
    const int64_t c = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (c > cells) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)keys_sorted[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    cell_start[c] = (int32_t)lo;
}

// THE STOPPING RULE.  A lane is finished when its best d2 is strictly below b2 = min over the box's faces that have
// cells beyond them of fl(fl(|q - F|)^2), F the face's coordinate as found here.  Argument: nn_cell is a composition
// of monotone steps (fp32 subtraction, division by h > 0, floor, clamp), so it is monotone in p.  nn_face_low returns
// an F that it has CHECKED to satisfy nn_cell(F) >= k; hence every point whose cell is < k - every point beyond the
// low face of a box that starts at cell k - has p < F, whatever the rounding of the cell assignment did, and that
// includes a point lying exactly on the face lo + k*h (it is wherever nn_cell put it, and F is on the same side).
// For such a point and q >= F, rounding being monotone too: fl(q - p) >= fl(q - F) >= 0, fl(dx*dx) >= fl(fl(q - F)^2),
// and adding the non-negative fl(dy*dy), fl(dz*dz) never rounds below the first term.  So the point's d2 as the
// kernel computes it is >= b2 > best: it is neither a better minimum nor a tie.  (q < F gives the bound 0, which
// finishes nothing.)  The starting guess lo + k*h is nudged by doubling steps of a few ulp until the check holds;
// if it never does the face is put at infinity, the bound is 0 and the search runs on until the box covers the grid.
__device__ __forceinline__ float nn_face_low(float lo, float h, int32_t g, int32_t k) {
    float F = __fadd_rn(lo, __fmul_rn((float)k, h));
    float step = fmaxf(fmaxf(fabsf(F), fabsf(lo)), h) * 2.3841858e-7f;
    for (int it = 0; it < 48 && nn_cell(F, lo, h, g) < k; ++it) {
        F = __fadd_rn(F, step);
        step = __fmul_rn(step, 2.0f);
    }
    return nn_cell(F, lo, h, g) >= k ? F : INFINITY;
}
// the mirror image: an F with nn_cell(F) <= k, so that every point whose cell is > k has p > F
__device__ __forceinline__ float nn_face_high(float lo, float h, int32_t g, int32_t k) {
    float F = __fadd_rn(lo, __fmul_rn((float)k + 1.0f, h));
    float step = fmaxf(fmaxf(fabsf(F), fabsf(lo)), h) * 2.3841858e-7f;
    for (int it = 0; it < 48 && nn_cell(F, lo, h, g) > k; ++it) {
        F = __fsub_rn(F, step);
        step = __fmul_rn(step, 2.0f);
    }
    return nn_cell(F, lo, h, g) <= k ? F : -INFINITY;
}

// keys of the n rows of p, sorted: w.keys_sorted, w.perm
static inline int nn_sorted_keys(const float *p, int64_t n, const NnGrid &G, int64_t cells, const HmKeySortWs &w,
                                 int32_t *status, int32_t bit, void *stream) {
    hipLaunchKernelGGL(nn_key_kernel, dim3(hm_grid(n, kNT)), dim3(kNT), 0, as_stream(stream), p, n, G, w.key, status,
                       bit);
    int key_bits = 1;
    while (key_bits < 31 && ((int64_t)1 << key_bits) < cells) ++key_bits;
    return hm_sort_pairs_i32(w.key, n, key_bits, w.keys_sorted, w.perm, w.sort_ws, w.sort_bytes, stream);
}
#endif
