// hm_nn_dev.h - the uniform grid of the Chamfer evaluation as hm_nn.hip (build, nearest neighbour) and
// hm_nn_radius.hip (greedy radius thinning) share it: the grid record, the cell function and the host-side check.
// Both files put a coordinate into its cell with the same fp32 operations, so what one builds the other can scan.
#pragma once
#include <math.h>

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
