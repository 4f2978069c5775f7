// hm_dtu_filter.hip - the per-point filters of the reference's DTU evaluation (evaluation/dtu_eval; contract:
// include/hashmod.h): inside the padded bounding box, inside the scan's observation mask, above the ground plane.
// One byte of flags per point, one lane per point.  The arithmetic is fp64 on the fp32 coordinates, every operation
// rounded once (__dadd_rn and friends: no contraction whatever the build flags say), so the numpy restatement
// (tests/dtu_cases.flags_ref) gives the same bits.  A grid index is compared with the volume's shape as a double,
// BEFORE it becomes an integer: a NaN, an infinity or a value beyond int32 fails the comparison and nothing is read.
#include <math.h>

#include "hm_common.h"

namespace {

constexpr int kFT = 256;

struct DtuParams {
    double lo[3];      // BB0 - patch      (inclusive)
    double hi[3];      // BB1 + 2*patch    (exclusive)
    double bb0[3];
    double res;
    double plane[4];
    int64_t shape[3];
};

// rint((p - bb0) / res) when it is an index of the axis, else -1
__device__ __forceinline__ int64_t dtu_index(double p, double bb0, double res, int64_t extent) {
    const double k = rint(__ddiv_rn(__dsub_rn(p, bb0), res));   // half to even, as np.around
    return (k >= 0.0 && k < (double)extent) ? (int64_t)k : -1;
}

__global__ __launch_bounds__(kFT) void dtu_flags_kernel(const float *__restrict__ pts, int64_t n,
                                                        const uint8_t *__restrict__ mask, DtuParams P,
                                                        uint8_t *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * kFT + threadIdx.x;
    if (i >= n) return;
    const float fx = pts[i * 3], fy = pts[i * 3 + 1], fz = pts[i * 3 + 2];
    uint8_t f = 0;
    if (isfinite(fx) && isfinite(fy) && isfinite(fz)) {
        const double x = fx, y = fy, z = fz;
        if (x >= P.lo[0] && y >= P.lo[1] && z >= P.lo[2] && x < P.hi[0] && y < P.hi[1] && z < P.hi[2]) f |= 1;
        const int64_t kx = dtu_index(x, P.bb0[0], P.res, P.shape[0]), ky = dtu_index(y, P.bb0[1], P.res, P.shape[1]),
                      kz = dtu_index(z, P.bb0[2], P.res, P.shape[2]);
        if (kx >= 0 && ky >= 0 && kz >= 0 && mask[(kx * P.shape[1] + ky) * P.shape[2] + kz] != 0) f |= 2;
        const double v = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(P.plane[0], x), __dmul_rn(P.plane[1], y)),
                                             __dmul_rn(P.plane[2], z)), P.plane[3]);
        if (v > 0.0) f |= 4;
    }
    flags[i] = f;
}

}  // namespace

extern "C" int hm_dtu_point_flags(const float *points, int64_t n, const uint8_t *mask, const int64_t *shape,
                                  const double *params, uint8_t *flags, void *stream) {
    HM_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "hm_dtu_point_flags: n must be in [0, 2^31)");
    HM_CHECK_ARG(shape && params, "hm_dtu_point_flags: NULL shape or params");
    DtuParams P;
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        HM_CHECK_ARG(shape[a] >= 1 && shape[a] < ((int64_t)1 << 31), "hm_dtu_point_flags: mask extents must be in [1, 2^31)");
        HM_CHECK_ARG(cells <= (((int64_t)1 << 62) / shape[a]), "hm_dtu_point_flags: the mask volume is too large");
        cells *= shape[a];
        P.shape[a] = shape[a];
        P.lo[a] = params[a];
        P.hi[a] = params[3 + a];
        P.bb0[a] = params[6 + a];
    }
    P.res = params[9];
    for (int a = 0; a < 4; ++a) P.plane[a] = params[10 + a];
    bool finite = true;
    for (int a = 0; a < 14; ++a) finite = finite && std::isfinite(params[a]);
    HM_CHECK_ARG(finite && P.res > 0.0, "hm_dtu_point_flags: the box, res and the plane must be finite and res > 0");
    if (n == 0) return HM_OK;
    HM_CHECK_ARG(points && mask && flags, "hm_dtu_point_flags: NULL pointer");
    hipLaunchKernelGGL(dtu_flags_kernel, dim3((unsigned)((n + kFT - 1) / kFT)), dim3(kFT), 0, as_stream(stream), points,
                       n, mask, P, flags);
    HM_CHECK_LAUNCH("hm_dtu_point_flags");
    return HM_OK;
}
