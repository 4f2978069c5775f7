// hm_mesh_sample.hip - deterministic upsampling of every triangle to a point density: the first step of the
// reference's DTU Chamfer evaluation (evaluation/dtu_eval), restated in include/hashmod.h.  All of the rule is fp64
// with every operation rounded once (the build passes -ffp-contract=off), so a numpy restatement gives the same
// counts and the same fp32 points.
//
//   hm_mesh_sample_count  one wave per face, lanes over the rows i: count[f], rows[f] = n1 + 1
//   hm_mesh_sample_emit   one wave per face and per kRowsPerWave rows: the rows' counts 64 at a time, a wave prefix
//                         sum, then the lanes take the block's SAMPLES (not its rows) round robin - a large face costs
//                         samples / 64 steps, and a face of more than kRowsPerWave rows is shared by several waves
//
// Both kernels get the number of samples of a row from ms_row_count, which evaluates the rule's own predicate
// fl(u + v) < 1: v grows with j, so the kept j of a row are 0 .. count - 1 and the count is found from an estimate
// corrected by the predicate.  A sample's position is prefix[f] + the counts of the rows before it + j: no atomics.
#include <math.h>

#include "hm_block_dev.h"

namespace {

constexpr int kRowsPerWave = 1024;
constexpr int64_t kTooMany = (int64_t)1 << 40;   // the count of a face whose n1*n2 is beyond 2^33

struct MsFace {
    double a[3], v1[3], v2[3];
    double n1, n2;   // integers >= 1 when the face has samples, else 0
};

// false when a face index is outside [0, n_verts) (status bit 0); F.n1 = 0 for a face without samples, -1 for too many
__device__ __forceinline__ bool ms_face(const float *__restrict__ verts, const int32_t *__restrict__ faces, int64_t f,
                                        int64_t n_verts, double density, MsFace &F, int32_t *status) {
    int32_t id[3];
    F.n1 = F.n2 = 0.0;
    if (!hm_face_ids(faces, f, n_verts, id)) {
        if (status) atomicOr(status, 1);   // only one lane of a wave reports
        return false;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        F.a[i] = (double)verts[(int64_t)id[0] * 3 + i];
        F.v1[i] = __dsub_rn((double)verts[(int64_t)id[1] * 3 + i], F.a[i]);
        F.v2[i] = __dsub_rn((double)verts[(int64_t)id[2] * 3 + i], F.a[i]);
    }
    const double *p = F.v1, *q = F.v2;
    const double l1 = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(p[0], p[0]), __dmul_rn(p[1], p[1])), __dmul_rn(p[2], p[2])));
    const double l2 = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(q[0], q[0]), __dmul_rn(q[1], q[1])), __dmul_rn(q[2], q[2])));
    const double cx = __dsub_rn(__dmul_rn(p[1], q[2]), __dmul_rn(p[2], q[1]));
    const double cy = __dsub_rn(__dmul_rn(p[2], q[0]), __dmul_rn(p[0], q[2]));
    const double cz = __dsub_rn(__dmul_rn(p[0], q[1]), __dmul_rn(p[1], q[0]));
    const double A2 = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(cx, cx), __dmul_rn(cy, cy)), __dmul_rn(cz, cz)));
    if (!(A2 > 0.0)) return true;
    const double thr = __dmul_rn(density, __dsqrt_rn(__ddiv_rn(__dmul_rn(l1, l2), A2)));
    const double n1 = floor(__ddiv_rn(l1, thr)), n2 = floor(__ddiv_rn(l2, thr));
    if (!(n1 >= 1.0 && n2 >= 1.0)) return true;
    if (!(n1 * n2 <= 8589934592.0)) {   // 2^33; also inf
        F.n1 = -1.0;
        return true;
    }
    F.n1 = n1;
    F.n2 = n2;
    return true;
}

__device__ __forceinline__ bool ms_keep(double u, int64_t j, double n2) {
    return __dadd_rn(u, __ddiv_rn((double)j + 0.5, n2)) < 1.0;
}

// the number of kept j in 0..n2 of row i: the predicate is monotone in j, so they are 0 .. count - 1
__device__ __forceinline__ int64_t ms_row_count(int64_t i, double n1, double n2) {
    const double u = __ddiv_rn((double)i + 0.5, n1);
    const int64_t n2i = (int64_t)n2;
    const double e = floor((1.0 - u) * n2 - 0.5);
    int64_t j = e < -1.0 ? -1 : (e > n2 ? n2i : (int64_t)e);   // estimate of the last kept j
    while (j + 1 <= n2i && ms_keep(u, j + 1, n2)) ++j;
    while (j >= 0 && !ms_keep(u, j, n2)) --j;
    return j + 1;
}

__global__ __launch_bounds__(64) void ms_count_kernel(const float *__restrict__ verts,
                                                      const int32_t *__restrict__ faces, int64_t n_verts,
                                                      double density, int64_t *__restrict__ count,
                                                      int32_t *__restrict__ rows, int32_t *status) {
    const int64_t f = blockIdx.x;
    const int lane = threadIdx.x;
    MsFace F;
    ms_face(verts, faces, f, n_verts, density, F, lane == 0 ? status : nullptr);
    int64_t c = 0;
    if (F.n1 >= 1.0) {
        const int64_t n1i = (int64_t)F.n1;
        for (int64_t i = lane; i <= n1i; i += 64) c += ms_row_count(i, F.n1, F.n2);
    }
    c = hm_wave_reduce(c, HmSum{});
    if (lane == 0) {
        count[f] = F.n1 < 0.0 ? kTooMany : c;
        rows[f] = F.n1 >= 1.0 ? (int32_t)fmin(F.n1 + 1.0, 2147483647.0) : 0;
    }
}

__global__ __launch_bounds__(64) void ms_emit_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                     int64_t n_verts, double density,
                                                     const int64_t *__restrict__ prefix, int64_t n_samples,
                                                     float *__restrict__ samples, int32_t *__restrict__ face_of) {
    __shared__ int64_t off[65];
    const int64_t f = blockIdx.x;
    const int lane = threadIdx.x;
    MsFace F;
    ms_face(verts, faces, f, n_verts, density, F, nullptr);
    if (!(F.n1 >= 1.0)) return;
    const int64_t n1i = (int64_t)F.n1;
    const int64_t row0 = (int64_t)blockIdx.y * kRowsPerWave;
    if (row0 > n1i) return;
    const int64_t row1 = min(row0 + kRowsPerWave, n1i + 1);   // this wave's rows [row0, row1)
    // the samples of the face's earlier rows
    int64_t before = 0;
    for (int64_t i = lane; i < row0; i += 64) before += ms_row_count(i, F.n1, F.n2);
    int64_t pos = prefix[f] + hm_wave_reduce(before, HmSum{});

    for (int64_t r = row0; r < row1; r += 64) {
        const int64_t i = r + lane;
        int64_t incl = i < row1 ? ms_row_count(i, F.n1, F.n2) : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        __syncthreads();
        off[lane + 1] = incl;
        if (lane == 0) off[0] = 0;
        __syncthreads();
        const int64_t total = off[64];
        for (int64_t t = lane; t < total; t += 64) {
            int a = 0, b = 64;   // the row with off[a] <= t < off[a + 1]
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (off[mid + 1] <= t) a = mid + 1;
                else b = mid;
            }
            const int64_t j = t - off[a], o = pos + t;
            const double u = __ddiv_rn((double)(r + a) + 0.5, F.n1), v = __ddiv_rn((double)j + 0.5, F.n2);
            if (o >= 0 && o < n_samples) {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    samples[o * 3 + k] =
                        (float)__dadd_rn(__dadd_rn(__dmul_rn(F.v1[k], u), __dmul_rn(F.v2[k], v)), F.a[k]);
                face_of[o] = (int32_t)f;
            }
        }
        pos += total;
    }
}

int ms_check(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts, double density,
             const char *what) {
    const std::string w(what);
    HM_CHECK_ARG(n_faces >= 0 && n_faces < ((int64_t)1 << 31), w + ": n_faces must be in [0, 2^31)");
    HM_CHECK_ARG(n_verts >= 0 && n_verts < ((int64_t)1 << 31), w + ": n_verts must be in [0, 2^31)");
    HM_CHECK_ARG(std::isfinite(density) && density > 0.0, w + ": density must be finite and positive");
    HM_CHECK_ARG(n_faces == 0 || (verts && faces), w + ": NULL mesh");
    return HM_OK;
}

}  // namespace

extern "C" {

int hm_mesh_sample_count(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts, double density,
                         int64_t *count, int32_t *rows, int32_t *status, void *stream) {
    if (int rc = ms_check(verts, faces, n_faces, n_verts, density, "hm_mesh_sample_count")) return rc;
    if (n_faces == 0) return HM_OK;
    HM_CHECK_ARG(count && rows && status, "hm_mesh_sample_count: NULL pointer");
    hipLaunchKernelGGL(ms_count_kernel, dim3((unsigned)n_faces), dim3(64), 0, as_stream(stream), verts, faces, n_verts,
                       density, count, rows, status);
    HM_CHECK_LAUNCH("hm_mesh_sample_count");
    return HM_OK;
}

int hm_mesh_sample_emit(const float *verts, const int32_t *faces, int64_t n_faces, int64_t n_verts, double density,
                        const int64_t *prefix, int64_t n_samples, int64_t max_rows, float *samples, int32_t *face_of,
                        void *stream) {
    if (int rc = ms_check(verts, faces, n_faces, n_verts, density, "hm_mesh_sample_emit")) return rc;
    HM_CHECK_ARG(n_samples >= 0 && n_samples < ((int64_t)1 << 31), "hm_mesh_sample_emit: n_samples must be in [0, 2^31)");
    HM_CHECK_ARG(max_rows >= 0 && max_rows < ((int64_t)1 << 31), "hm_mesh_sample_emit: max_rows must be in [0, 2^31)");
    if (n_faces == 0 || n_samples == 0 || max_rows == 0) return HM_OK;
    HM_CHECK_ARG(prefix && samples && face_of, "hm_mesh_sample_emit: NULL pointer");
    const int64_t split = (max_rows + kRowsPerWave - 1) / kRowsPerWave;
    HM_CHECK_ARG(split <= 65535, "hm_mesh_sample_emit: a face has more than 65535 * 1024 rows");
    hipLaunchKernelGGL(ms_emit_kernel, dim3((unsigned)n_faces, (unsigned)split), dim3(64), 0, as_stream(stream), verts,
                       faces, n_verts, density, prefix, n_samples, samples, face_of);
    HM_CHECK_LAUNCH("hm_mesh_sample_emit");
    return HM_OK;
}

}  // extern "C"
