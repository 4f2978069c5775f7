// hm_mesh_texture.hip - a per-face texture atlas of an extracted mesh (contract: include/hashmod.h; driver:
// ops.mesh_texture_points, ops.mesh_texture_sample, evaluation/texture.py, evaluation/mesh_views.py):
//
//   hm_mesh_texture_points  one lane per texel: which face owns it, its barycentric coordinates as small integers over
//                           2 res, and the point (and normal) they give on the face - what hm_mesh_vertex_colors then
//                           colours as if the texels were vertices
//   hm_mesh_texture_sample  one lane per sample: (face, weights) of the visibility buffer back to four texels of the
//                           face's half block and their bilinear blend
//
// Two faces share a block of (res + 2) x (res + 3) texels, the upper one point-mirrored; the texels are stored block
// after block, so a wave writes whole rows and neighbouring lanes hold neighbouring points of one face.  Every
// operation is fp64 and rounded once (hm_color_dev.h), a texel and a sample belong to one lane: no atomics but the
// status word's, no workspace, two calls give the same bits.  No face or vertex index is dereferenced before its range
// check, and the sampler clamps its position to the block as doubles before any integer is formed: the taps are in
// [0, res + 2] x [0, res + 1] whatever the weights are.
#include "hm_block_dev.h"
#include "hm_color_dev.h"

namespace {

constexpr int kTT = 256;
constexpr int64_t kTexMaxRes = 4096;
constexpr int64_t kTexMaxTexels = (int64_t)1 << 40;

struct TexBackground {
    float v[3];
};

// float(((b0 a) + (b1 b)) + (b2 c))
__device__ __forceinline__ float tex_mix(double b0, double b1, double b2, float a, float b, float c) {
    return __double2float_rn(color_dot(b0, b1, b2, (double)a, (double)b, (double)c));
}

__global__ __launch_bounds__(kTT) void texture_points_kernel(const float *__restrict__ verts,
                                                             const float *__restrict__ normals, int64_t n_verts,
                                                             const int32_t *__restrict__ faces, int64_t n_faces, int n,
                                                             int64_t n_texels, float *__restrict__ points,
                                                             float *__restrict__ tex_normals,
                                                             int32_t *__restrict__ face, int32_t *status) {
    const int64_t t = (int64_t)blockIdx.x * kTT + threadIdx.x;
    if (t >= n_texels) return;
    const int Wb = n + 3, per = (n + 2) * Wb;
    const int64_t b = t / per;
    const int r = (int)(t - b * per);
    int j = r / Wb, i = r - j * Wb;
    const bool upper = i + j > n + 1;
    if (upper) {
        i = n + 2 - i;
        j = n + 1 - j;
    }
    const int64_t f = 2 * b + (upper ? 1 : 0);
    const float nan = __uint_as_float(0x7fc00000u);
    int32_t id[3];
    if (f >= n_faces || !hm_face_ids(faces, f, n_verts, id, status)) {   // the absent half of the last block, or refused
        face[t] = -1;
#pragma unroll
        for (int c = 0; c < 3; ++c) points[t * 3 + c] = nan;
        if (tex_normals) {
#pragma unroll
            for (int c = 0; c < 3; ++c) tex_normals[t * 3 + c] = nan;
        }
        return;
    }
    // inside: the lattice point; on the gutter i + j = n + 1: the nearest point of the hypotenuse
    const int S = i + j <= n ? 2 * i : min(max(2 * i - 1, 0), 2 * n);
    const int T = i + j <= n ? 2 * j : 2 * n - S;
    const double d = (double)(2 * n);
    const double b0 = __ddiv_rn((double)(2 * n - S - T), d), b1 = __ddiv_rn((double)S, d), b2 = __ddiv_rn((double)T, d);
    const float *A = verts + (int64_t)id[0] * 3, *B = verts + (int64_t)id[1] * 3, *C = verts + (int64_t)id[2] * 3;
    face[t] = (int32_t)f;
#pragma unroll
    for (int c = 0; c < 3; ++c) points[t * 3 + c] = tex_mix(b0, b1, b2, A[c], B[c], C[c]);
    if (tex_normals) {
        A = normals + (int64_t)id[0] * 3, B = normals + (int64_t)id[1] * 3, C = normals + (int64_t)id[2] * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) tex_normals[t * 3 + c] = tex_mix(b0, b1, b2, A[c], B[c], C[c]);
    }
}

__global__ __launch_bounds__(kTT) void texture_sample_kernel(const float *__restrict__ texels, int n, int64_t n_faces,
                                                             const int32_t *__restrict__ face_id,
                                                             const float *__restrict__ weights, int64_t n_samples,
                                                             TexBackground bg, float *__restrict__ out,
                                                             int32_t *status) {
    const int64_t p = (int64_t)blockIdx.x * kTT + threadIdx.x;
    if (p >= n_samples) return;
    const int64_t f = face_id[p];
    const float w1 = weights[p * 3 + 1], w2 = weights[p * 3 + 2];
    const bool on = f >= 0 && f < n_faces && isfinite(weights[p * 3]) && isfinite(w1) && isfinite(w2);
    if (f >= n_faces) atomicOr(status, 1);
    if (!on) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[p * 3 + c] = bg.v[c];
        return;
    }
    const int Wb = n + 3, Hb = n + 2;
    const double s = __dmul_rn((double)w1, (double)n), t = __dmul_rn((double)w2, (double)n);
    double px = s, py = t;
    if (f & 1) {
        px = __dsub_rn((double)(n + 2), s);
        py = __dsub_rn((double)(n + 1), t);
    }
    // finite by now; the clamp comes before the integers
    px = fmin(fmax(px, 0.0), (double)(Wb - 1));
    py = fmin(fmax(py, 0.0), (double)(Hb - 1));
    const double fx0 = floor(px), fy0 = floor(py);
    const double fx = __dsub_rn(px, fx0), fy = __dsub_rn(py, fy0);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int x1 = min(x0 + 1, Wb - 1), y1 = min(y0 + 1, Hb - 1);
    const float *blk = texels + (f >> 1) * ((int64_t)Hb * Wb * 3);
    const float *taa = blk + (y0 * Wb + x0) * 3, *tab = blk + (y0 * Wb + x1) * 3;
    const float *tba = blk + (y1 * Wb + x0) * 3, *tbb = blk + (y1 * Wb + x1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        out[p * 3 + c] = __double2float_rn(color_lerp(color_lerp((double)taa[c], (double)tab[c], fx),
                                                      color_lerp((double)tba[c], (double)tbb[c], fx), fy));
}

int tex_check_res(int64_t res, int64_t n_faces, const char *what) {
    const std::string w(what);
    HM_CHECK_ARG(res >= 1 && res <= kTexMaxRes, w + ": res must be in [1, 4096]");
    HM_CHECK_ARG(n_faces >= 0 && n_faces < ((int64_t)1 << 31), w + ": n_faces must be in [0, 2^31)");
    HM_CHECK_ARG(((n_faces + 1) / 2) * (res + 2) * (res + 3) < kTexMaxTexels,
                 w + ": the atlas must have fewer than 2^40 texels");
    return HM_OK;
}

}  // namespace

extern "C" {

int hm_mesh_texture_points(const float *verts, const float *normals, int64_t n_verts, const int32_t *faces,
                           int64_t n_faces, int64_t res, float *points, float *tex_normals, int32_t *face,
                           int32_t *status, void *stream) {
    if (int rc = hm_check_mesh(n_faces, n_verts, faces, "hm_mesh_texture_points")) return rc;
    if (int rc = tex_check_res(res, n_faces, "hm_mesh_texture_points")) return rc;
    HM_CHECK_ARG((normals != nullptr) == (tex_normals != nullptr),
                 "hm_mesh_texture_points: normals and tex_normals go together");
    if (n_faces == 0) return HM_OK;
    HM_CHECK_ARG(points && face && status && (n_verts == 0 || verts), "hm_mesh_texture_points: NULL pointer");
    const int64_t n_texels = ((n_faces + 1) / 2) * (res + 2) * (res + 3);
    hipLaunchKernelGGL(texture_points_kernel, dim3(hm_grid(n_texels, kTT)), dim3(kTT), 0, as_stream(stream), verts,
                       normals, n_verts, faces, n_faces, (int)res, n_texels, points, tex_normals, face, status);
    HM_CHECK_LAUNCH("hm_mesh_texture_points");
    return HM_OK;
}

int hm_mesh_texture_sample(const float *texels, int64_t res, int64_t n_faces, const int32_t *face_id,
                           const float *weights, int64_t n_samples, const float *background, float *out,
                           int32_t *status, void *stream) {
    if (int rc = tex_check_res(res, n_faces, "hm_mesh_texture_sample")) return rc;
    HM_CHECK_ARG(n_samples >= 0 && n_samples < kTexMaxTexels, "hm_mesh_texture_sample: n_samples must be in [0, 2^40)");
    if (n_samples == 0) return HM_OK;
    HM_CHECK_ARG(face_id && weights && out && status && (n_faces == 0 || texels),
                 "hm_mesh_texture_sample: NULL pointer");
    TexBackground bg;
    for (int c = 0; c < 3; ++c) bg.v[c] = background ? background[c] : 0.0f;
    hipLaunchKernelGGL(texture_sample_kernel, dim3(hm_grid(n_samples, kTT)), dim3(kTT), 0, as_stream(stream), texels,
                       (int)res, n_faces, face_id, weights, n_samples, bg, out, status);
    HM_CHECK_LAUNCH("hm_mesh_texture_sample");
    return HM_OK;
}

}  // extern "C"
