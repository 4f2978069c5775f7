// hm_mesh_rec_dev.h - what the kernels that read the triangle grid share (hm_mesh_dist.hip builds it and answers
// closest-point queries, hm_mesh_ray.hip casts rays through it): the 48-byte face record, the fp32 vector operations
// of the two definitions (include/hashmod.h), each rounded once, and the host-side check of the record counts.  The
// grid itself (NnGrid, nn_cell, the checked cell faces) is hm_nn_dev.h's.
#pragma once
#include <math.h>

#include "hm_nn_dev.h"

constexpr int kRecVec = 3;    // float4 per record: ax ay az bx | by bz cx cy | cz face 0 0
constexpr int32_t kNoFace = 0x7fffffff;

struct MdVec {
    float x, y, z;
};
__device__ __forceinline__ MdVec md_sub(MdVec u, MdVec v) {
    return {__fsub_rn(u.x, v.x), __fsub_rn(u.y, v.y), __fsub_rn(u.z, v.z)};
}
__device__ __forceinline__ float md_dot(MdVec u, MdVec v) {
    return __fadd_rn(__fadd_rn(__fmul_rn(u.x, v.x), __fmul_rn(u.y, v.y)), __fmul_rn(u.z, v.z));
}
__device__ __forceinline__ MdVec md_cross(MdVec u, MdVec v) {
    return {__fsub_rn(__fmul_rn(u.y, v.z), __fmul_rn(u.z, v.y)), __fsub_rn(__fmul_rn(u.z, v.x), __fmul_rn(u.x, v.z)),
            __fsub_rn(__fmul_rn(u.x, v.y), __fmul_rn(u.y, v.x))};
}
// p0 + t*d
__device__ __forceinline__ MdVec md_along(MdVec p0, float t, MdVec d) {
    return {__fadd_rn(p0.x, __fmul_rn(t, d.x)), __fadd_rn(p0.y, __fmul_rn(t, d.y)), __fadd_rn(p0.z, __fmul_rn(t, d.z))};
}

inline int md_check_counts(int64_t n_pairs, int64_t n_big, const char *what) {
    const std::string w(what);
    HM_CHECK_ARG(n_pairs >= 0 && n_big >= 0 && n_pairs + n_big >= 1 && n_pairs + n_big < ((int64_t)1 << 31),
                 w + ": n_pairs and n_big must be >= 0 and their sum in [1, 2^31)");
    return HM_OK;
}
