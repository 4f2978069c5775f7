// hm_color_dev.h - the two fp64 expressions the colouring and the texture kernels share (hm_mesh_color.hip,
// hm_mesh_texture.hip), written once: each operation rounded once, in this association, whatever the build flags say.
#pragma once
#include "hm_common.h"

#ifdef __HIPCC__
// ((ax bx) + (ay by)) + (az bz)
__device__ __forceinline__ double color_dot(double ax, double ay, double az, double bx, double by, double bz) {
    return __dadd_rn(__dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by)), __dmul_rn(az, bz));
}

// (a (1 - f)) + (b f)
__device__ __forceinline__ double color_lerp(double a, double b, double f) {
    return __dadd_rn(__dmul_rn(a, __dsub_rn(1.0, f)), __dmul_rn(b, f));
}
#endif
