// hm_common.h - shared host/device definitions for libhashmod (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>

#include "../../include/hashmod.h"

// Level table handed to kernels BY VALUE (lands in kernarg / SGPRs; no device allocation).
struct HmLevels {
    int32_t L;
    int32_t F;
    int32_t E;                       // 3 + 2L + L*F
    int32_t pad_;
    int32_t res[HM_MAX_LEVELS];
    uint32_t rows[HM_MAX_LEVELS];
    uint32_t magic[HM_MAX_LEVELS];   // floor(2^32 / rows) for non power-of-two rows, 0 => use mask
    uint32_t row_off[HM_MAX_LEVELS]; // first row of the level inside the fused table
};

struct hm_grid_desc {
    HmLevels lv;
    uint64_t total_rows;
};

void hm_set_error(const std::string &msg);
int hm_fail(int code, const std::string &msg);

#define HM_CHECK_ARG(cond, msg)                                   \
    do {                                                          \
        if (!(cond)) return hm_fail(HM_ERR_INVALID, (msg));       \
    } while (0)

#define HM_CHECK_LAUNCH(what)                                                                     \
    do {                                                                                          \
        hipError_t e__ = hipGetLastError();                                                       \
        if (e__ != hipSuccess) return hm_fail(HM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e__)); \
    } while (0)

// a step of a launch sequence: its error code ends the sequence
#define HM_TRY(call)                      \
    do {                                  \
        const int rc__ = (call);          \
        if (rc__ != HM_OK) return rc__;   \
    } while (0)

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Carves a workspace into its parts: take<T>(count) is the next 256-byte-aligned block of count elements of T, `bytes`
// what has been taken so far.  With a null base it only counts, so ONE layout function written over it yields both
// hm_*_workspace_bytes and the launcher's pointers, and a part cannot be in one and not in the other.
struct HmCarve {
    char *base;
    int64_t bytes = 0;
    explicit HmCarve(void *ws) : base(static_cast<char *>(ws)) {}
    template <class T>
    T *take(int64_t count) {
        T *p = base ? reinterpret_cast<T *>(base + bytes) : nullptr;
        bytes += ((int64_t)sizeof(T) * count + 255) / 256 * 256;
        return p;
    }
};

// Workspace of "sort n int32 keys, keep the permutation" (hm_mesh_cc_sums, hm_nn_build, hm_nn_query):
// [key n i32 | keys_sorted n i32 | perm n i64 | hm_sort_pairs_i32's own workspace]
struct HmKeySortWs {
    int32_t *key, *keys_sorted;
    int64_t *perm;
    void *sort_ws;
    int64_t sort_bytes, bytes;
};

inline HmKeySortWs hm_keysort_layout(void *ws, int64_t n) {
    HmCarve c(ws);
    HmKeySortWs w;
    w.key = c.take<int32_t>(n);
    w.keys_sorted = c.take<int32_t>(n);
    w.perm = c.take<int64_t>(n);
    w.sort_bytes = hm_sort_workspace_bytes(n);
    w.sort_ws = c.take<char>(w.sort_bytes);
    w.bytes = c.bytes;
    return w;
}

// Opts Kernel in to `bytes` of dynamic LDS (above the 64 KB default), once per host thread (not a stream operation).
template <auto Kernel>
int hm_allow_dynamic_lds(int bytes) {
    static thread_local bool done = false;
    if (done) return HM_OK;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return hm_fail(HM_ERR_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e));
    done = true;
    return HM_OK;
}

// f(std::integral_constant<int, FRAC>{}) for the run-time frac_mode (HM_FRAC_REFERENCE or HM_FRAC_TRILINEAR): each
// launch is written once, with FRAC as its kernel's template value
template <class F>
auto hm_frac_dispatch(int frac_mode, F &&f) {
    if (frac_mode == HM_FRAC_REFERENCE) return f(std::integral_constant<int, HM_FRAC_REFERENCE>{});
    return f(std::integral_constant<int, HM_FRAC_TRILINEAR>{});
}

// f(std::true_type{}) or f(std::false_type{}) for the run-time b: a launch whose kernel takes b as a template value is
// written once
template <class F>
auto hm_bool_dispatch(bool b, F &&f) {
    if (b) return f(std::true_type{});
    return f(std::false_type{});
}

// Small-batch rule of the fused SDF forward (hm_sdf.hip): up to kSdfSmall live points run on the small-tile launch -
// 8-point tiles up to kSdfTiny, 4-point tiles up to kSdfMini - more on 64-point tiles.  hm_trace.hip picks its launch
// forms by the same bound: a launch that takes only counts above it passes run_min = kSdfSmall + 1.
constexpr int64_t kSdfSmall = 8192, kSdfTiny = 2048, kSdfMini = 1024;

#ifdef __HIPCC__
// Small device-side fills / copies as ordinary KERNELS.  hipMemsetAsync / hipMemcpyAsync become MEMSET / MEMCPY
// nodes when the call is recorded into a HIP graph; on ROCm 7.0 those nodes were seen to lose their place
// relative to the neighbouring kernel nodes when a graph is re-launched back to back (zeroed cursors in the
// middle of a ray search -> wild indices -> GPU memory fault).  Kernel nodes keep their order.
static __global__ __launch_bounds__(256) void hm_zero_u32_kernel(uint32_t *p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0u;
}
static __global__ __launch_bounds__(64) void hm_copy_u32_kernel(uint32_t *dst, const uint32_t *src, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
static inline void hm_zero_u32_async(void *p, int64_t n_words, hipStream_t st) {
    if (n_words > 0)
        hipLaunchKernelGGL(hm_zero_u32_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, st,
                           static_cast<uint32_t *>(p), n_words);
}

// nn.Softplus(beta, threshold) and its derivatives (shared by hm_elem.hip and the GEMM epilogues), evaluated with the
// native exp2 / log2 / rcp units (v_exp_f32, v_log_f32, v_rcp_f32: 1 ulp each) instead of libm's expf / log1pf and IEEE
// divisions - those were ~100 VALU instructions per activation on the epilogue of ~64 GEMMs per training step (+ 6 us
// on a 27 us GEMM), and VALU work is serial with the MFMAs on gfx950.
//   softplus(z) = log1p(exp(bz))/beta = max(z, 0) + ln(1 + exp(-|bz|))/beta     (bz = beta z <= threshold)
// the logarithm term is <= ln 2 / beta, so its 1-2 ulp error is < 2e-9 absolute for beta = 100; s1, s2 carry ~3e-7
// relative error (tests/test_gemm_ep_gpu.py compares all three with torch at 2e-5).
struct SpDeriv {
    float s1, s2;
};
__device__ __forceinline__ float hm_softplus_fwd(float z, float beta, float thr) {
    const float bz = z * beta;
    const float t = __builtin_amdgcn_exp2f(-fabsf(bz) * 1.4426950408889634f);
    const float l = __builtin_amdgcn_logf(1.0f + t) * (0.6931471805599453f * __builtin_amdgcn_rcpf(beta));
    return bz > thr ? z : fmaxf(z, 0.0f) + l;
}
// s1 = d softplus/dz = e/(e+1), s2 = d^2 softplus/dz^2 = beta*e/(e+1)^2 (no cancellation in 1 - s1), e = exp(beta z)
__device__ __forceinline__ SpDeriv hm_sp_deriv(float z, float beta, float thr) {
    SpDeriv d;
    const float bz = z * beta;
    if (bz > thr) {
        d.s1 = 1.0f;
        d.s2 = 0.0f;
    } else {
        const float e = __builtin_amdgcn_exp2f(bz * 1.4426950408889634f);
        const float r = __builtin_amdgcn_rcpf(e + 1.0f);
        d.s1 = e * r;
        d.s2 = beta * d.s1 * r;
    }
    return d;
}

// hash of one voxel corner: reference hashGridEmbedding.py:32-40 restated in uint32
// (primes 1, 3, 2654435761; xor fold; unsigned modulo by the level's row count).
__device__ __forceinline__ uint32_t hm_mod_rows(uint32_t h, uint32_t rows, uint32_t magic) {
    if (magic == 0u) return h & (rows - 1u);  // power of two (also rows == 1)
    uint32_t q = __umulhi(h, magic);          // q in {floor(h/rows) - 1, floor(h/rows)}
    uint32_t r = h - q * rows;
    return r >= rows ? r - rows : r;
}
__device__ __forceinline__ uint32_t hm_hash3(uint32_t ux, uint32_t uy, uint32_t uz) {
    return ux ^ (uy * 3u) ^ (uz * 2654435761u);
}
// xi = trunc(x*res): fp32 product, then truncation toward zero (hashGridEmbedding.py:84-85)
__device__ __forceinline__ int32_t hm_trunc_voxel(float x, int32_t res) {
    return (int32_t)__fmul_rn(x, (float)res);
}
// one axis of voxel corner `bit`: grid index u and interpolation weight w.  Reference mode: xf = x - x.float() == 0
// (hashGridEmbedding.py:86), so w = where(mask, 1 - xf, xf) is 1 for bit 0 and 0 for bit 1; trilinear: floor + fraction
template <int FRAC>
__device__ __forceinline__ void hm_corner(float x, int32_t res, int bit, uint32_t &u, float &w) {
    if (FRAC == HM_FRAC_REFERENCE) {
        u = (uint32_t)hm_trunc_voxel(x, res) + (uint32_t)bit;
        w = bit ? 0.0f : 1.0f;
    } else {
        const float xs = __fmul_rn(x, (float)res);
        const float fl = floorf(xs);
        u = (uint32_t)((int32_t)fl) + (uint32_t)bit;
        const float xf = __fsub_rn(xs, fl);
        w = bit ? xf : __fsub_rn(1.0f, xf);
    }
}
// Fourier argument a_c = (2 pi x) . B[:, c] (frequency_enc.py:63-67): s_d = 2 pi x_d rounded in fp32, then [N,3]@[3,L]
// as a k-ordered fma chain (matches torch's CPU sgemm bit for bit, see oracle)
__device__ __forceinline__ float hm_fourier_arg(const float *__restrict__ Bf, int L, int c, float s0, float s1, float s2) {
    float a = __fmul_rn(s0, Bf[c]);
    a = __fmaf_rn(s1, Bf[L + c], a);
    return __fmaf_rn(s2, Bf[2 * L + c], a);
}
// features of one point at level l: the weighted sum of its 8 corner rows of the fp32 table (F <= 8), corners in
// index order; zero-weight corners add exactly 0 and are skipped (reference mode: only corner 0 survives)
template <int FRAC>
__device__ __forceinline__ void hm_level_features(const HmLevels &lv, const float *__restrict__ table, int l, float x0,
                                                  float x1, float x2, float (&acc)[8]) {
    const int F = lv.F;
    if (F == 2 && (reinterpret_cast<uintptr_t>(table) & 7) == 0) {
        // two features per row: a corner's row is ONE 8-byte load, and the sums live in two named registers (the
        // generic path below fetches a dword at a time and indexes acc[] with a run-time f); same adds in the same order
        const float2 *tl2 = reinterpret_cast<const float2 *>(table) + lv.row_off[l];
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            uint32_t ux, uy, uz;
            float wx, wy, wz;
            hm_corner<FRAC>(x0, lv.res[l], c & 1, ux, wx);
            hm_corner<FRAC>(x1, lv.res[l], (c >> 1) & 1, uy, wy);
            hm_corner<FRAC>(x2, lv.res[l], (c >> 2) & 1, uz, wz);
            const float w = __fmul_rn(__fmul_rn(wx, wy), wz);
            if (w != 0.0f) {
                const float2 r = tl2[hm_mod_rows(hm_hash3(ux, uy, uz), lv.rows[l], lv.magic[l])];
                a0 = __fadd_rn(a0, __fmul_rn(r.x, w));
                a1 = __fadd_rn(a1, __fmul_rn(r.y, w));
            }
        }
        acc[0] = a0;
        acc[1] = a1;
        return;
    }
    for (int f = 0; f < F; ++f) acc[f] = 0.0f;
    const float *tl = table + (size_t)lv.row_off[l] * F;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        uint32_t ux, uy, uz;
        float wx, wy, wz;
        hm_corner<FRAC>(x0, lv.res[l], c & 1, ux, wx);
        hm_corner<FRAC>(x1, lv.res[l], (c >> 1) & 1, uy, wy);
        hm_corner<FRAC>(x2, lv.res[l], (c >> 2) & 1, uz, wz);
        const float w = __fmul_rn(__fmul_rn(wx, wy), wz);
        if (w != 0.0f) {
            const uint32_t id = hm_mod_rows(hm_hash3(ux, uy, uz), lv.rows[l], lv.magic[l]);
            for (int f = 0; f < F; ++f) acc[f] = __fadd_rn(acc[f], __fmul_rn(tl[(size_t)id * F + f], w));
        }
    }
}
#endif
