// hm_sdf_split.hip - the fused no-grad SDF forward on the 16-bit matrix cores with SPLIT operands.
//
// Same operator as hm_sdf.hip's sdf_fwd_kernel (reference: model/implicit_differentiable_renderer.py:89-113 under
// no_grad; density_net.py:20-30), sdf-only output, for the coarse scans of the ray tracer (model/ray_tracing.py:189-249,
// 270-298).  Every operand of every matrix product - weights, hidden activations AND the embedding - is carried as a
// pair (hi, lo) of 16-bit floats with  c v ~= hi + lo  (c = a power-of-two operand scale) and the product is evaluated as
//         W x  ~=  (Wh xh + Wh xl + Wl xh) / (c_w c_x)            (three MFMAs, fp32 accumulate; Wl xl is dropped)
// on v_mfma_f32_32x32x16_{bf16,f16}, which run at 16x the rate of the fp32 MFMA:
//   HM_SPLIT_BF16X2  hi, lo bf16 (s = 0): 16 significant bits per operand, relative error 2^-16 per product - the
//                    "bf16" configuration of BASELINE configs[4] with 250x the accuracy of plain bf16 operands;
//   HM_SPLIT_F16X2   hi, lo fp16; activations are stored scaled by 2^4 and weights by 2^8 (so that the lo parts of
//                    ordinary magnitudes are normal fp16 numbers; smaller ones are subnormals, which the MFMA keeps):
//                    22 significant bits per operand, relative error <= 3 * 2^-22 per product - below the rounding noise
//                    an fp32 accumulation over K = 512 adds anyway (~ sqrt(K) 2^-24); activations beyond |x| = 4094
//                    become non-finite and are counted by the tracer's non-finite counter.
// The reference has no such mode; tests/test_split_gpu.py measures both kinds against the exact-fp32 kernel and against
// an fp64 evaluation, and applies SURVEY.md 8(d)'s loss-curve criterion.
//
// Mapping: a workgroup (8 waves, one per CU) owns 64 points.  Activations live in LDS as two planes [k/8][point][8] of
// 2-byte elements (hi, lo) = 128 KB at 512 features, the embedding likewise (2 x 10 KB at E = 67) - the same 4 bytes
// per element as the fp32 kernel.  Wave w owns feature tiles 2w, 2w+1 for both 32-point tiles: per 16-wide k block it
// streams 4 KB of the split weight image ([tile][block][hi | lo][lane][8]) through a 4-slot register ring, reads the
// four B fragments with ds_read_b128 and issues 12 MFMAs (384 cycles), i.e. ~100 GB/s of weight stream per CU at the
// matrix rate: stream and pipe are about balanced, as in the bf16 kernel.  fp32: accumulators, bias, Softplus, the
// sqrt(2) of the layer before the skip, the last layer's dot product and the clamp.  The 1/sqrt(2) of the skip
// layer's EMBEDDING segment is folded into that segment's weights at pack time (hm_pack_mlp_layer_split).
// Point load, encode (one slot per wave and pass: level parameters are scalar loads), weight stream (WeightRing<4, 4,
// 2048>: hi and lo part of two feature tiles per 2-KB block), last-layer finish and the LDS layout (sdf_lds_split) are
// the stages of hm_sdf_common.h; the quad epilogue (split_quad: one instance per layer kind, bias fetched ahead of the
// k-loop) is hm_sdf_split_tile.h's own.
#include "hm_common.h"

#include <math.h>

namespace {

#include "hm_sdf_common.h"
#ifdef HM_SPLIT_PHASE_PROBE
// scripts/split_phase_probe.py: 100 MHz stamps of one tile's phases (workgroup 0, thread 0, its second tile) -> ts[i], and
// the shader clock over the same tile -> ts[120], ts[121]
__device__ unsigned long long hm_split_probe_ts[128];
#define HM_SPLIT_PROBE(i_)                                                                            \
    do {                                                                                              \
        if (blockIdx.x == 0 && threadIdx.x == 0 && tile == (int64_t)gridDim.x) {                      \
            if ((i_) < 120) hm_split_probe_ts[(i_)] = wall_clock64();                                 \
            if ((i_) == 0 || (i_) == 100) hm_split_probe_ts[120 + ((i_) != 0)] = clock64();           \
        }                                                                                             \
    } while (0)
#endif
#include "hm_sdf_split_tile.h"   // Split<KIND>, the LDS layout, sdf_split_tile: one 64-point tile, and the launch checks

template <int KIND, int FRAC>
__global__ __launch_bounds__(kTS, 2) void sdf_fwd_split_kernel(HmLevels lv, SdfNet net, const float *__restrict__ x,
                                                                int64_t n, const float *__restrict__ table,
                                                                const float *__restrict__ Bf,
                                                                float *__restrict__ out, int64_t out_stride,
                                                                const int32_t *__restrict__ n_dev, int64_t run_min,
                                                                int64_t run_max) {
    extern __shared__ __align__(16) float lds[];
    if (n_dev) n = min(n, (int64_t)max(*n_dev, 0));
    if (n < run_min || n > run_max) return;
    const int64_t n_tiles = (n + kPS - 1) / kPS;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
        sdf_split_tile<KIND, FRAC>(lv, net, x, n, table, Bf, out, out_stride, lds, tile);
}

struct PackSplitArgs {
    const float *W;
    void *img;
    int64_t ldw;
    int32_t out_dim, n_tiles, w0, w1, p16_0, nb;
    float scale0, scale1;
};

// element d of a layer's split image
template <int KIND>
__device__ __forceinline__ void pack_split_body(const PackSplitArgs a, int64_t d) {
    // img[(((u*nb + t)*2 + part)*64 + l)*8 + jj] = part(scale * W[32u + (l&31)][16t + 8(l>>5) + jj])
    const int64_t total = (int64_t)a.n_tiles * a.nb * 512;
    if (d >= total) return;
    const int jj = d & 7, l = (d >> 3) & 63;
    const int64_t blk = d >> 9;
    const int t = (int)(blk % a.nb), u = (int)(blk / a.nb);
    const int row = 32 * u + (l & 31), kpos = 16 * t + 8 * (l >> 5) + jj;
    int col;
    float sc;
    if (kpos < a.p16_0) {
        col = kpos < a.w0 ? kpos : -1;
        sc = a.scale0;
    } else {
        const int kk = kpos - a.p16_0;
        col = kk < a.w1 ? a.w0 + kk : -1;
        sc = a.scale1;
    }
    const float w = (row < a.out_dim && col >= 0) ? __fmul_rn(a.W[(int64_t)row * a.ldw + col], sc) : 0.0f;
    typename Split<KIND>::T hi, lo;
    split_val<KIND>(w * Split<KIND>::ws, hi, lo);
    typename Split<KIND>::T *img = static_cast<typename Split<KIND>::T *>(a.img);
    const int64_t o = (blk * 2) * 512 + l * 8 + jj;
    img[o] = hi;
    img[o + 512] = lo;
}

template <int KIND>
__global__ __launch_bounds__(256) void pack_layer_split_kernel(PackSplitArgs a) {
    pack_split_body<KIND>(a, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// every layer of a network in ONE launch (blockIdx.y = layer), as pack_layer_multi_kernel does for the fp32 images
struct PackSplitTable {
    PackSplitArgs a[HM_MAX_LAYERS];
};
template <int KIND>
__global__ __launch_bounds__(256) void pack_layer_split_multi_kernel(PackSplitTable t) {
    pack_split_body<KIND>(t.a[blockIdx.y], (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// the checks and kernel arguments of one layer's split image; *total = its 2-byte (hi, lo) element pairs
static int fill_pack_split_args(const char *who, PackSplitArgs &a, const float *W, int64_t ldw, int out_dim, int seg_width0,
                                int seg_width1, float seg_scale0, float seg_scale1, void *w_packed_split, int64_t &total) {
    HM_CHECK_ARG(W && w_packed_split, std::string(who) + ": NULL pointer");
    HM_CHECK_ARG(out_dim >= 1 && seg_width0 >= 1 && seg_width1 >= 0 && ldw >= seg_width0 + seg_width1,
                 std::string(who) + ": bad shape");
    a = {};
    a.W = W; a.img = w_packed_split; a.ldw = ldw; a.out_dim = out_dim;
    a.n_tiles = (out_dim + 31) / 32;
    a.w0 = seg_width0; a.w1 = seg_width1;
    a.p16_0 = (seg_width0 + 15) / 16 * 16;
    a.nb = a.p16_0 / 16 + (seg_width1 + 15) / 16;
    a.scale0 = seg_scale0; a.scale1 = seg_scale1;
    total = (int64_t)a.n_tiles * a.nb * 512;
    return HM_OK;
}

static int sdf_split_impl(const HmLevels &lv, const hm_mlp_desc *mlp, const float *x, int64_t emb_stride, int64_t n,
                          const float *table, const float *B_fourier, float *out, int64_t out_stride, int frac_mode,
                          const int32_t *n_dev, int64_t run_min, void *stream) {
    HM_CHECK_ARG(n >= 0, "hm_sdf_fwd_split: n < 0");
    HM_CHECK_ARG(frac_mode == HM_FRAC_REFERENCE || frac_mode == HM_FRAC_TRILINEAR, "hm_sdf_fwd_split: bad frac_mode");
    SdfNet net;
    size_t lds = 0;
    const int rc = sdf_split_net("hm_sdf_fwd_split", lv.E, mlp, emb_stride, net, &lds);
    if (rc != HM_OK) return rc;
    if (n == 0) return HM_OK;
    HM_CHECK_ARG(x && out && (emb_stride > 0 || (table && B_fourier)), "hm_sdf_fwd_split: NULL pointer");
    const int64_t tiles = (n + kPS - 1) / kPS;
    const int64_t grid = tiles < 256 ? tiles : 256;
    const int64_t big = (int64_t)1 << 62;
    const auto launch = [&](auto kind, auto frac) {
        constexpr auto kernel = sdf_fwd_split_kernel<decltype(kind)::value, decltype(frac)::value>;
        const int rc = hm_allow_dynamic_lds<kernel>(160 * 1024);
        if (rc != HM_OK) return rc;
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kTS), lds, as_stream(stream), lv, net, x, n, table,
                           B_fourier, out, out_stride, n_dev, run_min, big);
        HM_CHECK_LAUNCH("hm_sdf_fwd_split");
        return HM_OK;
    };
    return sdf_split_dispatch(mlp, frac_mode, launch);
}

}  // namespace

extern "C" {

#ifdef HM_SPLIT_PHASE_PROBE
HM_API int hm_split_probe_read(unsigned long long *out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(hm_split_probe_ts), sizeof(unsigned long long) * (size_t)(n < 128 ? n : 128)) == hipSuccess ? 0 : -1;
}
#endif

// (internal: hm_sdf_net_fits / hm_diag_sdf_lds, HM_SDF_SPLIT; regions may be NULL)
int sdf_split_fits(const hm_mlp_desc *mlp, int E, int32_t *regions) {
    SdfNet net;
    size_t lds = 0;
    return sdf_split_net("hm_sdf_net_fits", E, mlp, 0, net, &lds, regions);
}

int hm_pack_mlp_layer_split(const float *W, int64_t ldw, int out_dim, int seg_width0, int seg_width1, float seg_scale0,
                            float seg_scale1, int split_kind, void *w_packed_split, void *stream) {
    HM_CHECK_ARG(split_kind == HM_SPLIT_BF16X2 || split_kind == HM_SPLIT_F16X2, "hm_pack_mlp_layer_split: bad split_kind");
    PackSplitArgs a;
    int64_t total = 0;
    const int rc = fill_pack_split_args("hm_pack_mlp_layer_split", a, W, ldw, out_dim, seg_width0, seg_width1, seg_scale0,
                                        seg_scale1, w_packed_split, total);
    if (rc != HM_OK) return rc;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (split_kind == HM_SPLIT_BF16X2)
        hipLaunchKernelGGL(pack_layer_split_kernel<HM_SPLIT_BF16X2>, grid, dim3(256), 0, as_stream(stream), a);
    else
        hipLaunchKernelGGL(pack_layer_split_kernel<HM_SPLIT_F16X2>, grid, dim3(256), 0, as_stream(stream), a);
    HM_CHECK_LAUNCH("hm_pack_mlp_layer_split");
    return HM_OK;
}

int hm_pack_mlp_layers_split(const hm_pack_split_item *items, int n_items, int split_kind, void *stream) {
    HM_CHECK_ARG(n_items >= 0 && n_items <= HM_MAX_LAYERS && (n_items == 0 || items), "hm_pack_mlp_layers_split: bad argument");
    HM_CHECK_ARG(split_kind == HM_SPLIT_BF16X2 || split_kind == HM_SPLIT_F16X2, "hm_pack_mlp_layers_split: bad split_kind");
    if (n_items == 0) return HM_OK;
    PackSplitTable t;
    int64_t max_total = 0;
    for (int i = 0; i < n_items; ++i) {
        int64_t total = 0;
        const hm_pack_split_item &I = items[i];
        const int rc = fill_pack_split_args("hm_pack_mlp_layers_split", t.a[i], I.W, I.ldw, I.out_dim, I.seg_width0,
                                            I.seg_width1, I.seg_scale0, I.seg_scale1, I.w_packed_split, total);
        if (rc != HM_OK) return rc;
        max_total = total > max_total ? total : max_total;
    }
    for (int i = n_items; i < HM_MAX_LAYERS; ++i) t.a[i] = t.a[0];
    const dim3 grid((unsigned)((max_total + 255) / 256), (unsigned)n_items);
    if (split_kind == HM_SPLIT_BF16X2)
        hipLaunchKernelGGL(pack_layer_split_multi_kernel<HM_SPLIT_BF16X2>, grid, dim3(256), 0, as_stream(stream), t);
    else
        hipLaunchKernelGGL(pack_layer_split_multi_kernel<HM_SPLIT_F16X2>, grid, dim3(256), 0, as_stream(stream), t);
    HM_CHECK_LAUNCH("hm_pack_mlp_layers_split");
    return HM_OK;
}

int hm_sdf_fwd_split(const hm_grid_desc *desc, const hm_mlp_desc *mlp, const float *x, int64_t n, const float *table,
                     const float *B_fourier, float *out, int64_t out_stride, int frac_mode, const int32_t *n_dev,
                     int64_t run_min, void *stream) {
    HM_CHECK_ARG(desc, "hm_sdf_fwd_split: NULL descriptor");
    return sdf_split_impl(desc->lv, mlp, x, 0, n, table, B_fourier, out, out_stride, frac_mode, n_dev, run_min, stream);
}

int hm_sdf_fwd_emb_split(const hm_mlp_desc *mlp, const float *emb, int64_t emb_stride, int emb_width, int64_t n,
                         float *out, int64_t out_stride, const int32_t *n_dev, int64_t run_min, void *stream) {
    HmLevels lv;
    const int rc = sdf_emb_levels("hm_sdf_fwd_emb_split", emb_width, emb_stride, lv);
    if (rc != HM_OK) return rc;
    return sdf_split_impl(lv, mlp, emb, emb_stride, n, nullptr, nullptr, out, out_stride, HM_FRAC_REFERENCE, n_dev,
                          run_min, stream);
}

}  // extern "C"
