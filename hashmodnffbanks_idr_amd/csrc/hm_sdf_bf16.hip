// hm_sdf_bf16.hip - bf16 variant of the fused no-grad SDF forward (BASELINE configs[4]: "bf16, fused MLP path").
//
// Same operator as hm_sdf.hip's sdf_fwd_kernel (reference: model/implicit_differentiable_renderer.py:89-113 under
// no_grad), sdf-only output, for the COARSE searches of the ray tracer: the 100-sample sign-change scan and the
// closest-approach scan (model/ray_tracing.py:189-249, 270-298) - 80 % of the SDF evaluations of an iteration.  The
// sphere-tracing rounds and the secant refinement that produce the final hit stay on the exact-fp32 kernels, so the
// bf16 error (~1e-4 abs in the SDF) can only move the choice of a bracketing sample / closest sample, never the
// refined intersection.  The reference has no reduced-precision behaviour; the criterion is the
// measured error against the fp32 kernel and loss-curve agreement, both in tests/test_bf16_gpu.py.
//
// Mapping: v_mfma_f32_32x32x16_bf16 runs at 16x the fp32 MFMA rate, so the tile is bound by its weight stream, not by
// the matrix pipe: a workgroup (8 waves, one per CU) owns 96 points - X as bf16 [k/8][point][8] = 96 KB, the embedding
// in fp32 [e/4][point][4] = 27.6 KB - and every wave computes 2 feature tiles x 3 point tiles per 1-KB weight block
// (6 MFMAs = 192 cycles per 2 KB streamed: ~100 GB/s per CU at the matrix rate, i.e. the L2 stream and the pipe are
// about balanced).  What stays fp32: the embedding and every product that consumes it (layer 0 and the skip layer's
// embedding segment run on v_mfma_f32_32x32x2_f32 from the fp32 operand image - the raw coordinates never see 8-bit
// mantissas), all accumulators, bias / Softplus, the last layer's dot product and the clamp.  Hidden activations and
// hidden-layer weights are bf16 (round-to-nearest-even).  The C/D register layout of the two MFMA shapes is the same
// (row = 8(reg/4) + 4(lane/32) + reg%4, col = lane%32), so both accumulate into the same tiles.
// Point load, encode, weight stream (WeightRing<4, 2>), quad epilogue, embedding rescale, last-layer finish and the LDS
// layout (sdf_lds_bf16) are the stages of hm_sdf_common.h.
#include "hm_common.h"

#include <math.h>

namespace {

#include "hm_sdf_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int kPB = 96;            // points per workgroup tile
constexpr int kTB16 = 512;         // threads
constexpr int kPT = kPB / 32;      // point tiles per wave (3)
constexpr int kEmbGF = kPB * 4;    // floats per k-group row of the fp32 embedding image
constexpr int kXOct = kPB * 8;     // bf16 elements per k-octet row of X

// dynamic LDS: X as bf16 [x_groups / 2][kPB][8], the fp32 embedding, 5 partial sums per point
__host__ __device__ inline SdfLds sdf_lds_bf16(const SdfNet &net) {
    return sdf_lds(kPB, 1, net.x_groups / 2 * kXOct / 2, 1, net.emb_groups * kEmbGF, 5);
}

template <int FRAC>
__global__ __launch_bounds__(kTB16, 2) void sdf_fwd_bf16_kernel(HmLevels lv, SdfNet net, const float *__restrict__ x,
                                                                 int64_t n, const float *__restrict__ table,
                                                                 const float *__restrict__ Bf,
                                                                 float *__restrict__ out, int64_t out_stride,
                                                                 const int32_t *__restrict__ n_dev, int64_t run_min,
                                                                 int64_t run_max) {
    extern __shared__ __align__(16) float lds[];
    if (n_dev) n = min(n, (int64_t)max(*n_dev, 0));
    if (n < run_min || n > run_max) return;
    const SdfLds at = sdf_lds_bf16(net);
    __bf16 *X = reinterpret_cast<__bf16 *>(lds);    // [x_groups / 2][kPB][8] bf16 (k-octets of the widest layer)
    float *EMB = lds + at.emb;                      // [emb_groups][kPB][4] fp32
    float *SX = lds + at.sx;                        // [kPB][3] raw points (+ pad)
    float *RED = lds + at.red;                      // [5][kPB] last-layer partial sums

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform: descriptors / scalar offsets of the weight stream)
    const int lane = tid & 63;
    const int j = lane & 31;
    const int h = lane >> 5;
    const int L = lv.L, E = lv.E;
    const int64_t n_tiles = (n + kPB - 1) / kPB;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t base = tile * kPB;
        const int cnt = (int)min((int64_t)kPB, n - base);
        __syncthreads();
        load_points(net.emb_stride == 0, SX, x, base, cnt, kPB, tid);
        __syncthreads();

        // ---------------- embedding -> EMB[(e/4)][p][e%4] (fp32) ------------------------------------------------
        if (net.emb_stride > 0) {
            load_emb_tile(EMB, x, net.emb_stride, base, cnt, E, net.emb_groups, kPB, kEmbGF, tid, kTB16);
        } else {
            const int n_slot = 2 * L + 1;
            for (int idx = tid; idx < kPB * n_slot; idx += kTB16) {
                const int p = idx % kPB, slot = idx / kPB;
                embed_slot<FRAC>(lv, table, Bf, SX[p * 3], SX[p * 3 + 1], SX[p * 3 + 2], slot, net.emb_groups * 4,
                                 [&](int e, float v) { EMB[(e >> 2) * kEmbGF + p * 4 + (e & 3)] = v; });
            }
        }
        __syncthreads();

        // ---------------- layers ------------------------------------------------------------------------------
        for (int li = 0; li < net.n_layers; ++li) {
            const hm_mlp_layer &Ly = net.layer[li];
            if (li == net.n_layers - 1) {
                // sdf-only last layer (one segment, previous layer's output): fp32 VALU dot of row 0 of the fp32
                // image with the bf16 activations; thread = (point, k slice of 5)
                const float4 *W0 = reinterpret_cast<const float4 *>(Ly.w_packed);
                const int p = tid % kPB, sl = tid / kPB;       // 480 threads busy
                float part = 0.0f;
                if (sl < 5) {
                    const int n_o = Ly.seg_octets[0];
                    for (int kb = sl; kb < n_o; kb += 5) {
                        const bf16x8 xv = *reinterpret_cast<const bf16x8 *>(X + (size_t)kb * kXOct + p * 8);
                        const float4 w0 = W0[(size_t)kb * 64], w1 = W0[(size_t)kb * 64 + 32];   // k = 8kb+0..3 / +4..7
                        part = __fmaf_rn((float)xv[0], w0.x, part);
                        part = __fmaf_rn((float)xv[1], w0.y, part);
                        part = __fmaf_rn((float)xv[2], w0.z, part);
                        part = __fmaf_rn((float)xv[3], w0.w, part);
                        part = __fmaf_rn((float)xv[4], w1.x, part);
                        part = __fmaf_rn((float)xv[5], w1.y, part);
                        part = __fmaf_rn((float)xv[6], w1.z, part);
                        part = __fmaf_rn((float)xv[7], w1.w, part);
                    }
                    RED[sl * kPB + p] = part;
                }
                sdf_last_finish(RED, 5, kPB, cnt, Ly.bias, net.beta, out, base, out_stride, tid);
                break;
            }
            const int nt = Ly.n_tiles;
            const int t0 = 2 * wave;
            const int ntw = max(0, min(2, nt - t0));
            f32x16 acc[2][kPT];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int q = 0; q < kPT; ++q) acc[a][q] = f32x16{0};
            if (ntw > 0) {
                const int n_oct = Ly.seg_octets[0] + Ly.seg_octets[1];
                const int nb = Ly.seg_blocks16[0] + Ly.seg_blocks16[1];
                int oct0 = 0, blk0 = 0;
                for (int seg = 0; seg < 2; ++seg) {
                    if (Ly.seg_octets[seg] == 0) continue;
                    if (Ly.seg_src[seg] == 1) {
                        // ---- embedding segment: exact fp32 (v_mfma_f32_32x32x2_f32, fp32 operand image) -----------
                        const float4 *A0 = reinterpret_cast<const float4 *>(Ly.w_packed) +
                                           ((size_t)t0 * n_oct + oct0) * 64 + lane;
                        const float4 *A1 = A0 + (ntw > 1 ? (size_t)n_oct * 64 : 0);
                        for (int g = 0; g < Ly.seg_octets[seg]; ++g) {
                            const float4 a0 = A0[(size_t)g * 64], a1 = A1[(size_t)g * 64];
                            const float *src = EMB + (2 * g + h) * kEmbGF;
#pragma unroll
                            for (int q = 0; q < kPT; ++q) {
                                const float4 b = *reinterpret_cast<const float4 *>(src + (32 * q + j) * 4);
                                acc[0][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b.x, acc[0][q], 0, 0, 0);
                                acc[1][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b.x, acc[1][q], 0, 0, 0);
                                acc[0][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b.y, acc[0][q], 0, 0, 0);
                                acc[1][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b.y, acc[1][q], 0, 0, 0);
                                acc[0][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b.z, acc[0][q], 0, 0, 0);
                                acc[1][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b.z, acc[1][q], 0, 0, 0);
                                acc[0][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b.w, acc[0][q], 0, 0, 0);
                                acc[1][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b.w, acc[1][q], 0, 0, 0);
                            }
                        }
                    } else {
                        // ---- hidden segment: bf16 (v_mfma_f32_32x32x16_bf16), 1-KB weight blocks through a 4-slot ring
                        const int nbs = Ly.seg_blocks16[seg];
                        // (buffer loads: descriptor on the wave's first feature tile, lane * 16 the one VGPR offset, block /
                        //  tile offsets scalar - no address VALU between the MFMAs, hm_sdf_common.h: ld_w16)
                        const __amdgpu_buffer_rsrc_t rA =
                            w_rsrc(reinterpret_cast<const float *>(Ly.w_packed_bf16) + ((size_t)t0 * nb + blk0) * 256);
                        const int so[2] = {0, ntw > 1 ? nb * 1024 : 0};   // the wave's two feature tiles
                        WeightRing<4, 2> ring;
                        ring.voff = lane * 16;
                        ring.fill(rA, so, nbs);
                        ring.run(rA, so, nbs, no_pre, [&](int t, int, const float4 (&w)[2]) {
                            const bf16x8 a0 = __builtin_bit_cast(bf16x8, w[0]), a1 = __builtin_bit_cast(bf16x8, w[1]);
                            const __bf16 *src = X + (size_t)(2 * t + h) * kXOct;
#pragma unroll
                            for (int q = 0; q < kPT; ++q) {
                                const bf16x8 b = *reinterpret_cast<const bf16x8 *>(src + (32 * q + j) * 8);
                                acc[0][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b, acc[0][q], 0, 0, 0);
                                acc[1][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b, acc[1][q], 0, 0, 0);
                            }
                        });
                    }
                    oct0 += Ly.seg_octets[seg];
                    blk0 += Ly.seg_blocks16[seg];
                }
            }
            __syncthreads();  // every wave has finished reading X / EMB for this layer

            // epilogue: registers 4q..4q+3 of a tile = features 8q + 4h + {0..3} -> 4 bf16 of one k-octet of the next layer
            const bool act = Ly.activation != 0;
            const bool div = Ly.post_div_sqrt2 != 0;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                if (a >= ntw) continue;
                const int fbase = 32 * (t0 + a);
#pragma unroll
                for (int pt = 0; pt < kPT; ++pt) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int f = fbase + 8 * q + 4 * h;
                        const float4 bb = *reinterpret_cast<const float4 *>(Ly.bias + f);
                        float v[4] = {acc[a][pt][4 * q + 0] + bb.x, acc[a][pt][4 * q + 1] + bb.y,
                                      acc[a][pt][4 * q + 2] + bb.z, acc[a][pt][4 * q + 3] + bb.w};
                        act_quads(v, act, div);
                        bf16x4 o;
                        o[0] = (__bf16)v[0]; o[1] = (__bf16)v[1]; o[2] = (__bf16)v[2]; o[3] = (__bf16)v[3];
                        *reinterpret_cast<bf16x4 *>(X + (size_t)(f >> 3) * kXOct + (32 * pt + j) * 8 + 4 * h) = o;
                    }
                }
            }
            if (li == 0 && net.emb_groups > 0) rescale_emb(EMB, net.emb_groups * kEmbGF, tid, kTB16);
            __syncthreads();
        }
    }
}

// the network and LDS checks of every launch of this kernel (hm_sdf_net_fits asks the same): *lds = its dynamic LDS
static int sdf_bf16_net(const char *who, int E, const hm_mlp_desc *mlp, int64_t emb_stride, SdfNet &net, size_t *lds,
                        int32_t *regions = nullptr) {
    const int rc = sdf_net_from_desc(who, mlp, E, emb_stride, kImgBf16, 2, (E + 7) / 8 * 2, true, net);
    if (rc != HM_OK) return rc;
    *lds = sdf_lds_bf16(net).bytes();
    if (regions) sdf_lds_report(sdf_lds_bf16(net), regions);
    if (*lds > 160 * 1024) return hm_fail(HM_ERR_INVALID, std::string(who) + ": network does not fit the 160 KB LDS tile");
    return HM_OK;
}

static int sdf_bf16_impl(const HmLevels &lv, const hm_mlp_desc *mlp, const float *x, int64_t emb_stride, int64_t n,
                         const float *table, const float *B_fourier, float *out, int64_t out_stride, int frac_mode,
                         const int32_t *n_dev, int64_t run_min, void *stream) {
    HM_CHECK_ARG(n >= 0, "hm_sdf_fwd_bf16: n < 0");
    HM_CHECK_ARG(frac_mode == HM_FRAC_REFERENCE || frac_mode == HM_FRAC_TRILINEAR, "hm_sdf_fwd_bf16: bad frac_mode");
    SdfNet net;
    size_t lds = 0;
    const int rc = sdf_bf16_net("hm_sdf_fwd_bf16", lv.E, mlp, emb_stride, net, &lds);
    if (rc != HM_OK) return rc;
    if (n == 0) return HM_OK;
    HM_CHECK_ARG(x && out && (emb_stride > 0 || (table && B_fourier)), "hm_sdf_fwd_bf16: NULL pointer");
    const int64_t tiles = (n + kPB - 1) / kPB;
    const int64_t grid = tiles < 256 ? tiles : 256;
    const int64_t big = (int64_t)1 << 62;
    return hm_frac_dispatch(frac_mode, [&](auto frac) {
        constexpr auto kernel = sdf_fwd_bf16_kernel<decltype(frac)::value>;
        const int rc = hm_allow_dynamic_lds<kernel>(160 * 1024);
        if (rc != HM_OK) return rc;
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kTB16), lds, as_stream(stream), lv, net, x, n, table,
                           B_fourier, out, out_stride, n_dev, run_min, big);
        HM_CHECK_LAUNCH("hm_sdf_fwd_bf16");
        return HM_OK;
    });
}

}  // namespace

extern "C" {

// (internal: hm_sdf_net_fits / hm_diag_sdf_lds, HM_SDF_BF16; regions may be NULL)
int sdf_bf16_fits(const hm_mlp_desc *mlp, int E, int32_t *regions) {
    SdfNet net;
    size_t lds = 0;
    return sdf_bf16_net("hm_sdf_net_fits", E, mlp, 0, net, &lds, regions);
}

int hm_sdf_fwd_bf16(const hm_grid_desc *desc, const hm_mlp_desc *mlp, const float *x, int64_t n, const float *table,
                    const float *B_fourier, float *out, int64_t out_stride, int frac_mode, const int32_t *n_dev,
                    int64_t run_min, void *stream) {
    HM_CHECK_ARG(desc, "hm_sdf_fwd_bf16: NULL descriptor");
    return sdf_bf16_impl(desc->lv, mlp, x, 0, n, table, B_fourier, out, out_stride, frac_mode, n_dev, run_min, stream);
}

int hm_sdf_fwd_emb_bf16(const hm_mlp_desc *mlp, const float *emb, int64_t emb_stride, int emb_width, int64_t n,
                        float *out, int64_t out_stride, const int32_t *n_dev, int64_t run_min, void *stream) {
    HmLevels lv;
    const int rc = sdf_emb_levels("hm_sdf_fwd_emb_bf16", emb_width, emb_stride, lv);
    if (rc != HM_OK) return rc;
    return sdf_bf16_impl(lv, mlp, emb, emb_stride, n, nullptr, nullptr, out, out_stride, HM_FRAC_REFERENCE, n_dev,
                         run_min, stream);
}

}  // extern "C"
