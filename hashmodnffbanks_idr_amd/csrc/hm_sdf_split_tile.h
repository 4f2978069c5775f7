// hm_sdf_split_tile.h - the split-operand 64-point tile body (see hm_sdf_split.hip for the arithmetic and the mapping),
// its operand kinds, LDS layout and launch checks, shared by sdf_fwd_split_kernel (hm_sdf_split.hip) and the ray search's
// sdf_refine_scan_kernel (hm_sdf.hip).  Included inside each file's anonymous namespace, behind hm_sdf_common.h.
#pragma once
#ifndef HM_SPLIT_PROBE   // hm_sdf_split.hip's phase-probe stamps (scripts/split_phase_probe.py), never in the product build
#define HM_SPLIT_PROBE(i_) do { } while (0)
#endif
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

template <int KIND> struct Split;
template <> struct Split<HM_SPLIT_BF16X2> {
    typedef __bf16 T;
    typedef bf16x8 V8;
    typedef bf16x4 V4;
    typedef __bf16 V2 __attribute__((ext_vector_type(2)));
    static constexpr float xs = 1.0f, ws = 1.0f, inv = 1.0f;   // operand scales (bf16 has fp32's exponent range: none)
    static __device__ __forceinline__ f32x16 mfma(V8 a, V8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct Split<HM_SPLIT_F16X2> {
    typedef _Float16 T;
    typedef f16x8 V8;
    typedef f16x4 V4;
    typedef _Float16 V2 __attribute__((ext_vector_type(2)));
    // fp16 lo parts are ~2^-11 of their value: activations are stored scaled by 2^4 and weights by 2^8 so that the lo
    // parts of ordinary magnitudes (|x| >= 0.008, |w| >= 5e-4) are NORMAL fp16 numbers; smaller ones become subnormal,
    // which the MFMA keeps (scripts/f16_denorm_probe.hip) - their absolute error stays below 2^-25 / scale.  The
    // accumulators hold 2^12 x the sums; `inv` is applied together with the bias.  Range: |x| <= 4094, |w| <= 255.
    static constexpr float xs = 16.0f, ws = 256.0f, inv = 1.0f / 4096.0f;
    static __device__ __forceinline__ f32x16 mfma(V8 a, V8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
};

// v (already multiplied by the operand's scale) -> hi + lo
template <int KIND>
__device__ __forceinline__ void split_val(float v, typename Split<KIND>::T &hi, typename Split<KIND>::T &lo) {
    typedef typename Split<KIND>::T T;
    hi = (T)v;                                              // round to nearest even
    lo = (T)__fsub_rn(v, (float)hi);
}

// Epilogue of one register quad that already carries its bias: Softplus(100) (ACT), the /sqrt(2) in front of the skip layer
// (DIV), then the four values -> (hi, lo).  The arithmetic is softplus100_x2's and split_val's, operation for operation;
// written out so that hipcc takes the short forms: -|a| as source modifiers of the multiply, max(a, 0) on the scalar FMA
// result (no canonicalising v_max in front of it), and both pairs of the quad on the packed multiply / convert / subtract.
template <int KIND, bool ACT, bool DIV>
__device__ __forceinline__ void split_quad(float (&v)[4], typename Split<KIND>::V4 &oh, typename Split<KIND>::V4 &ol) {
    typedef Split<KIND> S;
    typedef typename S::V2 V2;
    if (ACT) {
#pragma unroll
        for (int i = 0; i < 4; i += 2) {
            f32x2p t = {__builtin_amdgcn_exp2f(-fabsf(v[i]) * 144.26950408889634f),          // -|100 a| log2(e)
                        __builtin_amdgcn_exp2f(-fabsf(v[i + 1]) * 144.26950408889634f)};
            t = t + 1.0f;
            const f32x2p lg = {__builtin_amdgcn_logf(t.x), __builtin_amdgcn_logf(t.y)};
            const f32x2p mx = {fmaxf(v[i], 0.0f), fmaxf(v[i + 1], 0.0f)};
            const f32x2p r = __builtin_elementwise_fma(lg, (f32x2p){0.006931471805599453f, 0.006931471805599453f}, mx);
            v[i] = r.x;
            v[i + 1] = r.y;
        }
    }
    if (DIV) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = __fdiv_rn(v[i], kSqrt2);
    }
#pragma unroll
    for (int i = 0; i < 4; i += 2) {
        const f32x2p s = (f32x2p){v[i], v[i + 1]} * S::xs;
        const V2 hi = __builtin_convertvector(s, V2);                                  // round to nearest even
        const V2 lo = __builtin_convertvector(s - __builtin_convertvector(hi, f32x2p), V2);
        oh[i] = hi.x; oh[i + 1] = hi.y;
        ol[i] = lo.x; ol[i + 1] = lo.y;
    }
}

constexpr int kPS = 64;            // points per workgroup tile
constexpr int kTS = 512;           // threads
constexpr int kWS = 8;             // waves
constexpr int kOctE = kPS * 8;     // 2-byte elements per k-octet row of a plane

// dynamic LDS: hi and lo plane [x_groups / 2][kPS][8] of 2-byte elements for the activations, the same for the
// embedding, 8 partial sums per point
__host__ __device__ inline SdfLds sdf_lds_split(const SdfNet &net) {
    return sdf_lds(kPS, 2, net.x_groups / 2 * kOctE / 2, 2, net.emb_groups / 2 * kOctE / 2, kWS);
}

// One 64-point tile (points tile * 64 .. of the n points at x) of sdf_fwd_split_kernel / sdf_refine_scan_kernel; lds = the
// workgroup's dynamic LDS (sdf_lds_split).  The tile starts with a barrier: the workgroup is done with its previous one.
template <int KIND, int FRAC>
__device__ __forceinline__ void sdf_split_tile(const HmLevels &lv, const SdfNet &net, const float *__restrict__ x,
                                               int64_t n, const float *__restrict__ table, const float *__restrict__ Bf,
                                               float *__restrict__ out, int64_t out_stride, float *lds, int64_t tile) {
    typedef Split<KIND> S;
    typedef typename S::T T;
    typedef typename S::V8 V8;
    typedef typename S::V4 V4;
    const SdfLds at = sdf_lds_split(net);
    const int e_oct = net.emb_groups / 2;
    T *XH = reinterpret_cast<T *>(lds);                       // [x_groups / 2][kPS][8]
    T *XL = reinterpret_cast<T *>(lds + at.x1);
    T *EH = reinterpret_cast<T *>(lds + at.emb);              // [e_oct][kPS][8]
    T *EL = reinterpret_cast<T *>(lds + at.emb1);
    float *SX = lds + at.sx;                                  // [kPS][3] raw points (+ pad)
    float *RED = lds + at.red;                                // [8][kPS] last-layer partial sums

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform: descriptors / scalar offsets of the weight stream)
    const int lane = tid & 63;
    const int j = lane & 31;
    const int h = lane >> 5;
    const int L = lv.L, E = lv.E;
    const int e_pad = e_oct * 8;

    auto put = [&](int p, int e, float v) {
        T hi, lo;
        split_val<KIND>(v * S::xs, hi, lo);
        const size_t o = (size_t)(e >> 3) * kOctE + p * 8 + (e & 7);
        EH[o] = hi;
        EL[o] = lo;
    };

    {
        const int64_t base = tile * kPS;
        const int cnt = (int)min((int64_t)kPS, n - base);
        HM_SPLIT_PROBE(0);
        __syncthreads();
        load_points(net.emb_stride == 0, SX, x, base, cnt, kPS, tid);
        __syncthreads();
        HM_SPLIT_PROBE(1);

        // ---------------- embedding (fp32 arithmetic) -> split planes EH / EL ---------------------------------
        if (net.emb_stride > 0) {
            for (int i = tid; i < kPS * e_pad; i += kTS) {
                const int p = i / e_pad, e = i - p * e_pad;
                put(p, e, (p < cnt && e < E) ? x[(base + p) * net.emb_stride + e] : 0.0f);
            }
        } else {
            const int n_slot = 2 * L + 1;
            // task (point, slot) = (lane, wave + 8 i): the slot is the WAVE's, so its kind is a scalar branch and the
            // level's res / rows / magic / row_off are scalar loads from the kernel arguments
            static_assert(kPS == 64, "one point per lane");
            const float x0 = SX[lane * 3], x1 = SX[lane * 3 + 1], x2 = SX[lane * 3 + 2];
            for (int slot = wave; slot < n_slot; slot += kWS)
                embed_slot<FRAC>(lv, table, Bf, x0, x1, x2, slot, e_pad, [&](int e, float v) { put(lane, e, v); });
        }
        __syncthreads();
        HM_SPLIT_PROBE(2);

        // ---------------- layers ------------------------------------------------------------------------------
        // weight ring (WeightRing, hm_sdf_common.h): 4 slots, 3 blocks of 2 KB in flight per feature tile; it lives across
        // the layers.  Streams per block: [hi | lo] of the wave's first feature tile, then of its second, a1 bytes on.
        WeightRing<4, 4, 2048> ring;
        ring.voff = lane * 16;
        bool ring_ready = false;
        auto prefetch_layer = [&](int l) {      // segment 0 of layer l, this wave's feature tiles
            const hm_mlp_layer &Lp = net.layer[l];
            const int ntp = max(0, min(2, Lp.n_tiles - 2 * wave));
            if (ntp <= 0) return false;
            const int nbp = Lp.seg_blocks16[0] + Lp.seg_blocks16[1];
            const __amdgpu_buffer_rsrc_t rp =
                w_rsrc(reinterpret_cast<const float *>(Lp.w_packed_split) + ((size_t)(2 * wave) * nbp) * 512);
            const int a1 = ntp > 1 ? nbp * 2048 : 0;
            const int so[4] = {0, 1024, a1, a1 + 1024};
            ring.fill(rp, so, Lp.seg_blocks16[0]);
            return true;
        };
        for (int li = 0; li < net.n_layers; ++li) {
            const hm_mlp_layer &Ly = net.layer[li];
            if (li == net.n_layers - 1) {
                // sdf-only last layer (one segment, previous layer's output): fp32 VALU dot of row 0 of the fp32 image
                // with the reassembled activations; thread = (point, k slice of 8)
                const float4 *W0 = reinterpret_cast<const float4 *>(Ly.w_packed);
                const int p = tid & (kPS - 1), sl = tid >> 6;
                float part = 0.0f;
                const int n_o = Ly.seg_octets[0];
                for (int kb = sl; kb < n_o; kb += kWS) {
                    const V8 xh = *reinterpret_cast<const V8 *>(XH + (size_t)kb * kOctE + p * 8);
                    const V8 xl = *reinterpret_cast<const V8 *>(XL + (size_t)kb * kOctE + p * 8);
                    const float4 w0 = W0[(size_t)kb * 64], w1 = W0[(size_t)kb * 64 + 32];   // k = 8kb+0..3 / +4..7
                    const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        part = __fmaf_rn(((float)xl[e] + (float)xh[e]) * (1.0f / S::xs), wv[e], part);
                }
                RED[sl * kPS + p] = part;
                sdf_last_finish(RED, kWS, kPS, cnt, Ly.bias, net.beta, out, base, out_stride, tid);
                HM_SPLIT_PROBE(100);
                break;
            }
            const int nt = Ly.n_tiles;
            const int t0 = 2 * wave;
            const int ntw = max(0, min(2, nt - t0));
            f32x16 acc[2][2];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int q = 0; q < 2; ++q) acc[a][q] = f32x16{0};
            // the epilogue's bias quads, requested in front of the k-loop: behind the barrier they would be one exposed
            // round trip to memory per layer, with every wave of the workgroup waiting at the same moment.  (Unconditional,
            // on a tile index clamped into the padded bias [nt][32], for the waves that own fewer than two tiles.)
            float4 bias4[2][4];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    bias4[a][q] = *reinterpret_cast<const float4 *>(Ly.bias + 32 * min(t0 + a, nt - 1) + 8 * q + 4 * h);
            if (ntw > 0) {
                const int nb = Ly.seg_blocks16[0] + Ly.seg_blocks16[1];
                int blk0 = 0;
                for (int seg = 0; seg < 2; ++seg) {
                    const int nbs = Ly.seg_blocks16[seg];
                    if (nbs == 0) continue;
                    const T *srcH = Ly.seg_src[seg] == 1 ? EH : XH;
                    const T *srcL = Ly.seg_src[seg] == 1 ? EL : XL;
                    // image: [tile][block][hi | lo][lane] float4
                    const __amdgpu_buffer_rsrc_t rA =
                        w_rsrc(reinterpret_cast<const float *>(Ly.w_packed_split) + ((size_t)t0 * nb + blk0) * 512);
                    const int a1 = ntw > 1 ? nb * 2048 : 0;
                    const int so[4] = {0, 1024, a1, a1 + 1024};
                    if (!(seg == 0 && ring_ready)) ring.fill(rA, so, nbs);
                    ring_ready = false;
                    ring.run(rA, so, nbs, no_pre, [&](int t, int, const float4 (&w)[4]) {
                        const V8 a0h = __builtin_bit_cast(V8, w[0]), a0l = __builtin_bit_cast(V8, w[1]),
                                 a1h = __builtin_bit_cast(V8, w[2]), a1l = __builtin_bit_cast(V8, w[3]);
                        const size_t o = (size_t)(2 * t + h) * kOctE + j * 8;
                        const V8 bh0 = *reinterpret_cast<const V8 *>(srcH + o);
                        const V8 bh1 = *reinterpret_cast<const V8 *>(srcH + o + 32 * 8);
                        const V8 bl0 = *reinterpret_cast<const V8 *>(srcL + o);
                        const V8 bl1 = *reinterpret_cast<const V8 *>(srcL + o + 32 * 8);
                        // hi x hi, then hi x lo, then lo x hi: accumulators that are used twice are four MFMAs apart
                        acc[0][0] = S::mfma(a0h, bh0, acc[0][0]);
                        acc[0][1] = S::mfma(a0h, bh1, acc[0][1]);
                        acc[1][0] = S::mfma(a1h, bh0, acc[1][0]);
                        acc[1][1] = S::mfma(a1h, bh1, acc[1][1]);
                        acc[0][0] = S::mfma(a0h, bl0, acc[0][0]);
                        acc[0][1] = S::mfma(a0h, bl1, acc[0][1]);
                        acc[1][0] = S::mfma(a1h, bl0, acc[1][0]);
                        acc[1][1] = S::mfma(a1h, bl1, acc[1][1]);
                        acc[0][0] = S::mfma(a0l, bh0, acc[0][0]);
                        acc[0][1] = S::mfma(a0l, bh1, acc[0][1]);
                        acc[1][0] = S::mfma(a1l, bh0, acc[1][0]);
                        acc[1][1] = S::mfma(a1l, bh1, acc[1][1]);
                    });
                    blk0 += nbs;
                }
            }
            if (li + 1 < net.n_layers - 1) ring_ready = prefetch_layer(li + 1);
            HM_SPLIT_PROBE(3 + 4 * li);
            __syncthreads();  // every wave has finished reading the planes for this layer
            HM_SPLIT_PROBE(4 + 4 * li);

            // epilogue: registers 4q..4q+3 of a tile = features 8q + 4h + {0..3} -> 4 elements of one k-octet of the next layer.
            // The layer's activation / division flags pick ONE instance of the quad loops (no branch inside them: the
            // scheduler interleaves the transcendentals of neighbouring quads).
            auto epilogue = [&](auto act, auto div) {
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    if (a >= ntw) continue;
                    const int fbase = 32 * (t0 + a);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int f = fbase + 8 * q + 4 * h;
                        const float4 bb = bias4[a][q];
#pragma unroll
                        for (int pt = 0; pt < 2; ++pt) {
                            float v[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] = acc[a][pt][4 * q + e];
                            v[0] = __fmaf_rn(v[0], S::inv, bb.x); v[1] = __fmaf_rn(v[1], S::inv, bb.y);
                            v[2] = __fmaf_rn(v[2], S::inv, bb.z); v[3] = __fmaf_rn(v[3], S::inv, bb.w);
                            V4 oh, ol;
                            split_quad<KIND, decltype(act)::value, decltype(div)::value>(v, oh, ol);
                            const size_t o = (size_t)(f >> 3) * kOctE + (32 * pt + j) * 8 + 4 * h;
                            *reinterpret_cast<V4 *>(XH + o) = oh;
                            *reinterpret_cast<V4 *>(XL + o) = ol;
                        }
                    }
                }
            };
            const auto with_div = [&](auto act) {
                if (Ly.post_div_sqrt2 != 0) epilogue(act, std::true_type{}); else epilogue(act, std::false_type{});
            };
            if (Ly.activation != 0) with_div(std::true_type{}); else with_div(std::false_type{});
            HM_SPLIT_PROBE(5 + 4 * li);
            __syncthreads();
            HM_SPLIT_PROBE(6 + 4 * li);
        }
    }
}

// the network and LDS checks of every launch of this kernel (hm_sdf_net_fits asks the same): *lds = its dynamic LDS
static int sdf_split_net(const char *who, int E, const hm_mlp_desc *mlp, int64_t emb_stride, SdfNet &net, size_t *lds,
                         int32_t *regions = nullptr) {
    // (EMB region: k-groups of 4 = 2 octets per 16-block)
    const int rc = sdf_net_from_desc(who, mlp, E, emb_stride, kImgSplit, 2, (E + 15) / 16 * 4, true, net);
    if (rc != HM_OK) return rc;
    *lds = sdf_lds_split(net).bytes();
    if (regions) sdf_lds_report(sdf_lds_split(net), regions);
    if (*lds > 160 * 1024) return hm_fail(HM_ERR_INVALID, std::string(who) + ": network does not fit the 160 KB LDS tile");
    return HM_OK;
}

// hm_frac_dispatch + the kind of the network's split image: f(kind, frac)
template <class F>
int sdf_split_dispatch(const hm_mlp_desc *mlp, int frac_mode, F &&f) {
    return hm_frac_dispatch(frac_mode, [&](auto frac) {
        if (mlp->split_kind == HM_SPLIT_BF16X2) return f(std::integral_constant<int, HM_SPLIT_BF16X2>{}, frac);
        return f(std::integral_constant<int, HM_SPLIT_F16X2>{}, frac);
    });
}
