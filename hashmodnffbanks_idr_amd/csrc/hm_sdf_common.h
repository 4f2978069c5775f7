// hm_sdf_common.h - device helpers shared by the fused SDF kernels (hm_sdf.hip: exact fp32; hm_sdf_bf16.hip: bf16
// coarse-search variant; hm_sdf_split.hip: split-operand variant).  Included inside each file's anonymous namespace.
#pragma once
typedef float f32x16 __attribute__((ext_vector_type(16)));


struct SdfNet {  // by value -> kernarg
    int32_t n_layers;
    int32_t x_groups;    // k-groups (of 4) in the X region
    int32_t emb_groups;  // k-groups in the EMB region
    float beta;          // Laplace density beta = |beta_param| + beta_min
    int64_t emb_stride;  // > 0: `x` holds PRECOMPUTED embedding rows (emb_stride floats apart, lv.E used) - the encode
                         //      phase becomes a tile load (embedders other than the plain hash grid, hm_sdf_fwd_emb)
    hm_mlp_layer layer[HM_MAX_LAYERS];
};

// 16 bytes of a packed weight image: buffer load with the descriptor in SGPRs, `voff` = lane * 16 (one loop-invariant
// VGPR) and the tile / octet offset as the SCALAR offset - no per-load 64-bit address arithmetic on the VALU, whose
// instructions are serial with the MFMAs of both waves on a SIMD (r3af: 128 -> 132 TFLOP/s on the 64-point kernel)
__device__ __forceinline__ float4 ld_w16(const __amdgpu_buffer_rsrc_t &rs, int voff, int soff) {
    const auto u = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
    return make_float4(__uint_as_float(u[0]), __uint_as_float(u[1]), __uint_as_float(u[2]), __uint_as_float(u[3]));
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t w_rsrc(const float *base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base), 0, 0x7fffffff, 0x00020000);
}

// Weight stream of a layer: a register ring of D slots over the blocks (BLK bytes apart) of a packed image, S 16-byte
// loads per block at the scalar offsets so[0..S) (the wave's feature tiles, or the hi / lo parts of the split image).
// D - 1 blocks are in flight.  fill() requests blocks 0 .. D-2 (for layer l + 1 before layer l's epilogue: weights do not
// depend on the activations, so the stream does not restart from an empty pipe behind the barriers of every layer);
// run() requests block t + D - 1 into the slot block t - 1 left, calls pre(t, u) - the hook where a body requests the LDS
// operands of block t + 1 - and runs body(t, u, slot of block t) for every block; u = t mod D is a constant after unrolling.
//   * Every load is unconditional with a clamped block index, so that hipcc emits counted vmcnt waits instead of
//     draining the ring per block.
//   * Whole groups of D blocks run without an exit test: with a `break` inside the unrolled group hipcc cannot count the
//     loads in flight across the back edge and drains them (vmcnt(0)) at every loop head.  The 1 .. D-1 left-over blocks
//     are already in slots 0 .. D-2.
//   * The loads stay above the scheduling barrier: left to itself hipcc sinks them below the block's MFMAs (their
//     destination registers double as MFMA temporaries), which halves the bytes in flight.
template <int D, int S, int BLK = 1024>
struct WeightRing {
    float4 slot[D][S];
    int voff;   // lane * 16: the one loop-invariant VGPR offset (ld_w16)
    __device__ __forceinline__ void load(int st, const __amdgpu_buffer_rsrc_t &rs, const int (&so)[S], int t, int n) {
        const int off = min(t, n - 1) * BLK;
#pragma unroll
        for (int s = 0; s < S; ++s) slot[st][s] = ld_w16(rs, voff, so[s] + off);
    }
    __device__ __forceinline__ void fill(const __amdgpu_buffer_rsrc_t &rs, const int (&so)[S], int n) {
#pragma unroll
        for (int st = 0; st < D - 1; ++st) load(st, rs, so, st, n);
    }
    template <class Pre, class Body>
    __device__ __forceinline__ void run(const __amdgpu_buffer_rsrc_t &rs, const int (&so)[S], int n, Pre &&pre,
                                        Body &&body) {
        const int n_full = (int)((unsigned)n / D * D);   // (n >= 1)
        for (int tt = 0; tt < n_full; tt += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                load((u + D - 1) % D, rs, so, tt + u + D - 1, n);
                pre(tt + u, u);
                __builtin_amdgcn_sched_barrier(0);
                body(tt + u, u, slot[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < D - 1; ++u)
            if (n_full + u < n) {
                pre(n_full + u, u);
                body(n_full + u, u, slot[u]);
            }
    }
};
__device__ __forceinline__ void no_pre(int, int) {}

// LDS layout of a tile body, offsets in floats: x_regions activation regions of x_floats each (two images used
// alternately, or the hi / lo planes of split operands), emb_regions embedding regions of emb_floats each, then
// SX = [pts][3] raw points (+ pad) and RED = [parts][pts] partial sums of the sdf-only last layer.  Each body has one
// function that builds it; the kernel takes its pointers from it and the host its byte count.
struct SdfLds {
    int x1;          // second activation region
    int emb, emb1;   // embedding; its second region
    int sx, red, total;
    __host__ __device__ size_t bytes() const { return sizeof(float) * (size_t)total; }
};
__host__ __device__ inline SdfLds sdf_lds(int pts, int x_regions, int x_floats, int emb_regions, int emb_floats, int parts) {
    SdfLds l;
    l.x1 = (x_regions - 1) * x_floats;
    l.emb = x_regions * x_floats;
    l.emb1 = l.emb + (emb_regions - 1) * emb_floats;
    l.sx = l.emb + emb_regions * emb_floats;
    l.red = l.sx + pts * 4;
    l.total = l.red + parts * pts;
    return l;
}

// the tile's raw points -> SX[p][3], zero beyond cnt
__device__ __forceinline__ void load_points(bool on, float *SX, const float *__restrict__ x, int64_t base, int cnt, int pts,
                                            int tid) {
    if (on && tid < pts * 3) SX[tid] = (tid < cnt * 3) ? x[base * 3 + tid] : 0.0f;
}

// tile of precomputed embedding rows -> EMB[(e/4)][p][e%4] (group stride gf floats), zero padded to 4*egroups columns
__device__ __forceinline__ void load_emb_tile(float *EMB, const float *__restrict__ emb, int64_t stride, int64_t base,
                                              int cnt, int E, int egroups, int pts, int gf, int tid, int nthreads) {
    const int epad = egroups * 4;
    for (int i = tid; i < pts * epad; i += nthreads) {
        const int p = i / epad, e = i - p * epad;
        EMB[(e >> 2) * gf + p * 4 + (e & 3)] = (p < cnt && e < E) ? emb[(base + p) * stride + e] : 0.0f;
    }
}

// nn.Softplus(beta=100, threshold=20): y = x if 100x > 20 else log1p(exp(100x))/100
// evaluated as max(a,0) + ln(1 + 2^(-|z| log2 e)) / 100, z = 100 a, with the native exp2/log2 units (abs error of the
// logarithm term < 1e-9 after the scaling): 9 VALU instructions.  The 1/100 is folded into the log2 -> ln constant: an
// IEEE fp32 division here was a 10-instruction v_div_scale / v_rcp / v_fma / v_div_fixup sequence per activation -
// more than the rest of the function - and the epilogue VALU work is serial with the MFMAs on gfx950.
__device__ __forceinline__ float softplus100(float a) {
    const float z = a * 100.0f;
    const float t = __builtin_amdgcn_exp2f(-fabsf(z) * 1.4426950408889634f);
    const float l = __builtin_amdgcn_logf(1.0f + t) * 0.006931471805599453f;  // v_log_f32 is log2; ln 2 / 100
    const float sp = fmaxf(a, 0.0f) + l;
    return z > 20.0f ? a : sp;
}

// Four activations at once on the packed fp32 VALU ops (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32: two lanes' worth per
// issue slot): 6.5 instead of 11 instructions per activation.  The epilogue is VALU work that cannot overlap the MFMAs
// (in-place activations, workgroup barriers): in the split-operand kernel it costs as many SIMD cycles as the matrix
// products themselves (profiles/r03_split_mfma_pmc.json), in the fp32 kernel ~19 %.  The threshold select of the scalar
// form is dropped: for 100 a > 20 the logarithm term is < 2.1e-11 < half an ulp of a >= 0.2, so max(a, 0) + l == a bit
// for bit - the value nn.Softplus(100, threshold=20) returns.
typedef float f32x2p __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2p softplus100_x2(f32x2p a) {
    const f32x2p na = {-fabsf(a.x), -fabsf(a.y)};
    const f32x2p arg = na * 144.26950408889634f;                       // -|100 a| log2(e)
    f32x2p t = {__builtin_amdgcn_exp2f(arg.x), __builtin_amdgcn_exp2f(arg.y)};
    t = t + 1.0f;
    const f32x2p lg = {__builtin_amdgcn_logf(t.x), __builtin_amdgcn_logf(t.y)};
    const f32x2p mx = {fmaxf(a.x, 0.0f), fmaxf(a.y, 0.0f)};
    return __builtin_elementwise_fma(lg, (f32x2p){0.006931471805599453f, 0.006931471805599453f}, mx);   // ln 2 / 100
}
__device__ __forceinline__ void softplus100_4(float &v0, float &v1, float &v2, float &v3) {
    const f32x2p a = softplus100_x2((f32x2p){v0, v1}), b = softplus100_x2((f32x2p){v2, v3});
    v0 = a.x; v1 = a.y; v2 = b.x; v3 = b.y;
}

// hidden-layer epilogue on register quads that already carry their bias: Softplus(100), then the /sqrt(2) in front of
// the skip layer
constexpr float kSqrt2 = 1.41421356237309515f;
template <int N>
__device__ __forceinline__ void act_quads(float (&v)[N], bool act, bool div) {
    if (act) {
#pragma unroll
        for (int i = 0; i < N; i += 4) softplus100_4(v[i], v[i + 1], v[i + 2], v[i + 3]);
    }
    if (div) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = __fdiv_rn(v[i], kSqrt2);
    }
}
// after layer 0: the skip layer consumes cat[x, emb]/sqrt(2) - rescale the kept embedding (n floats) once, in place
__device__ __forceinline__ void rescale_emb(float *EMB, int n, int tid, int nthreads) {
    for (int i = tid; i < n; i += nthreads) EMB[i] = __fdiv_rn(EMB[i], kSqrt2);
}

// density_net.py:20-30 + implicit_differentiable_renderer.py:112
__device__ __forceinline__ float sdf_clamp(float s, float beta) {
    const float alpha = 1.0f / beta;
    const float sg = (s > 0.0f) ? 1.0f : ((s < 0.0f) ? -1.0f : 0.0f);
    const float rho = alpha * (0.5f + 0.5f * sg * expm1f(-fabsf(s) / beta));
    return tanhf(s / (2.0f + rho));
}

// Sdf-only last layer, second half: every lane that holds a partial dot product has written it to RED[part][pts];
// point tid of the tile = bias[0] + its `parts` partial sums, clamped, -> out[(base + tid) * stride]
__device__ __forceinline__ void sdf_last_finish(const float *RED, int parts, int pts, int cnt,
                                                const float *__restrict__ bias, float beta, float *__restrict__ out,
                                                int64_t base, int64_t stride, int tid) {
    __syncthreads();
    if (tid < cnt) {
        float sacc = bias[0];
        for (int w = 0; w < parts; ++w) sacc += RED[w * pts + tid];
        out[(base + tid) * stride] = sdf_clamp(sacc, beta);
    }
}
// Full-width output stage: X[(f/4)][p][f%4] (gf floats per k-group) -> out[base + p][f], column 0 clamped
__device__ __forceinline__ void store_rows(const float *X, int gf, int cnt, int od, float beta, float *__restrict__ out,
                                           int64_t base, int64_t stride, int tid, int nthreads) {
    for (int i = tid; i < cnt * od; i += nthreads) {
        const int p = i / od, f = i - p * od;
        float v = X[(f >> 2) * gf + p * 4 + (f & 3)];
        if (f == 0) v = sdf_clamp(v, beta);
        out[(base + p) * stride + f] = v;
    }
}

// Encode stage of the fused SDF kernels: the embedding row [x | sin a_c | cos a_c | level features | 0 ... e_pad) of
// the point (x0, x1, x2), written through put(e, v) so that each kernel keeps its own LDS layout.  The row is cut into
// 2L + 1 slots: 0 = pass-through + zero padding, 1..L = Fourier channel slot - 1, L+1..2L = hash level slot - L - 1.
template <class Put>
__device__ __forceinline__ void embed_passthrough(int E, int e_pad, float x0, float x1, float x2, Put &put) {
    put(0, x0); put(1, x1); put(2, x2);
    for (int e = E; e < e_pad; ++e) put(e, 0.0f);
}
template <class Put>
__device__ __forceinline__ void embed_fourier(const float *__restrict__ Bf, int L, int c, float s0, float s1, float s2,
                                              Put &put) {
    float sn, cs;
    sincosf(hm_fourier_arg(Bf, L, c, s0, s1, s2), &sn, &cs);
    put(3 + c, sn);
    put(3 + L + c, cs);
}
// a level's F features -> put(e0 + f, .)  (F == 2, the usual table: no run-time index into acc[])
template <class Put>
__device__ __forceinline__ void put_features(int e0, int F, const float (&acc)[8], Put &put) {
    if (F == 2) {
        put(e0, acc[0]);
        put(e0 + 1, acc[1]);
    } else {
        for (int f = 0; f < F; ++f) put(e0 + f, acc[f]);
    }
}
// the thread owns slots first, first + step, ... of its point (Fourier channels and levels walked separately)
template <int FRAC, class Put>
__device__ __forceinline__ void embed_point(const HmLevels &lv, const float *__restrict__ table,
                                            const float *__restrict__ Bf, float x0, float x1, float x2, int first,
                                            int step, int e_pad, Put &&put) {
    const int L = lv.L;
    if (first == 0) embed_passthrough(lv.E, e_pad, x0, x1, x2, put);
    const float two_pi = 6.283185307179586f;
    const float s0 = __fmul_rn(two_pi, x0), s1 = __fmul_rn(two_pi, x1), s2 = __fmul_rn(two_pi, x2);
    for (int c = first; c < L; c += step) embed_fourier(Bf, L, c, s0, s1, s2, put);
    const int F = lv.F;
    for (int l = first; l < L; l += step) {
        float acc[8];
        hm_level_features<FRAC>(lv, table, l, x0, x1, x2, acc);
        put_features(3 + 2 * L + l * F, F, acc, put);
    }
}

// one slot of the point
template <int FRAC, class Put>
__device__ __forceinline__ void embed_slot(const HmLevels &lv, const float *__restrict__ table,
                                           const float *__restrict__ Bf, float x0, float x1, float x2, int slot,
                                           int e_pad, Put &&put) {
    const int L = lv.L;
    if (slot == 0) {
        embed_passthrough(lv.E, e_pad, x0, x1, x2, put);
    } else if (slot <= L) {
        const float two_pi = 6.283185307179586f;
        embed_fourier(Bf, L, slot - 1, __fmul_rn(two_pi, x0), __fmul_rn(two_pi, x1), __fmul_rn(two_pi, x2), put);
    } else {
        const int l = slot - L - 1, F = lv.F;
        float acc[8];
        hm_level_features<FRAC>(lv, table, l, x0, x1, x2, acc);
        put_features(3 + 2 * L + l * F, F, acc, put);
    }
}

// the thread owns slots 1 + first, 1 + first + step, ... of its point (and slot 0 where first == 0): Fourier channels and
// levels side by side, each on threads of its own where step covers the 2L slots
template <int FRAC, class Put>
__device__ __forceinline__ void embed_slots(const HmLevels &lv, const float *__restrict__ table,
                                            const float *__restrict__ Bf, float x0, float x1, float x2, int first,
                                            int step, int e_pad, Put &&put) {
    if (first == 0) embed_passthrough(lv.E, e_pad, x0, x1, x2, put);
    for (int slot = 1 + first; slot <= 2 * lv.L; slot += step) embed_slot<FRAC>(lv, table, Bf, x0, x1, x2, slot, e_pad, put);
}

// ---- host side ---------------------------------------------------------------------------------------------------
// hm_diag_sdf_lds: the byte offsets of a layout's regions, in order, and its size
static void sdf_lds_report(const SdfLds &l, int32_t *regions) {
    const int f[6] = {l.x1, l.emb, l.emb1, l.sx, l.red, l.total};
    for (int i = 0; i < 6; ++i) regions[i] = 4 * f[i];
}

// the level descriptor of the precomputed-embedding entry points (no grid: only E is read) behind their common check
static int sdf_emb_levels(const char *who, int emb_width, int64_t emb_stride, HmLevels &lv) {
    if (!(emb_width >= 1 && emb_width <= 512 && emb_stride >= emb_width))
        return hm_fail(HM_ERR_INVALID, std::string(who) + ": bad embedding width / stride");
    lv = {};
    lv.L = 0; lv.F = 2; lv.E = emb_width;
    return HM_OK;
}

// the weight image a fused SDF kernel reads from every layer besides the fp32 one (w_packed): the fp32 16-point image
// (w_packed_m16; optional for hm_sdf_fwd, which runs the small tiles only when every layer carries it), the bf16 image or
// the split-operand image
enum SdfImage { kImgM16Optional, kImgM16, kImgBf16, kImgSplit };

// Kernel-side image of the network descriptor + the checks every fused SDF launch makes on it.  The kernel families
// differ in the image they read (img), their minimum layer count, the k-groups of their EMB region (emb_groups:
// 2 ceil(E/8) for the fp32 and bf16 kernels, 4 ceil(E/16) for the split kernel) and whether the last layer may read
// nothing but the previous layer (last_prev_only).  *all_m16: every layer carries w_packed_m16 (kImgM16Optional).
static int sdf_net_from_desc(const char *who, const hm_mlp_desc *mlp, int E, int64_t emb_stride, SdfImage img,
                             int min_layers, int emb_groups, bool last_prev_only, SdfNet &net, bool *all_m16 = nullptr) {
    const auto bad = [who](const char *what) { return hm_fail(HM_ERR_INVALID, std::string(who) + ": " + what); };
    if (!mlp) return bad("NULL descriptor");
    if (mlp->n_layers < min_layers || mlp->n_layers > HM_MAX_LAYERS) return bad("n_layers out of range");
    if (img == kImgSplit && mlp->split_kind != HM_SPLIT_BF16X2 && mlp->split_kind != HM_SPLIT_F16X2)
        return bad("the descriptor carries no split image (split_kind)");
    const int emb_oct = (E + 7) / 8, emb_b16 = (E + 15) / 16;
    net.n_layers = mlp->n_layers;
    net.x_groups = 0;
    net.emb_groups = emb_groups;
    net.beta = mlp->beta;
    net.emb_stride = emb_stride;
    if (all_m16) *all_m16 = true;
    for (int l = 0; l < mlp->n_layers; ++l) {
        const hm_mlp_layer &Ly = mlp->layer[l];
        // the layer's 16-block image (segment lengths in seg_blocks16), if it has the one the kernel reads
        const void *img16 = img == kImgBf16 ? Ly.w_packed_bf16 : img == kImgSplit ? Ly.w_packed_split : Ly.w_packed_m16;
        if (!Ly.w_packed || !Ly.bias) return bad("layer has NULL weights/bias");
        if (!img16 && img != kImgM16Optional) return bad("layer lacks the weight image of this kernel");
        if (!img16 && all_m16) *all_m16 = false;
        // (every kernel has 8 waves of up to 64 output features each)
        if (Ly.n_tiles < 1 || Ly.n_tiles > 16) return bad("layer wider than 512 features");
        if (Ly.out_dim < 1 || Ly.out_dim > Ly.n_tiles * 32) return bad("out_dim / n_tiles mismatch");
        if (Ly.seg_octets[0] < 1 || Ly.seg_octets[1] < 0) return bad("bad segment length");
        for (int s = 0; s < 2; ++s) {
            if (Ly.seg_octets[s] == 0 && !(img16 && Ly.seg_blocks16[s] != 0)) continue;
            if (Ly.seg_src[s] == 1) {
                if (Ly.seg_octets[s] != emb_oct) return bad("embedding segment must span ceil(E/8) octets");
                if (img16 && Ly.seg_blocks16[s] != emb_b16) return bad("embedding segment must span ceil(E/16) 16-blocks");
            } else {
                if (Ly.seg_src[s] != 0 || l == 0)
                    return bad("a segment reads the embedding (1) or, after layer 0, the previous layer (0)");
                const hm_mlp_layer &prev = mlp->layer[l - 1];
                if (Ly.seg_octets[s] * 8 > prev.n_tiles * 32)
                    return bad("layer reads more inputs than the previous layer produces");
                if (Ly.seg_octets[s] * 8 < prev.out_dim)
                    return bad("layer reads fewer inputs than the previous layer produces");
                if (img16 && (Ly.seg_blocks16[s] * 16 > prev.n_tiles * 32 || Ly.seg_blocks16[s] * 16 < prev.out_dim))
                    return bad("16-block segment length does not match the previous layer");
            }
        }
        net.x_groups = max(net.x_groups, Ly.n_tiles * 8);
        net.layer[l] = Ly;
    }
    const hm_mlp_layer &last = mlp->layer[mlp->n_layers - 1];
    if (last_prev_only && (last.seg_octets[1] != 0 || last.seg_src[0] != 0))
        return bad("the last layer must read the previous layer only");
    return HM_OK;
}
