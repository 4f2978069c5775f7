// hm_sdf_tile64.h - the exact-fp32 64-point tile loop (sdf64_run; see hm_sdf.hip for the mapping), shared by
// sdf_fwd_kernel, sdf_scan_secant_kernel and sdf_refine_scan_kernel.  Included inside hm_sdf.hip's anonymous namespace,
// behind hm_sdf_common.h; HM_PROBE / HM_PROBE_WAVES are hm_sdf.hip's phase-probe stamps.
#pragma once
#ifndef HM_PROBE
#define HM_PROBE(i_) do { } while (0)
#define HM_PROBE_WAVES(base_) do { } while (0)
#endif

// third value of the kernels' FRAC template parameter: `x` holds PRECOMPUTED embedding rows (hm_sdf_fwd_emb).  A template
// value rather than a run-time branch on net.emb_stride: with both input paths in one kernel body the register
// allocation of the hash-grid variant changed (178 -> 205 VGPRs, 33 -> 42 spilled SGPRs) and it lost 4 %.
constexpr int kFracEmb = 2;

constexpr int kPts = 64;        // points per workgroup tile
constexpr int kThreadsSdf = 512;
constexpr int kWaves = 8;
constexpr int kGroupFloats = kPts * 4;  // floats per k-group row of X: [point][4]
typedef float f32x4q __attribute__((ext_vector_type(4)));   // accumulator of a 16x16x4 MFMA (quarter tile)

// v_permlane32_swap: lanes 32..63 of a change places with lanes 0..31 of b -> a = (a[0..31] | b[0..31]), b = (a[32..63] |
// b[32..63]), each in lane order
__device__ __forceinline__ void lane32_swap(float &a, float &b) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    a = __uint_as_float(r[0]);
    b = __uint_as_float(r[1]);
}

// dynamic LDS of the 64-point tile: X, the embedding (kept for the skip connection), 8 partial sums per point
__host__ __device__ inline SdfLds sdf_lds64(const SdfNet &net) {
    return sdf_lds(kPts, 1, net.x_groups * kGroupFloats, 1, net.emb_groups * kGroupFloats, kWaves);
}

// Filler tiles.  A launch whose own points end in a partly filled last round can take the 64-point tiles that complete
// the round from a SECOND point set that has to be evaluated anyway (the ray search: the closest-approach scan, whose
// values nothing in the sampler's launches waits for).  Which of that set's tiles a launch takes follows from the
// device-side counts alone, the same way in every launch of the chain: a launch with TA own tiles on G workgroups takes
// pad = (G - TA mod G) mod G filler tiles if that many are still available and it runs on the 64-point kernel at all,
// none otherwise (its remainder then follows the half-tile rule).
struct SdfFill {               // resolved, per launch
    const float *x;
    float *out;
    int64_t n;                 // points of the filler set
    int64_t tile0;             // its first tile that is still free
};
struct SdfFillArgs {           // kernel argument (all zero: no filler)
    const float *x;
    float *out;
    const int32_t *n_dev;      // device-side point count of the filler set
    const int32_t *prev_dev;   // own-point count of the launch that took filler tiles before this one (or NULL)
    int32_t prev_grid;
    int32_t pad_;
};

__device__ __forceinline__ int64_t fill_quota(int64_t n_own, int64_t grid, int64_t avail, int64_t run_min) {
    if (n_own < run_min || grid <= 0) return 0;
    const int64_t ta = (n_own + 63) / 64;
    const int64_t pad = (grid - ta % grid) % grid;
    return (pad > 0 && avail >= pad) ? pad : 0;
}

// The 64-point tile loop of sdf_fwd_kernel / sdf_scan_secant_kernel.  DYN = false: the static schedule below
// (tile = round * grid + workgroup); DYN = true: the SAME tiles in the same enumeration, handed out by an atomic cursor
// (zero at launch) - workgroups that start late (they carried secant rays first) simply take fewer of them.
// QUARTER (no filler set): a launch of at most 16 points per workgroup runs QUARTER tiles of <= 16 points
// on v_mfma_f32_16x16x4_f32 - see the k-loop below; every other count keeps the schedule of QUARTER = false.  With DYN the
// quarter tiles are the static schedule's (tile u = points [16 u, 16 u + 16)), handed out by the cursor.
template <int FRAC, bool DYN, bool QUARTER = false>
__device__ __forceinline__ void sdf64_run(const HmLevels &lv, const SdfNet &net, const float *__restrict__ x, int64_t n,
                                          const float *__restrict__ table, const float *__restrict__ Bf,
                                          float *__restrict__ out, int64_t out_stride, int out_cols, float *lds,
                                          unsigned *cursor, const SdfFill &fb) {
    __shared__ unsigned s_next_tile;
    const SdfLds at = sdf_lds64(net);
    float *X = lds;
    float *EMB = lds + at.emb;
    float *SX = lds + at.sx;     // [64][3] raw points
    float *RED = lds + at.red;   // [8][64] cross-wave partial sums

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform: the weight pointers below stay in SGPRs)
    const int lane = tid & 63;
    const int j = lane & 31;  // point within a 32-point tile / feature row within a 32-feature tile
    const int h = lane >> 5;
    const int m = lane & 15;  // quarter tile: point / feature row within a 16-feature sub-tile
    const int q = lane >> 4;  //               K slot of the 16x16x4 MFMA; feature quad of its result
    const int E = lv.E;
    // Tile schedule: `rounds` full rounds of 64-point tiles (tile = round * grid + workgroup), then ONE remainder tile
    // per workgroup.  When the remainder fits 32 points per workgroup it is cut into 32-point HALF tiles (the MFMAs of
    // the second point block are skipped), so the last round costs about half a round instead of a full one on part of
    // the chip: 204 800 points on 256 CUs are 12 rounds + 256 half tiles instead of 13 rounds on 128 CUs.  A point's
    // value does not depend on the tile it sits in (tests: permutation equivariance bit for bit).
    const int64_t G = gridDim.x;
    // filler tiles (static schedule only): TA own tiles, then tiles fb.tile0 .. of the second set up to the end of the round
    const int64_t TA = (n + kPts - 1) / kPts;
    const int64_t n_fill = DYN ? 0 : fill_quota(n, G, max((fb.n + kPts - 1) / kPts - fb.tile0, (int64_t)0), 0);
    const int64_t rounds = n_fill > 0 ? (TA + n_fill) / G : (n / kPts) / G;
    const int64_t rem_base = rounds * G * kPts;
    // quarter tiles: the whole launch is one remainder round of 16-point tiles
    const bool qt = QUARTER && n_fill == 0 && n <= G * 16;
    const int64_t rem_step = qt ? 16 : (n - rem_base <= G * 32) ? 32 : kPts;

    for (int64_t it = 0;; ++it) {
        int64_t itr = it, wg = blockIdx.x;
        if (DYN) {
            __syncthreads();   // every thread has read the previous hand-out
            if (tid == 0) s_next_tile = atomicAdd(cursor, 1u);
            __syncthreads();
            const int64_t u = s_next_tile;
            itr = u / G;
            wg = u - itr * G;
        }
        if (itr > rounds) break;
        int64_t base;
        int cnt;
        const float *__restrict__ xs = x;       // this tile's point set
        float *__restrict__ os = out;
        if (n_fill > 0) {                        // whole rounds: own tiles (the last one may be ragged), then filler tiles
            if (itr == rounds) break;
            const int64_t v = itr * G + wg;
            if (v < TA) {
                base = v * kPts;
                cnt = (int)min((int64_t)kPts, n - base);
            } else {
                base = (fb.tile0 + (v - TA)) * kPts;
                cnt = (int)min((int64_t)kPts, fb.n - base);
                xs = fb.x;
                os = fb.out;
            }
        } else if (itr < rounds) {
            base = (itr * G + wg) * kPts;
            cnt = kPts;
        } else {
            base = rem_base + wg * rem_step;
            if (base >= n) break;
            cnt = (int)min(rem_step, n - base);
        }
        const bool half = cnt <= 32;   // (also a ragged last tile of <= 32 points)
        HM_PROBE(0);
        __syncthreads();  // previous tile's output stage is done with X
        load_points(FRAC != kFracEmb, SX, xs, base, cnt, kPts, tid);
        __syncthreads();

        // ---------------- encode -> EMB[(e/4)][p][e%4] ------------------------------------
        if constexpr (FRAC == kFracEmb) {
            load_emb_tile(EMB, xs, net.emb_stride, base, cnt, E, net.emb_groups, qt ? 16 : kPts, kGroupFloats, tid,
                          kThreadsSdf);
        } else {
            // (quarter tile: 16 points, so 32 threads share a point's slots; rows 16.. of the image are never read by a
            //  lane whose value is kept)
            const int p = qt ? (tid & 15) : (tid & (kPts - 1));
            const int grp = qt ? (tid >> 4) : (tid >> 6);  // 0..31 / 0..7
            const float x0 = SX[p * 3], x1 = SX[p * 3 + 1], x2 = SX[p * 3 + 2];
            embed_point<FRAC>(lv, table, Bf, x0, x1, x2, grp, qt ? kThreadsSdf / 16 : kWaves, net.emb_groups * 4,
                              [&](int e, float v) { EMB[(e >> 2) * kGroupFloats + p * 4 + (e & 3)] = v; });
        }
        __syncthreads();
        HM_PROBE(1);

        // ---------------- layers ------------------------------------------------------------
        // (a generic lambda: the quarter tile's copy of the layer loop is compiled beside the other two forms', not into
        //  them - with the three k-loops in one loop body the registers of all of them were live together)
        auto run_layers = [&](auto qt_c) {
        constexpr bool QT = decltype(qt_c)::value;
        // weight ring (WeightRing, hm_sdf_common.h: 4 slots, 3 octets = 6 KB per wave in flight); it lives across layers
        WeightRing<4, 2> ring;
        // Quarter tile: the SAME image and the same two 16-byte loads per octet.  Octet g of a 32-feature tile holds, in
        // image lane (feature j, h), W[j][8g + 4h + 0..3], and the 32x32x2 loop below hands an accumulator k = 8g + 0, 4,
        // 1, 5, 2, 6, 3, 7 in that order (component x of h = 0 / 1, then y, z, w).  On 16x16x4 that chain is two MFMAs per
        // octet and 16-feature sub-tile u with K slots (k0, k4, k1, k5) and (k2, k6, k3, k7): lane (row m, slot q) needs
        // components q >> 1 and 2 + (q >> 1) of image lane (16 u + m, h = q & 1) for u = 0 and 1.  It loads image lane
        // (16 (q >> 1) + m, h = q & 1) - every lane another 16 bytes, as in the other forms - and holds the components its
        // partner lane ^ 32 needs of that sub-tile where the partner holds what it needs of the other one:
        // v_permlane32_swap on (x, y) and on (z, w) leaves sub-tile 0's operands of both MFMAs in x / z and sub-tile 1's in
        // y / w.  Four VALU instructions per octet and no load a lane does not use (dword loads of single components,
        // eight per octet, were bound by the texture addresser: 0.43 instead of 0.26 ms for the bench's list).
        ring.voff = QT ? (16 * (q >> 1) + m + 32 * (q & 1)) * 16 : lane * 16;
        bool ring_ready = false;
        auto prefetch64 = [&](int l) {
            const hm_mlp_layer &Lp = net.layer[l];
            const int nop = Lp.seg_octets[0] + Lp.seg_octets[1];
            const int ntp = max(0, min(2, Lp.n_tiles - 2 * wave));
            // descriptor on the wave's first feature tile; the second one is nop KB on
            const __amdgpu_buffer_rsrc_t rs = w_rsrc(Lp.w_packed + ((size_t)(2 * wave) * nop) * 256);
            const int so[2] = {0, ntp > 1 ? nop * 1024 : 0};
            ring.fill(rs, so, nop);
        };
        for (int li = 0; li < net.n_layers; ++li) {
            const hm_mlp_layer &Ly = net.layer[li];
            const int n_oct = Ly.seg_octets[0] + Ly.seg_octets[1];
            if (li == net.n_layers - 1 && out_cols == 1) {
                // sdf-only: one output feature.  A 32-row MFMA tile would idle 7 of 8 waves for a full
                // layer time; instead every wave takes a k-slice of the dot product on the VALU
                // (row 0 of the packed image: tile 0, lanes 0 and 32).
                const float4 *W0 = reinterpret_cast<const float4 *>(Ly.w_packed);
                float part = 0.0f;
                int kg0 = 0;
                for (int seg = 0; seg < 2; ++seg) {
                    const float *src = (Ly.seg_src[seg] == 0) ? X : EMB;
                    const int ng = 2 * Ly.seg_octets[seg];
                    for (int kg = wave; kg < ng; kg += kWaves) {
                        const float4 xv = *reinterpret_cast<const float4 *>(src + kg * kGroupFloats + lane * 4);
                        const int kk = kg0 + kg;
                        const float4 wv = W0[(size_t)(kk >> 1) * 64 + 32 * (kk & 1)];
                        part = __fmaf_rn(xv.x, wv.x, part);
                        part = __fmaf_rn(xv.y, wv.y, part);
                        part = __fmaf_rn(xv.z, wv.z, part);
                        part = __fmaf_rn(xv.w, wv.w, part);
                    }
                    kg0 += ng;
                }
                RED[wave * kPts + lane] = part;
                sdf_last_finish(RED, kWaves, kPts, cnt, Ly.bias, net.beta, os, base, out_stride, tid);
                break;
            }
            const int nt = Ly.n_tiles;
            const int t0 = 2 * wave;
            const int ntw = max(0, min(2, nt - t0));
            f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};
            f32x4q aq[4] = {{0}, {0}, {0}, {0}};      // quarter tile: [feature tile][16-feature sub-tile]
            if constexpr (QT) {
                if (ntw > 0) {
                    const __amdgpu_buffer_rsrc_t rsA = w_rsrc(Ly.w_packed + ((size_t)t0 * n_oct) * 256);
                    const int so[2] = {0, ntw > 1 ? n_oct * 1024 : 0};
                    const int no0 = Ly.seg_octets[0];
                    const float *src0 = ((Ly.seg_src[0] == 0) ? X : EMB) + (q & 1) * kGroupFloats + m * 4 + (q >> 1);
                    const float *src1 = ((Ly.seg_src[1] == 0) ? X : EMB) + (q & 1) * kGroupFloats + m * 4 + (q >> 1);
                    if (!ring_ready) prefetch64(li);
                    ring_ready = false;
                    auto loadBq = [&](int gg, float &b0, float &b1) {
                        const int gc = min(gg, n_oct - 1);
                        const float *src = (gc < no0) ? src0 + 2 * gc * kGroupFloats : src1 + 2 * (gc - no0) * kGroupFloats;
                        b0 = src[0];
                        b1 = src[2];
                    };
                    // (the slot is consumed: x / z become sub-tile 0's operands of the two MFMAs, y / w sub-tile 1's)
                    auto mfma8 = [&](float4 (&w)[2], float b0, float b1) {
#pragma unroll
                        for (int ft = 0; ft < 2; ++ft) {
                            lane32_swap(w[ft].x, w[ft].y);
                            lane32_swap(w[ft].z, w[ft].w);
                        }
                        aq[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[0].x, b0, aq[0], 0, 0, 0);
                        aq[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[0].y, b0, aq[1], 0, 0, 0);
                        aq[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[1].x, b0, aq[2], 0, 0, 0);
                        aq[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[1].y, b0, aq[3], 0, 0, 0);
                        aq[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[0].z, b1, aq[0], 0, 0, 0);
                        aq[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[0].w, b1, aq[1], 0, 0, 0);
                        aq[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[1].z, b1, aq[2], 0, 0, 0);
                        aq[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[1].w, b1, aq[3], 0, 0, 0);
                        // (the next octet's loads stay below: hoisted into this slot's registers while its last MFMAs
                        //  still read them, they cost a copy behind a vmcnt(0) per octet)
                        __builtin_amdgcn_sched_barrier(0);
                    };
                    float bA0, bA1, bB0, bB1;       // B components: even octets in set A, odd octets in set B
                    loadBq(0, bA0, bA1);
                    ring.run(rsA, so, n_oct,
                             [&](int gg, int u) { if (u & 1) loadBq(gg + 1, bA0, bA1); else loadBq(gg + 1, bB0, bB1); },
                             [&](int, int u, float4 (&w)[2]) { if (u & 1) mfma8(w, bB0, bB1); else mfma8(w, bA0, bA1); });
                }
            } else if (ntw > 0) {
                const __amdgpu_buffer_rsrc_t rsA = w_rsrc(Ly.w_packed + ((size_t)t0 * n_oct) * 256);
                const int so[2] = {0, ntw > 1 ? n_oct * 1024 : 0};     // byte offsets of the wave's two feature tiles
                const int no0 = Ly.seg_octets[0];
                const float *src0 = (Ly.seg_src[0] == 0) ? X : EMB;
                const float *src1 = (Ly.seg_src[1] == 0) ? X : EMB;
                if (!ring_ready) prefetch64(li);
                ring_ready = false;
                auto loadB = [&](int gg, float4 &b0, float4 &b1) {
                    const int gc = min(gg, n_oct - 1);
                    const float *src = (gc < no0) ? src0 + (2 * gc + h) * kGroupFloats
                                                  : src1 + (2 * (gc - no0) + h) * kGroupFloats;
                    b0 = *reinterpret_cast<const float4 *>(src + j * 4);
                    b1 = *reinterpret_cast<const float4 *>(src + (32 + j) * 4);
                };
                auto mfma16 = [&](const float4 &a0, const float4 &a1, const float4 &b0, const float4 &b1) {
                    acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b0.x, acc00, 0, 0, 0);
                    acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b1.x, acc01, 0, 0, 0);
                    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b0.x, acc10, 0, 0, 0);
                    acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b1.x, acc11, 0, 0, 0);
                    acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b0.y, acc00, 0, 0, 0);
                    acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b1.y, acc01, 0, 0, 0);
                    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b0.y, acc10, 0, 0, 0);
                    acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b1.y, acc11, 0, 0, 0);
                    acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b0.z, acc00, 0, 0, 0);
                    acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b1.z, acc01, 0, 0, 0);
                    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b0.z, acc10, 0, 0, 0);
                    acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b1.z, acc11, 0, 0, 0);
                    acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b0.w, acc00, 0, 0, 0);
                    acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b1.w, acc01, 0, 0, 0);
                    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b0.w, acc10, 0, 0, 0);
                    acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b1.w, acc11, 0, 0, 0);
                };
                // (full tiles request the B fragments of octet gg + 1 before octet gg's MFMAs - two register sets, loadB / mfma16:
                //  with the ds_reads behind the scheduling barrier of their own octet every octet starts with an exposed
                //  LDS round trip.  Alone this changed nothing - one wave's k-loop 62.4 -> 54.2 us per layer, but then 11 us
                //  at the barrier, scripts/sdf_phase_probe.py; on top of the buffer-load weight stream: 132.0 -> 134.2
                //  TFLOP/s)
                // half tile: the same stream, point block 0 only (8 MFMAs per octet)
                auto octet_h = [&](int gg, const float4 &a0, const float4 &a1) {
                    const float *src = (gg < no0) ? src0 + (2 * gg + h) * kGroupFloats
                                                  : src1 + (2 * (gg - no0) + h) * kGroupFloats;
                    const float4 b0 = *reinterpret_cast<const float4 *>(src + j * 4);
                    acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b0.x, acc00, 0, 0, 0);
                    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b0.x, acc10, 0, 0, 0);
                    acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b0.y, acc00, 0, 0, 0);
                    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b0.y, acc10, 0, 0, 0);
                    acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b0.z, acc00, 0, 0, 0);
                    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b0.z, acc10, 0, 0, 0);
                    acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b0.w, acc00, 0, 0, 0);
                    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b0.w, acc10, 0, 0, 0);
                };
                if (!half) {
                    float4 bA0, bA1, bB0, bB1;      // B fragments: even octets in set A, odd octets in set B
                    loadB(0, bA0, bA1);
                    ring.run(rsA, so, n_oct,
                             [&](int gg, int u) { if (u & 1) loadB(gg + 1, bA0, bA1); else loadB(gg + 1, bB0, bB1); },
                             [&](int, int u, const float4 (&w)[2]) {
                                 if (u & 1) mfma16(w[0], w[1], bB0, bB1); else mfma16(w[0], w[1], bA0, bA1);
                             });
                } else {
                    ring.run(rsA, so, n_oct, no_pre, [&](int gg, int, const float4 (&w)[2]) { octet_h(gg, w[0], w[1]); });
                }
            }
            if (li + 1 < net.n_layers && !(li + 1 == net.n_layers - 1 && out_cols == 1) &&
                net.layer[li + 1].n_tiles - 2 * wave > 0) {
                prefetch64(li + 1);
                ring_ready = true;
            }
            HM_PROBE(2 + 4 * li);
            HM_PROBE_WAVES(64);
            __syncthreads();  // every wave has finished reading X / EMB for this layer
            HM_PROBE(3 + 4 * li);
            HM_PROBE_WAVES(72);

            // epilogue: registers 4q..4q+3 of a tile = features 8q+4h+{0..3} = one k-group of the next layer
            const bool act = Ly.activation != 0;
            const bool div = Ly.post_div_sqrt2 != 0;
            auto store_tile = [&](const f32x16 &acc, int ft, int pt) {
                const int fbase = 32 * (t0 + ft);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int f = fbase + 8 * q + 4 * h;
                    const float4 bb = *reinterpret_cast<const float4 *>(Ly.bias + f);
                    float v[4] = {acc[4 * q + 0] + bb.x, acc[4 * q + 1] + bb.y, acc[4 * q + 2] + bb.z, acc[4 * q + 3] + bb.w};
                    act_quads(v, act, div);
                    *reinterpret_cast<float4 *>(X + (f >> 2) * kGroupFloats + (32 * pt + j) * 4) =
                        make_float4(v[0], v[1], v[2], v[3]);
                }
            };
            // quarter tile: registers 0..3 of sub-tile a = features 16 a + 4q + {0..3} of the wave's tiles, point m
            auto store_quarter = [&](const f32x4q &acc, int a) {
                const int f = 32 * t0 + 16 * a + 4 * q;
                const float4 bb = *reinterpret_cast<const float4 *>(Ly.bias + f);
                float v[4] = {acc[0] + bb.x, acc[1] + bb.y, acc[2] + bb.z, acc[3] + bb.w};
                act_quads(v, act, div);
                *reinterpret_cast<float4 *>(X + (f >> 2) * kGroupFloats + m * 4) = make_float4(v[0], v[1], v[2], v[3]);
            };
            if constexpr (QT) {
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    if (a < 2 * ntw) store_quarter(aq[a], a);
            } else {
                if (ntw > 0) {
                    store_tile(acc00, 0, 0);
                    if (!half) store_tile(acc01, 0, 1);
                }
                if (ntw > 1) {
                    store_tile(acc10, 1, 0);
                    if (!half) store_tile(acc11, 1, 1);
                }
            }
            if (li == 0 && net.emb_groups > 0) rescale_emb(EMB, net.emb_groups * kGroupFloats, tid, kThreadsSdf);
            HM_PROBE(4 + 4 * li);
            __syncthreads();
            HM_PROBE(5 + 4 * li);
        }
        };
        if (QUARTER && qt) run_layers(std::true_type{});
        else run_layers(std::false_type{});
        HM_PROBE(100);

        // ---------------- output: X[(f/4)][p][f%4] -> out[p][f] -----------------------------
        const hm_mlp_layer &last = net.layer[net.n_layers - 1];
        if (out_cols != 1) store_rows(X, kGroupFloats, cnt, last.out_dim, net.beta, os, base, out_stride, tid, kThreadsSdf);
    }
}
