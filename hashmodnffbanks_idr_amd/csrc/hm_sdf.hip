// hm_sdf.hip - fused no-grad SDF network forward for gfx950: hash-grid encode + all MLP layers
// + tanh/Laplace clamp in ONE kernel; activations never leave the CU.
//
// Replaces ImplicitNetwork.forward under torch.no_grad()
// (reference: model/implicit_differentiable_renderer.py:89-113, density_net.py:20-30) - the
// callable RayTracing evaluates ~123 times per ray.
//
// Mapping (MI355X-first, not a GEMM-library call chain):
//   * a workgroup (8 waves, 512 threads, 1 per CU) owns a tile of 64 points for ALL layers;
//   * activations live in LDS as X[k/4][point][4] (fp32, 16-B k-groups), 128 KB + the embedding
//     (kept for the skip connection) 18 KB  -> 146 KB of the CU's 160 KB;
//   * each layer is D^T[feature, point] = W[feature, k] * X[k, point] on v_mfma_f32_32x32x2_f32
//     (exact fp32, k-ordered fma chain): W is the A operand streamed straight from L2 into
//     registers as coalesced 1-KB dwordx4 wave loads of a pre-packed image (each wave owns 64
//     output features, so weights are never shared between waves and LDS staging would be pure
//     overhead); X is the B operand read with conflict-free ds_read_b128;
//   * the accumulator tile has the point on the lane and 4 consecutive features per register
//     quad, i.e. exactly one 16-B k-group of the NEXT layer: the epilogue (bias, Softplus(100),
//     optional /sqrt(2)) writes it back with ds_write_b128 - no transpose, no shuffles.
// Small batches (the ray search issues ~30 dependent calls of 1...4096 points per iteration) use 16-, 8- and
// 4-point tiles so that every call is ONE tile per CU; the tile size is chosen on the device from the live
// point count (sdf_fwd_small_kernel -> sdf_small_body<Tile16 | Tile8<8> | Tile8<4>>).
// The stages all tile bodies share - point load, weight stream (WeightRing), quad epilogue, embedding rescale, last-layer
// finish, output rows, LDS layout (SdfLds) - are in hm_sdf_common.h; sdf64_run (hm_sdf_tile64.h) is the 64-point body.
#include "hm_common.h"
#include "hm_trace_host.h"   // the ray search's entries into this file

#include <math.h>
#include <stdlib.h>

namespace {

#include "hm_sdf_common.h"
#include "hm_trace_dev.h"   // the ray search's state machine, run by the persistent march kernel below

#ifdef HM_SDF_PHASE_PROBE
// scripts/sdf_phase_probe.py: cycle stamps of one tile's phases (workgroup 0, wave 0, second tile), never in the product build
__device__ unsigned long long hm_probe_ts[128];
#define HM_PROBE(i_)                                                                                  \
    do {                                                                                              \
        if (blockIdx.x == 0 && threadIdx.x == 0 && it == 1 && (i_) < 120) hm_probe_ts[(i_)] = wall_clock64(); \
        if (blockIdx.x == 0 && threadIdx.x == 0 && it == 1 && ((i_) == 0 || (i_) == 100))                 \
            hm_probe_ts[120 + ((i_) != 0)] = clock64();   /* shader-clock cycles over the same tile */      \
    } while (0)
// every wave's own stamp (lane 0) at the end of layer 2's k-loop -> ts[64 + wave], after its first barrier -> ts[72 + wave]
#define HM_PROBE_WAVES(base_)                                                                                  \
    do {                                                                                                       \
        if (blockIdx.x == 0 && (threadIdx.x & 63) == 0 && it == 1 && li == 2) hm_probe_ts[(base_) + (threadIdx.x >> 6)] = wall_clock64(); \
    } while (0)
// small-tile bodies: workgroup 0 / thread 0 stamps of its first tile -> ts[i]
#define HM_PROBE_S(i_)                                                                                \
    do {                                                                                              \
        if (blockIdx.x == 0 && threadIdx.x == 0 && (i_) < 120) hm_probe_ts[(i_)] = wall_clock64();   \
    } while (0)
#else
#define HM_PROBE(i_) do { } while (0)
#define HM_PROBE_WAVES(base_) do { } while (0)
#define HM_PROBE_S(i_) do { } while (0)
#endif

#include "hm_sdf_tile64.h"        // sdf64_run: the 64-point fp32 tile body
#include "hm_sdf_split_tile.h"    // sdf_split_tile: the 64-point f16x2 / bf16x2 tile body (sdf_refine_scan_kernel)
#include "hm_scan_pool.h"         // scan_pool_quota: the closest-approach scan's tiles per launch of the guarded search

// ... of the small tiles (pts = 16 or 8 points in the LDS image): two activation images + the embedding in whole
// 16-blocks.  (The 8-point layout needs half of the 16-point one, which is what every launch asks for.)
__host__ __device__ inline SdfLds sdf_lds_small(const SdfNet &net, int E, int pts) {
    return sdf_lds(pts, 2, net.x_groups * pts * 4, 1, (E + 15) / 16 * 4 * pts * 4, kWaves);
}

// QUARTER: the launch with quarter tiles enabled (HM_SDF_TILE64_QUARTER) - a kernel of its own, so that the third tile
// form costs the launches without it nothing
template <int FRAC, bool QUARTER>
__global__ __launch_bounds__(kThreadsSdf, 2) void sdf_fwd_kernel(HmLevels lv, SdfNet net,
                                                                  const float *__restrict__ x, int64_t n,
                                                                  const float *__restrict__ table,
                                                                  const float *__restrict__ Bf,
                                                                  float *__restrict__ out, int64_t out_stride,
                                                                  int out_cols, const int32_t *__restrict__ n_dev, int64_t run_min,
                                                                  int64_t run_max, SdfFillArgs fa) {
    extern __shared__ __align__(16) float lds[];
    if (n_dev) n = min(n, (int64_t)max(*n_dev, 0));  // device-side point count (sync-free callers)
    if (n < run_min || n > run_max) return;          // the other tile-size kernel owns this batch size
    SdfFill fb = {nullptr, nullptr, 0, 0};
    if (fa.n_dev) {
        fb.x = fa.x;
        fb.out = fa.out;
        fb.n = max(*fa.n_dev, 0);
        if (fa.prev_dev)
            fb.tile0 = fill_quota(max(*fa.prev_dev, 0), fa.prev_grid, (fb.n + kPts - 1) / kPts, run_min);
    }
    sdf64_run<FRAC, false, QUARTER>(lv, net, x, n, table, Bf, out, out_stride, out_cols, lds, nullptr, fb);
}


// ------------------------------------------------------------------------------------------------
// Small tiles for SMALL batches (sphere-tracing rounds evaluate only 2 points per ray): with 64-point tiles a
// 4096-point call occupies 64 of the 256 CUs for a full 9-layer latency.  sdf_small_body is the tile loop and layer
// skeleton of the 16-, 8- and 4-point forms; a Tile (Tile16, Tile8<8>, Tile8<4>) supplies what differs: the MFMA block of
// one 16-wide k-block, the reduction over k quarters of the 8-point form, the epilogue's lane -> (feature quad, point)
// mapping and the lane mapping of the sdf-only last layer.  Every wave owns 4 feature tiles of 16.
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kPts16 = 16;
constexpr int kRing16 = 4;   // weight ring depth of the 16-point tile (k-blocks)
constexpr int kPts8 = 8;
constexpr int kRing8 = 5;    // weight ring depth of the 8-point tile (k-blocks)

// 16-point tile: a workgroup owns 16 points (v_mfma_f32_16x16x4_f32), so a 4096-point call spreads over 256
// workgroups; the price is 4x the weight traffic per point, which L2 absorbs at this size.  Same LDS image
// X[k/4][point][4] (64 floats per k-group), same epilogue identity as the 64-point tile: lane (point j, quarter q) holds
// features 4q..4q+3 of a tile = one k-group.
struct Tile16 {
    static constexpr int kTile = 16, kStride = 16, kDepth = kRing16, kGF = 64;
    static_assert(kDepth % 2 == 0, "the B double buffer alternates with the parity of the block in the group");
    int j, q;      // point; k quarter / feature quarter
    f32x4 acc[4];
    __device__ __forceinline__ Tile16(int lane) : j(lane & 15), q(lane >> 4) {}
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    // acc = W[this wave's tiles][k-blocks 0 .. nb) * X.  A small batch is bound by the round trip of the packed weights
    // (7.9 MB per workgroup, served from the Infinity Cache at ~2 us), not by the MFMAs: bytes in flight per CU set the
    // rate - kDepth-1 k-blocks of 4 KB per wave.
    __device__ __forceinline__ void products(WeightRing<kDepth, 4> &ring, const __amdgpu_buffer_rsrc_t &rA,
                                             const int (&so)[4], int nb, int nb0, const float *src0, const float *src1) {
        // B fragment of k-block t (LDS), requested one block ahead of its MFMAs (two registers sets, as in the
        // 64-point kernel)
        auto loadB16 = [&](int t) -> float4 {
            const int tc = min(t, nb - 1);
            const float *src = (tc < nb0) ? src0 + (4 * tc + q) * kGF : src1 + (4 * (tc - nb0) + q) * kGF;
            return *reinterpret_cast<const float4 *>(src + j * 4);
        };
        auto block16 = [&](const float4 &b, const float4 (&w)[4]) {
            // component-major order: four INDEPENDENT accumulators between two uses of the same one
#pragma unroll
            for (int a = 0; a < 4; ++a) acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[a].x, b.x, acc[a], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < 4; ++a) acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[a].y, b.y, acc[a], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < 4; ++a) acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[a].z, b.z, acc[a], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < 4; ++a) acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[a].w, b.w, acc[a], 0, 0, 0);
        };
        float4 bE = loadB16(0), bO;      // even / odd blocks (kDepth is even: block t has the parity of u)
        ring.run(rA, so, nb, [&](int t, int u) { if (u & 1) bE = loadB16(t + 1); else bO = loadB16(t + 1); },
                 [&](int, int u, const float4 (&w)[4]) { if (u & 1) block16(bO, w); else block16(bE, w); });
    }
    __device__ __forceinline__ void reduce() {}
    // bias (bias64: the wave's 64 bias floats in LDS, see sdf_small_body), activation and store of the wave's ntw feature
    // tiles (first: u0) -> Xn.  bias64 lies in the part of Xn this epilogue fills: every quad is read before the first store.
    __device__ __forceinline__ void epilogue(const float *bias64, int u0, int ntw, bool act, bool div, float *Xn) {
        if (ntw <= 0) return;
        float4 bq[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) bq[a] = *reinterpret_cast<const float4 *>(bias64 + 16 * a + 4 * q);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            if (a >= ntw) continue;
            const int f = 16 * (u0 + a) + 4 * q;
            const float4 bb = bq[a];
            float v[4] = {acc[a][0] + bb.x, acc[a][1] + bb.y, acc[a][2] + bb.z, acc[a][3] + bb.w};
            act_quads(v, act, div);
            *reinterpret_cast<float4 *>(Xn + (f >> 2) * kGF + j * 4) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
    // sdf-only last layer: VALU dot product, lane (point j, quarter q) walks k-groups == q (mod 4); partial sums -> RED
    __device__ __forceinline__ void last_layer(const hm_mlp_layer &Ly, const float *X, const float *EMB, int wave, int lane,
                                               float *RED) {
        const float4 *W0 = reinterpret_cast<const float4 *>(Ly.w_packed_m16);
        float part = 0.0f;
        int t0 = 0;
        for (int seg = 0; seg < 2; ++seg) {
            const float *src = (Ly.seg_src[seg] == 0) ? X : EMB;
            const int nbs = Ly.seg_blocks16[seg];
            for (int t = wave; t < nbs; t += kWaves) {
                const float4 xv = *reinterpret_cast<const float4 *>(src + (4 * t + q) * kGF + j * 4);
                const float4 wv = W0[(size_t)(t0 + t) * 64 + q * 16];
                part = __fmaf_rn(xv.x, wv.x, part);
                part = __fmaf_rn(xv.y, wv.y, part);
                part = __fmaf_rn(xv.z, wv.z, part);
                part = __fmaf_rn(xv.w, wv.w, part);
            }
            t0 += nbs;
        }
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        if (q == 0) RED[wave * kPts16 + j] = part;
    }
};

// 8-point tiles for the smallest batches (late sphere-tracing rounds, secant steps: <= 2048 live points).
// A 16-point tile costs the same MFMA time however few of its points are live (8 x 13.6 us per network on
// one CU); with 8 points per workgroup the matrix work halves and the call is bound by the weight stream
// alone.  v_mfma_f32_4x4x1_16b_f32 computes 16 independent 4x4 outer products: lane l = 16q + j supplies
//   A = W[16u + j][k]  (k in quarter q of the 16-wide k-block: the SAME packed image as the 16-point kernel)
//   B = X[point l & 3][k]
// and block (q, j / 4) accumulates, for its four features and four points, the partial sum over the k of
// quarter q; the four quarters are added with two lane exchanges at the end of the layer, which also hand
// each lane exactly one (feature quad, point) of the next layer's X image.
// PTS = 8: two point groups per tile; PTS = 4: one (<= 1024 live points: the second group's MFMAs are skipped,
// the LDS image keeps its 8-point stride)
template <int PTS>
struct Tile8 {
    // (a ring one block deeper for the 4-point variant measured the same: 94 vs 93 us)
    static constexpr int kTile = PTS, kStride = kPts8, kDepth = kRing8, kGF = 32;
    static constexpr bool TWO = PTS == 8;
    int q, jj, p4;            // k quarter of the A operand; feature quad within the 16-feature tile; point within a group of four
    f32x4 acc0[4], acc1[4];   // points 0-3 / 4-7
    f32x4 r0, r1;             // the lane's complete sums after reduce()
    __device__ __forceinline__ Tile8(int lane) : q(lane >> 4), jj((lane & 15) >> 2), p4(lane & 3) {}
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            acc0[a] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            acc1[a] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
    }
    __device__ __forceinline__ void products(WeightRing<kDepth, 4> &ring, const __amdgpu_buffer_rsrc_t &rA,
                                             const int (&so)[4], int nb, int nb0, const float *src0, const float *src1) {
        ring.run(rA, so, nb, no_pre, [&](int t, int, const float4 (&w)[4]) {
            const float *src = (t < nb0) ? src0 + (4 * t + q) * kGF : src1 + (4 * (t - nb0) + q) * kGF;
            const float4 b0 = *reinterpret_cast<const float4 *>(src + p4 * 4);
            const float4 b1 = TWO ? *reinterpret_cast<const float4 *>(src + (p4 + 4) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const float4 av = w[a];
                acc0[a] = __builtin_amdgcn_mfma_f32_4x4x1f32(av.x, b0.x, acc0[a], 0, 0, 0);
                if (TWO) acc1[a] = __builtin_amdgcn_mfma_f32_4x4x1f32(av.x, b1.x, acc1[a], 0, 0, 0);
                acc0[a] = __builtin_amdgcn_mfma_f32_4x4x1f32(av.y, b0.y, acc0[a], 0, 0, 0);
                if (TWO) acc1[a] = __builtin_amdgcn_mfma_f32_4x4x1f32(av.y, b1.y, acc1[a], 0, 0, 0);
                acc0[a] = __builtin_amdgcn_mfma_f32_4x4x1f32(av.z, b0.z, acc0[a], 0, 0, 0);
                if (TWO) acc1[a] = __builtin_amdgcn_mfma_f32_4x4x1f32(av.z, b1.z, acc1[a], 0, 0, 0);
                acc0[a] = __builtin_amdgcn_mfma_f32_4x4x1f32(av.w, b0.w, acc0[a], 0, 0, 0);
                if (TWO) acc1[a] = __builtin_amdgcn_mfma_f32_4x4x1f32(av.w, b1.w, acc1[a], 0, 0, 0);
            }
        });
    }
    // add the four k quarters; lane q ends up with the complete sums of feature tile a == q
    // (exchange across lane bit 5 keeps tiles {0,1} or {2,3}, across bit 4 keeps one of the pair)
    __device__ __forceinline__ void reduce() {
        const bool hi2 = (q & 2) != 0, hi1 = (q & 1) != 0;
        f32x4 k0[2], k1[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float keep0 = hi2 ? acc0[a + 2][r] : acc0[a][r], send0 = hi2 ? acc0[a][r] : acc0[a + 2][r];
                const float keep1 = hi2 ? acc1[a + 2][r] : acc1[a][r], send1 = hi2 ? acc1[a][r] : acc1[a + 2][r];
                k0[a][r] = keep0 + __shfl_xor(send0, 32);
                k1[a][r] = TWO ? keep1 + __shfl_xor(send1, 32) : 0.0f;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float keep0 = hi1 ? k0[1][r] : k0[0][r], send0 = hi1 ? k0[0][r] : k0[1][r];
            const float keep1 = hi1 ? k1[1][r] : k1[0][r], send1 = hi1 ? k1[0][r] : k1[1][r];
            r0[r] = keep0 + __shfl_xor(send0, 16);
            r1[r] = TWO ? keep1 + __shfl_xor(send1, 16) : 0.0f;
        }
    }
    // (Tile16::epilogue: the lane's one quad of bias64 is read before its stores)
    __device__ __forceinline__ void epilogue(const float *bias64, int u0, int ntw, bool act, bool div, float *Xn) {
        if (q < ntw) {
            const int f = 16 * (u0 + q) + 4 * jj;
            const float4 bb = *reinterpret_cast<const float4 *>(bias64 + 16 * q + 4 * jj);
            float v[8] = {r0[0] + bb.x, r0[1] + bb.y, r0[2] + bb.z, r0[3] + bb.w,
                          r1[0] + bb.x, r1[1] + bb.y, r1[2] + bb.z, r1[3] + bb.w};
            act_quads(v, act, div);
            float *dst = Xn + (f >> 2) * kGF;
            *reinterpret_cast<float4 *>(dst + p4 * 4) = make_float4(v[0], v[1], v[2], v[3]);
            if (TWO) *reinterpret_cast<float4 *>(dst + (p4 + 4) * 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
    }
    // sdf-only last layer: VALU dot product.  lane -> (point, k quarter, block parity); partial sums -> RED
    __device__ __forceinline__ void last_layer(const hm_mlp_layer &Ly, const float *X, const float *EMB, int wave, int lane,
                                               float *RED) {
        const float4 *W0 = reinterpret_cast<const float4 *>(Ly.w_packed_m16);
        const int pp = lane & 7, qq = (lane >> 3) & 3, th = lane >> 5;
        float part = 0.0f;
        int t0 = 0;
        for (int seg = 0; seg < 2; ++seg) {
            const float *src = (Ly.seg_src[seg] == 0) ? X : EMB;
            const int nbs = Ly.seg_blocks16[seg];
            for (int t = 2 * wave + th; t < nbs; t += 2 * kWaves) {
                const float4 xv = *reinterpret_cast<const float4 *>(src + (4 * t + qq) * kGF + pp * 4);
                const float4 wv = W0[(size_t)(t0 + t) * 64 + qq * 16];
                part = __fmaf_rn(xv.x, wv.x, part);
                part = __fmaf_rn(xv.y, wv.y, part);
                part = __fmaf_rn(xv.z, wv.z, part);
                part = __fmaf_rn(xv.w, wv.w, part);
            }
            t0 += nbs;
        }
        part += __shfl_xor(part, 8);
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        if (lane < kPts8) RED[wave * kPts8 + lane] = part;
    }
};

template <int FRAC, class Tile>
__device__ __forceinline__ void sdf_small_body(const HmLevels &lv, const SdfNet &net, const float *__restrict__ x,
                                               int64_t n, const float *__restrict__ table,
                                               const float *__restrict__ Bf, float *__restrict__ out,
                                               int64_t out_stride, int out_cols, float *lds, int64_t tile_first,
                                               int64_t tile_step) {
    constexpr int PTS = Tile::kTile, ST = Tile::kStride, GF = Tile::kGF;   // live points; points / floats per k-group of the LDS image
    const int emb_groups16 = ((lv.E + 15) / 16) * 4;
    // two activation images, used alternately (layer l reads one, its epilogue writes the other): no barrier between a
    // layer's k-loop and its epilogue - a wave that finishes early does not wait for the others before its Softplus
    const SdfLds at = sdf_lds_small(net, lv.E, ST);
    float *X0 = lds;
    float *X1 = lds + at.x1;
    float *EMB = lds + at.emb;
    float *RED = lds + at.red;   // [8 waves][ST]

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform: descriptors / scalar offsets of the weight stream)
    const int lane = tid & 63;
    const int E = lv.E;
    Tile tl(lane);
    const int64_t n_tiles = (n + PTS - 1) / PTS;

    for (int64_t tile = tile_first; tile < n_tiles; tile += tile_step) {
        const int64_t base = tile * PTS;
        const int cnt = (int)min((int64_t)PTS, n - base);
        HM_PROBE_S(0);
        float *X = X0, *Xn = X1;     // X: the image the current layer reads; Xn: the one its epilogue fills
        __syncthreads();   // the workgroup is done with its previous tile

        // ---- encode: thread -> (point p, slot group c0); the 512 / ST groups walk the Fourier channels and the levels side
        // by side (embed_slots).  The lanes of a point read its 12 bytes themselves: no staging in LDS, no barrier
        if constexpr (FRAC == kFracEmb) {
            load_emb_tile(EMB, x, net.emb_stride, base, cnt, E, emb_groups16, PTS, GF, tid, kThreadsSdf);
        } else {
            const int p = tid & (ST - 1);
            const int c0 = tid / ST;
            const float *xp = x + (base + min(p, cnt - 1)) * 3;      // (zero beyond cnt)
            const float x0 = p < cnt ? xp[0] : 0.0f, x1 = p < cnt ? xp[1] : 0.0f, x2 = p < cnt ? xp[2] : 0.0f;
            embed_slots<FRAC>(lv, table, Bf, x0, x1, x2, c0, kThreadsSdf / ST, emb_groups16 * 4,
                              [&](int e, float v) { EMB[(e >> 2) * GF + p * 4 + (e & 3)] = v; });
        }
        __syncthreads();
        HM_PROBE_S(1);

        // weight ring (WeightRing, hm_sdf_common.h); streams: the wave's four 16-feature tiles, clamped to the live ones
        WeightRing<Tile::kDepth, 4> ring;
        ring.voff = lane * 16;
        bool ring_ready = false;
        auto prefetch = [&](int l) {
            const hm_mlp_layer &Lp = net.layer[l];
            const int nbp = Lp.seg_blocks16[0] + Lp.seg_blocks16[1];
            const int ntp = max(0, min(4, Lp.n_tiles * 2 - 4 * wave));
            const __amdgpu_buffer_rsrc_t rp = w_rsrc(Lp.w_packed_m16 + ((size_t)(4 * wave) * nbp) * 256);
            const int ts = nbp * 1024;     // bytes to the next feature tile
            const int so[4] = {0, (1 < ntp ? 1 : 0) * ts, (2 < ntp ? 2 : 0) * ts, (3 < ntp ? 3 : 0) * ts};
            ring.fill(rp, so, nbp);
        };
        // The epilogue's bias: the wave's 64 floats (its four feature tiles, clamped into the padded bias [nt16][16]), one per
        // lane, requested a layer ahead - in front of the encode / of the previous layer's epilogue - so that no layer waits
        // for a round trip to memory behind its k-loop.  The lanes exchange them through LDS (bias64, below).
        const auto mfma_layer = [&](int l) { return l < net.n_layers && !(l == net.n_layers - 1 && out_cols == 1); };
        const auto wave_bias = [&](int l) {
            const hm_mlp_layer &Lb = net.layer[l];
            return Lb.bias[min(64 * wave + lane, 32 * Lb.n_tiles - 1)];
        };
        float bias_nx = mfma_layer(0) ? wave_bias(0) : 0.0f;
        for (int li = 0; li < net.n_layers; ++li) {
            const hm_mlp_layer &Ly = net.layer[li];
            if (li == net.n_layers - 1 && out_cols == 1) {
                tl.last_layer(Ly, X, EMB, wave, lane, RED);
                sdf_last_finish(RED, kWaves, ST, cnt, Ly.bias, net.beta, out, base, out_stride, tid);
                break;
            }
            const int nb = Ly.seg_blocks16[0] + Ly.seg_blocks16[1];  // 16-wide k blocks
            const int nt16 = Ly.n_tiles * 2;
            const int u0 = 4 * wave;
            const int ntw = max(0, min(4, nt16 - u0));
            tl.zero();
            // bias64: the first 64 floats of the part of Xn that this wave alone fills (feature tile u0).  Nobody else reads or
            // writes them before the barrier behind the epilogue, which reads its quads before its first store.
            float *bias64 = Xn + 4 * u0 * GF;
            if (ntw > 0) {
                bias64[lane] = bias_nx;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            if (ntw > 0) {
                const __amdgpu_buffer_rsrc_t rA = w_rsrc(Ly.w_packed_m16 + ((size_t)u0 * nb) * 256);
                const int tstride = nb * 1024;  // bytes to the next feature tile
                const int so[4] = {0, (1 < ntw ? 1 : 0) * tstride, (2 < ntw ? 2 : 0) * tstride, (3 < ntw ? 3 : 0) * tstride};
                const float *src0 = (Ly.seg_src[0] == 0) ? X : EMB;
                const float *src1 = (Ly.seg_src[1] == 0) ? X : EMB;
                if (!ring_ready) prefetch(li);
                ring_ready = false;
                tl.products(ring, rA, so, nb, Ly.seg_blocks16[0], src0, src1);
            }
            // request the next layer's first blocks now: they travel while this layer's epilogue and the two
            // barriers run (weights do not depend on the activations)
            if (mfma_layer(li + 1)) {
                if (2 * net.layer[li + 1].n_tiles - 4 * wave > 0) {
                    bias_nx = wave_bias(li + 1);
                    prefetch(li + 1);
                    ring_ready = true;
                }
            }
            HM_PROBE_S(2 + 4 * li);
            tl.reduce();
            HM_PROBE_S(3 + 4 * li);
            if (li == 0) __syncthreads();   // (layer 0 only: its epilogue rescales EMB in place, which every wave has read)
            HM_PROBE_S(4 + 4 * li);
            tl.epilogue(bias64, u0, ntw, Ly.activation != 0, Ly.post_div_sqrt2 != 0, Xn);
            if (li == 0) rescale_emb(EMB, emb_groups16 * GF, tid, kThreadsSdf);
            HM_PROBE_S(40 + li);
            __syncthreads();
            { float *t_ = X; X = Xn; Xn = t_; }
            HM_PROBE_S(5 + 4 * li);
        }
        HM_PROBE_S(100);

        const hm_mlp_layer &last = net.layer[net.n_layers - 1];
        if (out_cols != 1) store_rows(X, GF, cnt, last.out_dim, net.beta, out, base, out_stride, tid, kThreadsSdf);
    }
}

// small batches: one launch, the tile size is chosen on the device from the live point count
template <int FRAC>
__global__ __launch_bounds__(kThreadsSdf, 1) void sdf_fwd_small_kernel(HmLevels lv, SdfNet net,
                                                                        const float *__restrict__ x, int64_t n,
                                                                        const float *__restrict__ table,
                                                                        const float *__restrict__ Bf,
                                                                        float *__restrict__ out, int64_t out_stride,
                                                                        int out_cols, const int32_t *__restrict__ n_dev,
                                                                        int64_t run_min, int64_t run_max, int64_t m8_max,
                                                                        int64_t m4_max) {
    extern __shared__ __align__(16) float lds[];
    if (n_dev) n = min(n, (int64_t)max(*n_dev, 0));
    if (n < run_min || n > run_max) return;
    if (n <= m4_max)
        sdf_small_body<FRAC, Tile8<4>>(lv, net, x, n, table, Bf, out, out_stride, out_cols, lds, blockIdx.x, gridDim.x);
    else if (n <= m8_max)
        sdf_small_body<FRAC, Tile8<8>>(lv, net, x, n, table, Bf, out, out_stride, out_cols, lds, blockIdx.x, gridDim.x);
    else
        sdf_small_body<FRAC, Tile16>(lv, net, x, n, table, Bf, out, out_stride, out_cols, lds, blockIdx.x, gridDim.x);
}

// ---------------------------------------------------------------------------------------------------------
// Persistent TAIL of the sphere-tracing march (reference: model/ray_tracing.py:98-187).  The search needs
// 1 + sphere_tracing_iters rounds when no ray runs a line search and up to 1 + iters * (1 + line_step_iters) = 41 when
// one does in every iteration; the launch-per-round form must enqueue all 41 (SDF launch, update launch) pairs, and
// the 30 surplus pairs - empty launches, ~4.7 us of dispatch each - cost more than a live round.  Rays are independent,
// so the surplus rounds need no grid at all: after the guaranteed rounds this kernel gives every workgroup EIGHT rays
// (at most 16 pending points, in 16 slots of its own behind the compact list; cursor in LDS) and lets it carry them
// through all remaining rounds - evaluate the pending points on the 16-point body, run trace_advance_ray for its own
// rays, repeat until they are done.  Nothing is exchanged between workgroups, nothing synchronises the grid; a
// workgroup without stragglers (the usual case: every one) leaves at once.  The guaranteed rounds stay launches of
// their own: there the compact list balances the live points over all CUs (a march of the whole search inside this
// kernel was measured: -0.21 ms per step with every ray live to the end, +0.20 ms with a third of them live - the
// slowest workgroup sets the time).
// (the per-ray functions are out of line: inlined, their registers are live across the tile body)
__device__ __attribute__((noinline)) void march_adopt_ray(const TraceArgs &a, int64_t i, int32_t *cursor, int32_t slot_base) {
    // a ray that is not done has pending points in the compact list of round `first`: move them to this workgroup's slots
    const TraceWs &w = a.w;
    if (w.stage[i] == ST_DONE) return;
    const int32_t ss = w.slot_s[i], se = w.slot_e[i];
    w.slot_s[i] = ss >= 0 ? append_point(a, cursor, slot_base, i, w.t_s[i]) : -1;
    w.slot_e[i] = se >= 0 ? append_point(a, cursor, slot_base, i, w.t_e[i]) : -1;
}
__device__ __attribute__((noinline)) void march_advance_ray(const TraceArgs &a, int64_t ray, int32_t *cursor, int32_t slot_base) {
    trace_advance_ray(a, ray, cursor, slot_base);
}

template <int FRAC>
__global__ __launch_bounds__(kThreadsSdf, 1) void trace_march_tail_kernel(HmLevels lv, SdfNet net,
                                                                           const float *__restrict__ table,
                                                                           const float *__restrict__ Bf, TraceArgs a,
                                                                           int first, int rounds, int lds_floats, int body16) {
    extern __shared__ __align__(16) float lds[];
    if (a.w.cnt[C_ROUND0 + first] == 0) return;     // no ray has a pending point: every state machine has finished
    int32_t *ctl = reinterpret_cast<int32_t *>(lds + lds_floats);   // [0] cursor of the round being filled
    const int tid = threadIdx.x;
    const int32_t slot_base = (int32_t)a.w.cap + (int32_t)blockIdx.x * 16;   // (second region of pts / vals)
    const int64_t ray = (int64_t)blockIdx.x * 8 + tid;
    const bool mine = tid < 8 && ray < a.n;
    const float *xp = a.w.pts + (int64_t)slot_base * 3;
    float *vp = a.w.vals + slot_base;
    if (tid == 0) ctl[0] = 0;
    __syncthreads();
    if (mine) march_adopt_ray(a, ray, ctl, slot_base);
    __syncthreads();
    for (int r = first; r < rounds; ++r) {
        const int n_loc = ctl[0];
        if (n_loc == 0) break;      // (uniform) every ray of this workgroup is done
        // the search's evaluation count (statistics; round `first` was counted when its points were appended)
        if (tid == 0 && r > first) atomicAdd(a.w.cnt + C_ROUND0 + r, n_loc);
        // the small-tile body that fits the workgroup's OWN pending points: a straggler's rounds cost 83 instead of 130 us
        // (600 training steps, r3aq: 7.00 ms per step with every tail round on the 16-point body against 6.43 ms with the
        // launch-per-round form, whose compact list runs such rounds on 4-point tiles).  body16 (tile_points = 16): the
        // 16-point body always - bit-identical to hm_sdf_fwd with 16-point tiles, how the tests compare this kernel
        // with the generic tracer.  (With the three bodies inlined the kernel spills ~60 VGPRs, none inside an MFMA loop.)
        if (n_loc <= 4 && !body16)
            sdf_small_body<FRAC, Tile8<4>>(lv, net, xp, n_loc, table, Bf, vp, 1, 1, lds, 0, 1 << 30);
        else if (n_loc <= 8 && !body16)
            sdf_small_body<FRAC, Tile8<8>>(lv, net, xp, n_loc, table, Bf, vp, 1, 1, lds, 0, 1 << 30);
        else
            sdf_small_body<FRAC, Tile16>(lv, net, xp, n_loc, table, Bf, vp, 1, 1, lds, 0, 1 << 30);
        __syncthreads();            // the values (global stores of this workgroup) are visible to its threads
        if (tid == 0) ctl[0] = 0;
        __syncthreads();
        if (mine) march_advance_ray(a, ray, ctl, slot_base);
        __syncthreads();
    }
}

// diagnostic (hm_diag_mfma_f32_stream): the MFMA stream of the 64-point kernel's k-loop without its memory traffic
__global__ __launch_bounds__(kThreadsSdf, 2) void mfma_f32_stream_kernel(int iters, float *out) {
    f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};
    float a0 = (float)(threadIdx.x & 63) * 1e-3f, a1 = a0 + 0.5f, b0 = 1.0f - a0, b1 = 0.25f + a0;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
        }
    }
    out[(size_t)blockIdx.x * kThreadsSdf + threadIdx.x] = acc00[0] + acc01[5] + acc10[9] + acc11[15];
}

// ---------------------------------------------------------------------------------------------------------
// Persistent secant refinement (reference: model/ray_tracing.py:251-268): the secant rays are a compact list, a tile
// of them (4 / 8 / 16 by the list's length - the rule of sdf_fwd_small_kernel, so the values are those of one
// hm_sdf_fwd launch per iteration) stays with its workgroup through all iterations: evaluate the tile's midpoints, run
// secant_advance_ray for its rays, repeat.  Nothing is exchanged between workgroups: 8 (SDF launch, update launch) pairs
// become one launch.
__device__ __attribute__((noinline)) void secant_step_ray(const TraceArgs &a, int64_t q, int last) {
    secant_advance_ray(a, q, last);
}

// The chain's state (pts, vals, the bracket arrays) lives in global memory between iterations, so a launch may run any
// RANGE of them: iterations [it_first, it_first + it_count) of a chain of it_total (the last one of the whole chain
// writes the results).
template <int FRAC>
__device__ __forceinline__ void secant_role(const HmLevels &lv, const SdfNet &net, const float *__restrict__ table,
                                            const float *__restrict__ Bf, const TraceArgs &a, int it_first, int it_count,
                                            int it_total, int64_t n, int pts, float *lds) {
    const int64_t n_tiles = (n + pts - 1) / pts;
    for (int it = it_first; it < it_first + it_count; ++it) {
        if (pts == 4)
            sdf_small_body<FRAC, Tile8<4>>(lv, net, a.w.pts, n, table, Bf, a.w.vals, 1, 1, lds, blockIdx.x, gridDim.x);
        else if (pts == 8)
            sdf_small_body<FRAC, Tile8<8>>(lv, net, a.w.pts, n, table, Bf, a.w.vals, 1, 1, lds, blockIdx.x, gridDim.x);
        else
            sdf_small_body<FRAC, Tile16>(lv, net, a.w.pts, n, table, Bf, a.w.vals, 1, 1, lds, blockIdx.x, gridDim.x);
        __syncthreads();       // the tile's values (global stores of this workgroup) are visible to its threads
        for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
            const int64_t q = tile * pts + threadIdx.x;
            if ((int)threadIdx.x < pts && q < n) secant_step_ray(a, q, it == it_total - 1 ? 1 : 0);
        }
        __syncthreads();       // the next iteration's points are written
    }
}

template <int FRAC>
__global__ __launch_bounds__(kThreadsSdf, 1) void trace_secant_kernel(HmLevels lv, SdfNet net,
                                                                       const float *__restrict__ table,
                                                                       const float *__restrict__ Bf, TraceArgs a,
                                                                       int n_iters, int64_t m8_max, int64_t m4_max,
                                                                       int64_t scan_hide) {
    extern __shared__ __align__(16) float lds[];
    const int64_t n = a.w.cnt[C_NSEC];
    if (n <= 0) return;
    // scan_hide > 0: the tile rule of sdf_scan_secant_kernel, so that both forms of the search give the same values
    const bool as_scan = scan_hide > 0 && a.w.cnt[C_NSEL_PTS] >= scan_hide;
    const int pts = as_scan ? 16 : (n <= m4_max ? 4 : (n <= m8_max ? 8 : 16));
    secant_role<FRAC>(lv, net, table, Bf, a, 0, n_iters, n_iters, n, pts, lds);
}

// ---------------------------------------------------------------------------------------------------------
// Closest-approach scan + secant refinement in ONE launch (training, tile size left to the library).  The secant
// iterations are a chain of eight dependent small-tile evaluations that keeps a few dozen workgroups busy for most of a
// millisecond while the rest of the chip idles; the closest-approach scan of the mask-loss rays (ray_tracing.py:71-92,
// ~77 k points at the bench workload) depends on neither the sampler nor the secant.  Here the workgroups that own secant
// tiles run that chain first (trace_secant_kernel's code), every other workgroup starts on the scan's 64-point tiles at
// once, and the tiles are handed out by an atomic cursor, so the late workgroups simply take fewer.  Values: the scan's
// are those of sdf_fwd_kernel (same tiles); the secant uses 16-point tiles when the scan is long enough to hide their
// latency (a 16-point tile does four times the rays of a 4-point one for 1.6x the time: least chip time), and the list
// length rule of trace_secant_kernel otherwise.
// The guarded mode runs the same kernel with another scan: scan_x -> scan_out, cnt[c_scan] points = the refinement list of
// the closest-approach rows' marked samples (any length on the 64-point body: scan_min 1), whose ~60 tiles fit beside the
// secant tiles; the secant's tile rule still reads the closest-approach scan's length.
// The launch runs iterations [it_first, it_first + n_iters) of a chain of it_total (secant_role).  QUARTER: the list runs
// on the tile schedule of sdf_fwd_kernel<FRAC, true> (quarter tiles up to 16 points per workgroup, else its half / full
// tiles) - the LAST rounds of a chain that was cut in two launches, with the list's one round under them; the workgroups
// that own secant tiles join the list afterwards if a tile is left.  No secant ray: the launch is the list's alone.
template <int FRAC, bool QUARTER>
__global__ __launch_bounds__(kThreadsSdf, 2) void sdf_scan_secant_kernel(HmLevels lv, SdfNet net,
                                                                          const float *__restrict__ table,
                                                                          const float *__restrict__ Bf, TraceArgs a,
                                                                          int it_first, int n_iters, int it_total,
                                                                          int64_t m8_max, int64_t m4_max,
                                                                          const float *__restrict__ scan_x,
                                                                          float *__restrict__ scan_out, int c_scan,
                                                                          int64_t scan_cap, int64_t scan_min,
                                                                          int64_t scan_hide, int c_prev1, int grid1,
                                                                          int c_prev2, int grid2) {
    extern __shared__ __align__(16) float lds[];
    const int64_t n_scan = min((int64_t)max(a.w.cnt[c_scan], 0), scan_cap);
    const int64_t n_sec = a.w.cnt[C_NSEC];
    if (n_sec > 0 && n_iters > 0) {
        // (the secant's tiles follow the closest-approach scan's length also where the scan of this launch is another list)
        const int pts = a.w.cnt[C_NSEL_PTS] >= scan_hide ? 16 : (n_sec <= m4_max ? 4 : (n_sec <= m8_max ? 8 : 16));
        secant_role<FRAC>(lv, net, table, Bf, a, it_first, n_iters, it_total, n_sec, pts, lds);
    }
    if (n_scan < scan_min) return;      // (a short scan is the small-tile launch's job; an empty list is nobody's)
    // the scan's first tiles completed the last rounds of the sampler's launches (filler tiles, see fill_quota)
    const int64_t tb = (n_scan + kPts - 1) / kPts;
    int64_t done = c_prev1 >= 0 ? fill_quota(max(a.w.cnt[c_prev1], 0), grid1, tb, scan_min) : 0;
    if (c_prev2 >= 0) done += fill_quota(max(a.w.cnt[c_prev2], 0), grid2, tb - done, scan_min);
    const int64_t skip = done * kPts;
    if (skip >= n_scan) return;
    const SdfFill none = {nullptr, nullptr, 0, 0};
    sdf64_run<FRAC, true, QUARTER>(lv, net, scan_x + skip * 3, n_scan - skip, table, Bf, scan_out + skip, 1, 1, lds,
                                   reinterpret_cast<unsigned *>(a.w.cnt + C_TILE_CURSOR), none);
}

// ---------------------------------------------------------------------------------------------------------
// Guarded coarse scans (hm_trace.hip): the exact refinement of a list of the sampler's marked samples and split tiles of the
// approximate closest-approach scan in ONE launch.  The refinement list is ~190 fp32 half tiles, one round on part of the
// chip; the closest-approach scan (1200 split tiles at the bench workload) depends on neither the sampler's values nor
// their refinement.  Every workgroup first takes fp32 64-point tiles of the list (sdf64_run with the atomic cursor: the
// tiles and values of the stand-alone refinement launch), then split tiles of this launch's range of the scan
// (hm_scan_pool.h: one per workgroup that got no fp32 tile, plus what would not fit under the secant chain) from a second
// cursor (the tile of sdf_fwd_split_kernel: a tile's values do not depend on the workgroup or the launch that runs it).
// The workgroups that got no fp32 tile start on the scan at once; nothing is exchanged between workgroups.  Both cursors
// are zero at launch.  which = 0 / 1: the launch of the list cnt[c_ref1] / of cnt[c_ref2] (lazy sampler, second pass).
template <int KIND, int FRAC>
__device__ __forceinline__ void split_scan_range(const HmLevels &lv, const SdfNet &net_split, const float *__restrict__ table,
                                                 const float *__restrict__ Bf, const TraceArgs &a, int64_t scan_off,
                                                 int64_t n_scan, int64_t first, int64_t quota, unsigned *cursor, float *lds) {
    __shared__ unsigned s_scan_tile;
    if (quota <= 0) return;
    for (;;) {
        __syncthreads();   // every thread has read the previous hand-out (and is done with the other tiles' LDS)
        if (threadIdx.x == 0) s_scan_tile = atomicAdd(cursor, 1u);
        __syncthreads();
        const int64_t k = s_scan_tile;
        if (k >= quota) break;
        sdf_split_tile<KIND, FRAC>(lv, net_split, a.w.pts + scan_off * 3, n_scan, table, Bf, a.w.vals + scan_off, 1, lds,
                                   first + k);
    }
}

template <int KIND, int FRAC>
__global__ __launch_bounds__(kThreadsSdf, 2) void sdf_refine_scan_kernel(HmLevels lv, SdfNet net, SdfNet net_split,
                                                                          const float *__restrict__ table,
                                                                          const float *__restrict__ Bf, TraceArgs a,
                                                                          int c_ref1, int c_ref2, int which,
                                                                          int64_t scan_off, int64_t chain_tiles) {
    extern __shared__ __align__(16) float lds[];
    const int64_t n_ref1 = min((int64_t)max(a.w.cnt[c_ref1], 0), a.w.cap);
    const int64_t n_ref2 = which ? min((int64_t)max(a.w.cnt[c_ref2], 0), a.w.cap) : 0;   // (not final in the first launch)
    const int64_t n_ref = which ? n_ref2 : n_ref1;
    const int64_t n_scan = min((int64_t)max(a.w.cnt[C_NSEL_PTS], 0), a.w.cap);
    if (n_ref > 0) {
        const SdfFill none = {nullptr, nullptr, 0, 0};
        sdf64_run<FRAC, true>(lv, net, a.w.ref_pts, n_ref, table, Bf, a.w.ref_vals, 1, 1, lds,
                              reinterpret_cast<unsigned *>(a.w.cnt + (which ? C_XREF2_CURSOR : C_XREF_CURSOR)), none);
    }
    const ScanPool p = scan_pool_quota(n_scan, n_ref1, n_ref2, c_ref2 >= 0, gridDim.x, a.w.cnt[C_NSAMP], chain_tiles);
    // (constant indices: a run-time index would put the struct into scratch)
    split_scan_range<KIND, FRAC>(lv, net_split, table, Bf, a, scan_off, n_scan, which ? p.first[1] : p.first[0],
                                 which ? p.quota[1] : p.quota[0],
                                 reinterpret_cast<unsigned *>(a.w.cnt + (which ? C_XSCAN2_CURSOR : C_XSCAN_CURSOR)), lds);
}

// ---------------------------------------------------------------------------------------------------------
// Guarded coarse scans: the secant chain and the REST of the closest-approach scan's split tiles in ONE launch.  The chain
// is eight dependent rounds of ~60 16-point tiles, a pure latency chain of about a millisecond; the scan's tiles that the
// refine-scan launches in front left over (hm_scan_pool.h: as many as fit under the chain) run on every other workgroup
// meanwhile, and the secant's workgroups join when their chain is done.  secant_role is sdf_scan_secant_kernel's (the tile
// rule reads the scan's length, so the secant's values are those of every other form of the search); the tiles are
// sdf_refine_scan_kernel's.  No workgroup waits for another.  grid_x: workgroups of the refine-scan launches.
// The launch runs iterations [it_first, it_first + n_iters) of a chain of it_total (secant_role): where the chain is cut,
// its first rounds, with ALL remaining tiles of the scan - the closest-approach rows are selected behind this launch.
template <int KIND, int FRAC>
__global__ __launch_bounds__(kThreadsSdf, 2) void sdf_split_scan_secant_kernel(HmLevels lv, SdfNet net, SdfNet net_split,
                                                                                const float *__restrict__ table,
                                                                                const float *__restrict__ Bf, TraceArgs a,
                                                                                int it_first, int n_iters, int it_total,
                                                                                int64_t m8_max, int64_t m4_max,
                                                                                int64_t scan_hide, int c_ref1, int c_ref2,
                                                                                int grid_x, int64_t scan_off,
                                                                                int64_t chain_tiles) {
    extern __shared__ __align__(16) float lds[];
    const int64_t n_sec = a.w.cnt[C_NSEC];
    if (n_sec > 0 && n_iters > 0) {
        const int pts = a.w.cnt[C_NSEL_PTS] >= scan_hide ? 16 : (n_sec <= m4_max ? 4 : (n_sec <= m8_max ? 8 : 16));
        secant_role<FRAC>(lv, net, table, Bf, a, it_first, n_iters, it_total, n_sec, pts, lds);
    }
    const int64_t n_scan = min((int64_t)max(a.w.cnt[C_NSEL_PTS], 0), a.w.cap);
    const int64_t n_ref1 = min((int64_t)max(a.w.cnt[c_ref1], 0), a.w.cap);
    const int64_t n_ref2 = c_ref2 >= 0 ? min((int64_t)max(a.w.cnt[c_ref2], 0), a.w.cap) : 0;
    const ScanPool p = scan_pool_quota(n_scan, n_ref1, n_ref2, c_ref2 >= 0, grid_x, a.w.cnt[C_NSAMP], chain_tiles);
    split_scan_range<KIND, FRAC>(lv, net_split, table, Bf, a, scan_off, n_scan, p.first[2], p.quota[2],
                                 reinterpret_cast<unsigned *>(a.w.cnt + C_YSCAN_CURSOR), lds);
}

// network descriptor -> kernel argument for the exact-fp32 kernels (sdf_net_from_desc)
static int sdf_net_fp32(const char *who, const HmLevels &lv, const hm_mlp_desc *mlp, int64_t emb_stride, SdfImage img,
                        SdfNet &net, bool *all_m16 = nullptr) {
    return sdf_net_from_desc(who, mlp, lv.E, emb_stride, img, 1, (lv.E + 7) / 8 * 2, false, net, all_m16);
}

// LDS limits of the small-tile (16 / 8 / 4-point) and 64-point launches; the tracer's persistent kernels keep 64 bytes of
// their own on top of the tile
constexpr size_t kLds16Max = 96 * 1024, kLds64Max = 160 * 1024, kLdsTrace = 64;

// The checks of every fp32 launch that can evaluate the network - hm_sdf_fwd / hm_sdf_fwd_emb at any tile size and the
// tracer's march, secant and scan-secant kernels - at their tightest bounds (hm_sdf_net_fits, HM_SDF_FP32).
static int sdf_fp32_fits(const hm_mlp_desc *mlp, int E) {
    HmLevels lv = {};
    lv.E = E;
    SdfNet net;
    bool have16 = true;
    const int rc = sdf_net_fp32("hm_sdf_net_fits", lv, mlp, 0, kImgM16Optional, net, &have16);
    if (rc != HM_OK) return rc;
    HM_CHECK_ARG(sdf_lds64(net).bytes() + kLdsTrace <= kLds64Max, "hm_sdf_net_fits: network does not fit the 160 KB LDS tile");
    HM_CHECK_ARG(!have16 || sdf_lds_small(net, E, kPts16).bytes() + kLdsTrace <= kLds16Max,
                 "hm_sdf_net_fits: network does not fit the 16-point LDS tile");
    return HM_OK;
}

// tile-size thresholds of the small-tile kernels: 8-point tiles up to m8_max live points, 4-point tiles up to m4_max,
// 16-point tiles above.  tile_points 0 / -1: by the live count (kSdfTiny, kSdfMini); 4, 8, 16: that size only.
struct SmallTiles {
    int64_t m8_max, m4_max;
};
static SmallTiles sdf_small_tiles(int tile_points) {
    const int64_t kBig = (int64_t)1 << 62;
    if (tile_points == 16) return {0, 0};
    if (tile_points == 8) return {kBig, 0};
    if (tile_points == 4) return {kBig, kBig};
    return {kSdfTiny, kSdfMini};
}
// workgroups of a small-tile launch over up to n live points: one tile each, at most `cap`
static unsigned sdf_small_grid(int64_t n, SmallTiles t, int64_t cap) {
    int64_t tiles = t.m8_max >= n ? 0 : (n + kPts16 - 1) / kPts16;
    if (t.m8_max > 0) tiles = max(tiles, ((n < t.m8_max ? n : t.m8_max) + kPts8 - 1) / kPts8);
    if (t.m4_max > 0) tiles = max(tiles, ((n < t.m4_max ? n : t.m4_max) + 3) / 4);
    return (unsigned)(tiles < cap ? tiles : cap);
}

// workgroups of a refine-scan launch (and of the stand-alone refinement launch it stands for) over a refinement region of
// `cap` points: up to one 32-point half tile of the list per workgroup
static unsigned refine_scan_grid(int64_t cap) {
    const int64_t tiles = (cap + 31) / 32;
    return (unsigned)(tiles < 256 ? tiles : 256);
}

// hm_frac_dispatch + the precomputed-embedding form of the kernels (mode kFracEmb)
template <class F>
int sdf_dispatch(int mode, F &&f) {
    if (mode == kFracEmb) return f(std::integral_constant<int, kFracEmb>{});
    return hm_frac_dispatch(mode, f);
}

// The host half that the ray search's fused launches share (hm_trace_host.h).  TILES = the tile bodies the entry's kernel
// runs: they decide which networks are built, which LDS tiles must fit and the launch's dynamic LDS - the largest of them
// plus `own` bytes that the kernel keeps behind the tile.  An entry opens it (argument checks, networks), makes its own
// range checks and returns if the call is empty, then launches: every kernel's arguments start with
// (lv, net[, net_split], table, B_fourier, TraceArgs).
enum : unsigned { kTile16 = 1, kTile64 = 2, kTileSplit = 4 };
template <unsigned TILES>
struct TraceLaunch {
    const char *who; const HmTraceCtx *cx; const TraceArgs *a;
    SdfNet net, net_split;
    size_t lds16 = 0, lds64 = 0, lds_split = 0, own = 0;

    int fail(const char *what) const { return hm_fail(HM_ERR_INVALID, std::string(who) + ": " + what); }

    int open(const char *who_, const HmTraceCtx *cx_, const void *trace_args, size_t own_ = 0) {
        who = who_; cx = cx_; own = own_;
        a = static_cast<const TraceArgs *>(trace_args);
        if (!(cx && cx->desc && cx->mlp && cx->table && cx->B_fourier && a)) return fail("NULL argument");
        if (cx->frac_mode != HM_FRAC_REFERENCE && cx->frac_mode != HM_FRAC_TRILINEAR) return fail("bad frac_mode");
        int rc = sdf_net_fp32(who, cx->desc->lv, cx->mlp, 0, kImgM16, net);
        if (rc == HM_OK && (TILES & kTileSplit)) rc = sdf_split_net(who, cx->desc->lv.E, cx->mlp, 0, net_split, &lds_split);
        if (rc != HM_OK) return rc;
        if (TILES & kTile16) lds16 = sdf_lds_small(net, cx->desc->lv.E, kPts16).bytes();
        if (TILES & kTile64) lds64 = sdf_lds64(net).bytes();
        return HM_OK;
    }

    template <auto Kernel, class... A>
    int launch(unsigned grid, A... args) const {
        constexpr bool only16 = TILES == kTile16;
        if (lds16 + own > kLds16Max || lds64 > kLds64Max - kLdsTrace || lds_split > kLds64Max - kLdsTrace)
            return fail(only16 ? "network does not fit the 16-point LDS tile" : "network does not fit the LDS tiles");
        const size_t lds64s = lds64 > lds_split ? lds64 : lds_split, lds = (lds16 > lds64s ? lds16 : lds64s) + own;
        HM_TRY(hm_allow_dynamic_lds<Kernel>((int)(only16 ? kLds16Max : kLds64Max - kLdsTrace)));
        if constexpr ((TILES & kTileSplit) != 0)
            hipLaunchKernelGGL(Kernel, dim3(grid), dim3(kThreadsSdf), lds, as_stream(cx->stream), cx->desc->lv, net, net_split,
                               cx->table, cx->B_fourier, *a, args...);
        else
            hipLaunchKernelGGL(Kernel, dim3(grid), dim3(kThreadsSdf), lds, as_stream(cx->stream), cx->desc->lv, net, cx->table,
                               cx->B_fourier, *a, args...);
        HM_CHECK_LAUNCH(who);
        return HM_OK;
    }
};

}  // namespace

extern "C" {

int hm_diag_mfma_f32_stream(int workgroups, int iters, float *out, void *stream) {
    HM_CHECK_ARG(workgroups >= 1 && workgroups <= 65535 && iters >= 1 && out, "hm_diag_mfma_f32_stream: bad argument");
    hipLaunchKernelGGL(mfma_f32_stream_kernel, dim3((unsigned)workgroups), dim3(kThreadsSdf), 0, as_stream(stream), iters, out);
    HM_CHECK_LAUNCH("hm_diag_mfma_f32_stream");
    return HM_OK;
}

#ifdef HM_SDF_PHASE_PROBE
HM_API int hm_probe_read(unsigned long long *out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(hm_probe_ts), sizeof(unsigned long long) * (size_t)(n < 128 ? n : 128)) == hipSuccess ? 0 : -1;
}
#endif

static int sdf_fwd_impl(const HmLevels &lv, const hm_mlp_desc *mlp, const float *x, int64_t emb_stride, int64_t n,
                        const float *table, const float *B_fourier, float *out, int64_t out_stride, int out_cols,
                        int frac_mode, int tile_points, const int32_t *n_dev, int max_workgroups, void *stream,
                        const SdfFillArgs *fill = nullptr, int *grid64_out = nullptr);
// hm_sdf_bf16.hip / hm_sdf_split.hip: the network and LDS checks of their launches (hm_sdf_net_fits)
int sdf_bf16_fits(const hm_mlp_desc *mlp, int E, int32_t *regions);
int sdf_split_fits(const hm_mlp_desc *mlp, int E, int32_t *regions);

// hm_sdf_fwd for the ray search's sampler launches (hm_trace_host.h)
int hm_sdf_fwd_fill(const HmTraceCtx *cx, const float *x, int64_t n, float *out, const int32_t *n_dev, const float *x_fill,
                    float *out_fill, const int32_t *n_fill_dev, const int32_t *prev_dev, int prev_grid, int *grid64_out) {
    HM_CHECK_ARG(cx && cx->desc && cx->mlp, "hm_sdf_fwd_fill: NULL descriptor");
    HM_CHECK_ARG(n == 0 || (cx->table && cx->B_fourier && n_dev && x_fill && out_fill && n_fill_dev),
                 "hm_sdf_fwd_fill: NULL pointer");
    SdfFillArgs fa = {x_fill, out_fill, n_fill_dev, prev_grid > 0 ? prev_dev : nullptr, prev_grid, 0};
    if (grid64_out) *grid64_out = 0;
    return sdf_fwd_impl(cx->desc->lv, cx->mlp, x, 0, n, cx->table, cx->B_fourier, out, 1, 1, cx->frac_mode, 0, n_dev, 0,
                        cx->stream, &fa, grid64_out);
}

int hm_sdf_fwd(const hm_grid_desc *desc, const hm_mlp_desc *mlp, const float *x, int64_t n, const float *table,
               const float *B_fourier, float *out, int64_t out_stride, int out_cols, int frac_mode, int tile_points,
               const int32_t *n_dev, int max_workgroups, void *stream) {
    HM_CHECK_ARG(desc && mlp, "hm_sdf_fwd: NULL descriptor");
    HM_CHECK_ARG(n == 0 || (table && B_fourier), "hm_sdf_fwd: NULL pointer");
    return sdf_fwd_impl(desc->lv, mlp, x, 0, n, table, B_fourier, out, out_stride, out_cols, frac_mode, tile_points,
                        n_dev, max_workgroups, stream);
}

int hm_sdf_fwd_emb(const hm_mlp_desc *mlp, const float *emb, int64_t emb_stride, int emb_width, int64_t n, float *out,
                   int64_t out_stride, int out_cols, int tile_points, const int32_t *n_dev, int max_workgroups,
                   void *stream) {
    HM_CHECK_ARG(mlp, "hm_sdf_fwd_emb: NULL descriptor");
    HmLevels lv;
    const int rc = sdf_emb_levels("hm_sdf_fwd_emb", emb_width, emb_stride, lv);
    if (rc != HM_OK) return rc;
    return sdf_fwd_impl(lv, mlp, emb, emb_stride, n, nullptr, nullptr, out, out_stride, out_cols, HM_FRAC_REFERENCE,
                        tile_points, n_dev, max_workgroups, stream);
}

// ---- the ray search's fused launches (hm_trace_host.h, where each entry is described) ----------------------------------
int hm_trace_march_tail(const HmTraceCtx *cx, const void *trace_args, int first, int rounds) {
    TraceLaunch<kTile16> L;
    HM_TRY(L.open("hm_trace_march_tail", cx, trace_args, kLdsTrace));
    HM_CHECK_ARG(first >= 1 && first < 64 && rounds <= 64, "hm_trace_march_tail: bad round range");
    const TraceArgs &a = *L.a;
    if (a.n == 0 || first >= rounds) return HM_OK;
    HM_CHECK_ARG(a.w.cap >= ((a.n + 7) / 8) * 16, "hm_trace_march_tail: point buffer too small");
    return hm_frac_dispatch(cx->frac_mode, [&](auto frac) {
        return L.launch<trace_march_tail_kernel<decltype(frac)::value>>(
            (unsigned)((a.n + 7) / 8), first, rounds, (int)(L.lds16 / sizeof(float)), cx->tile_points == 16 ? 1 : 0);
    });
}

int hm_trace_secant_persistent(const HmTraceCtx *cx, const void *trace_args, int n_iters, int scan_rule) {
    TraceLaunch<kTile16> L;
    HM_TRY(L.open("hm_trace_secant_persistent", cx, trace_args));
    const int tp = cx->tile_points;
    HM_CHECK_ARG(tp == 0 || tp == 4 || tp == 8 || tp == 16, "hm_trace_secant_persistent: tile_points must be 0, 4, 8 or 16");
    if (L.a->n == 0 || n_iters <= 0) return HM_OK;
    const SmallTiles t = sdf_small_tiles(tp);
    // workgroups for the longest list the call can see (every ray a secant ray), one tile each up to one per CU
    const unsigned grid = sdf_small_grid(L.a->n, t, 256);
    return hm_frac_dispatch(cx->frac_mode, [&](auto frac) {
        return L.launch<trace_secant_kernel<decltype(frac)::value>>(
            grid, n_iters, t.m8_max, t.m4_max, (int64_t)((scan_rule && tp == 0) ? kTraceScanHide : 0));
    });
}

int hm_trace_scan_secant(const HmTraceCtx *cx, const void *trace_args, int it_first, int n_iters, int it_total, int quarter,
                         const float *scan_x, float *scan_out, int64_t scan_capacity, int c_scan, int small_front,
                         int c_prev1, int grid1, int c_prev2, int grid2) {
    TraceLaunch<kTile16 | kTile64> L;
    HM_TRY(L.open("hm_trace_scan_secant", cx, trace_args));
    HM_CHECK_ARG(it_first >= 0 && n_iters >= 0 && it_first + n_iters <= it_total, "hm_trace_scan_secant: bad iteration range");
    HM_CHECK_ARG(!quarter || !small_front, "hm_trace_scan_secant: quarter tiles are a refinement list's");
    HM_CHECK_ARG(c_scan >= 0 && c_scan < C_COUNT && scan_capacity >= 0, "hm_trace_scan_secant: bad scan counter / capacity");
    HM_CHECK_ARG(small_front || (grid1 <= 0 && grid2 <= 0), "hm_trace_scan_secant: a refinement list has no filler tiles");
    const TraceArgs &a = *L.a;
    if (a.n == 0) return HM_OK;
    HM_CHECK_ARG(scan_x && scan_out, "hm_trace_scan_secant: NULL scan pointer");
    if (small_front) {
        // the scan's small-count form (tile_points -1: returns at once above kSdfSmall live points)
        HM_TRY(hm_sdf_fwd(cx->desc, cx->mlp, scan_x, scan_capacity, cx->table, cx->B_fourier, scan_out, 1, 1, cx->frac_mode, -1,
                          a.w.cnt + c_scan, 0, cx->stream));
    }
    // 16-point secant tiles once the scan keeps the chip busy for longer than their chain takes (8 x 131 us ~ 2.3 rounds
    // of 64-point tiles: 3 rounds = 49 152 points)
    static_assert(kTraceScanHide == 3 * 256 * kPts, "kTraceScanHide counts rounds of 64-point tiles");
    // c_prev*: counters holding the own-point counts of the sampler launches that took filler tiles of this scan (-1: none)
    const int p1 = grid1 > 0 ? c_prev1 : -1, p2 = grid2 > 0 ? c_prev2 : -1;
    const SmallTiles t = sdf_small_tiles(0);
    // (quarter: the grid of the stand-alone launch it stands for, sdf_fwd_impl - one quarter tile per workgroup at most)
    const int64_t qtiles = (scan_capacity + 15) / 16;
    const unsigned grid = quarter && qtiles < 256 ? (unsigned)(qtiles > 0 ? qtiles : 1) : 256u;
    return hm_frac_dispatch(cx->frac_mode, [&](auto frac) {
        return hm_bool_dispatch(quarter != 0, [&](auto q) {
            return L.launch<sdf_scan_secant_kernel<decltype(frac)::value, decltype(q)::value>>(
                grid, it_first, n_iters, it_total, t.m8_max, t.m4_max, scan_x, scan_out, c_scan, scan_capacity,
                (int64_t)(small_front ? kSdfSmall + 1 : 1), (int64_t)kTraceScanHide, p1, grid1, p2, grid2);
        });
    });
}

int hm_trace_refine_scan(const HmTraceCtx *cx, const void *trace_args, int c_ref1, int c_ref2, int which, int64_t scan_off,
                         int64_t scan_capacity, int64_t chain_tiles) {
    static_assert(sizeof(HmLevels) + 2 * sizeof(SdfNet) + sizeof(TraceArgs) + 64 <= 4096, "kernel arguments exceed 4 KB");
    TraceLaunch<kTile64 | kTileSplit> L;
    HM_TRY(L.open("hm_trace_refine_scan", cx, trace_args));
    HM_CHECK_ARG(c_ref1 >= 0 && c_ref1 < C_COUNT && c_ref2 < C_COUNT, "hm_trace_refine_scan: bad list counter");
    HM_CHECK_ARG((which == 0 || which == 1) && (which == 0 || c_ref2 >= 0) && chain_tiles >= 0,
                 "hm_trace_refine_scan: bad launch index / chain capacity");
    const TraceArgs &a = *L.a;
    if (a.n == 0) return HM_OK;
    HM_CHECK_ARG(a.w.pts && a.w.vals && a.w.ref_pts && a.w.ref_vals && a.w.cnt, "hm_trace_refine_scan: NULL workspace pointer");
    HM_CHECK_ARG(scan_off >= 0 && scan_capacity >= 0 && scan_capacity <= a.w.cap, "hm_trace_refine_scan: bad scan region");
    if (which == 0)
        HM_TRY(hm_sdf_fwd(cx->desc, cx->mlp, a.w.pts + scan_off * 3, scan_capacity, cx->table, cx->B_fourier,
                          a.w.vals + scan_off, 1, 1, cx->frac_mode, -1, a.w.cnt + C_NSEL_PTS, 0, cx->stream));
    return sdf_split_dispatch(cx->mlp, cx->frac_mode, [&](auto kind, auto frac) {
        return L.launch<sdf_refine_scan_kernel<decltype(kind)::value, decltype(frac)::value>>(
            refine_scan_grid(a.w.cap), c_ref1, c_ref2, which, scan_off, chain_tiles);
    });
}

int hm_trace_split_scan_secant(const HmTraceCtx *cx, const void *trace_args, int it_first, int n_iters, int it_total,
                               int c_ref1, int c_ref2, int64_t scan_off, int64_t scan_capacity, int64_t chain_tiles) {
    TraceLaunch<kTile16 | kTileSplit> L;
    HM_TRY(L.open("hm_trace_split_scan_secant", cx, trace_args));
    HM_CHECK_ARG(it_first >= 0 && n_iters >= 0 && it_first + n_iters <= it_total,
                 "hm_trace_split_scan_secant: bad iteration range");
    HM_CHECK_ARG(c_ref1 >= 0 && c_ref1 < C_COUNT && c_ref2 < C_COUNT && chain_tiles >= 0,
                 "hm_trace_split_scan_secant: bad list counter / chain capacity");
    const TraceArgs &a = *L.a;
    if (a.n == 0) return HM_OK;
    HM_CHECK_ARG(a.w.pts && a.w.vals && a.w.cnt, "hm_trace_split_scan_secant: NULL workspace pointer");
    HM_CHECK_ARG(scan_off >= 0 && scan_capacity >= 0 && scan_capacity <= a.w.cap, "hm_trace_split_scan_secant: bad scan region");
    const int grid_x = (int)refine_scan_grid(a.w.cap);     // workgroups of the refine-scan launches
    const SmallTiles t = sdf_small_tiles(0);
    return sdf_split_dispatch(cx->mlp, cx->frac_mode, [&](auto kind, auto frac) {
        return L.launch<sdf_split_scan_secant_kernel<decltype(kind)::value, decltype(frac)::value>>(
            256u, it_first, n_iters, it_total, t.m8_max, t.m4_max, (int64_t)kTraceScanHide, c_ref1, c_ref2, grid_x, scan_off,
            chain_tiles);
    });
}

int hm_trace_scan_pool_plan(int64_t n_scan, int64_t n_ref1, int64_t n_ref2, int two_x, int grid_x, int64_t n_sec_bound,
                            int n_iters, int64_t chain_tiles, int64_t *first, int64_t *quota) {
    HM_CHECK_ARG(n_scan >= 0 && n_ref1 >= 0 && n_ref2 >= 0 && grid_x >= 1 && grid_x <= 256 && n_sec_bound >= 0 &&
                     n_iters >= 0 && chain_tiles >= -1 && first && quota,
                 "hm_trace_scan_pool_plan: bad argument");
    const ScanPool p = scan_pool_quota(n_scan, n_ref1, n_ref2, two_x != 0, grid_x, n_sec_bound,
                                       trace_chain_tiles(n_iters, chain_tiles));
    for (int k = 0; k < 3; ++k) {
        first[k] = p.first[k];
        quota[k] = p.quota[k];
    }
    return HM_OK;
}

static int sdf_fwd_impl(const HmLevels &lv, const hm_mlp_desc *mlp, const float *x, int64_t emb_stride, int64_t n,
                        const float *table, const float *B_fourier, float *out, int64_t out_stride, int out_cols,
                        int frac_mode, int tile_points, const int32_t *n_dev, int max_workgroups, void *stream,
                        const SdfFillArgs *fill, int *grid64_out) {
    HM_CHECK_ARG(n >= 0, "hm_sdf_fwd: n < 0");
    HM_CHECK_ARG(frac_mode == HM_FRAC_REFERENCE || frac_mode == HM_FRAC_TRILINEAR, "hm_sdf_fwd: bad frac_mode");
    // the 64-point launch with quarter tiles enabled
    const bool quarter = tile_points == HM_SDF_TILE64_QUARTER;
    if (quarter) tile_points = 64;
    HM_CHECK_ARG(tile_points == 0 || tile_points == 4 || tile_points == 8 || tile_points == 16 || tile_points == 64 ||
                     tile_points == -1,
                 "hm_sdf_fwd: tile_points must be -1, 0, 4, 8, 16, 64 or HM_SDF_TILE64_QUARTER");
    SdfNet net;
    bool have16 = true;
    {
        const int rc = sdf_net_fp32("hm_sdf_fwd", lv, mlp, emb_stride, kImgM16Optional, net, &have16);
        if (rc != HM_OK) return rc;
    }
    const int mode = emb_stride > 0 ? kFracEmb : frac_mode;    // kernel template value
    const hm_mlp_layer &last = mlp->layer[mlp->n_layers - 1];
    HM_CHECK_ARG(out_cols == 1 || out_cols == last.out_dim, "hm_sdf_fwd: out_cols must be 1 or the last layer's out_dim");
    HM_CHECK_ARG(out_stride >= out_cols, "hm_sdf_fwd: out_stride < out_cols");
    HM_CHECK_ARG((tile_points != 16 && tile_points != 8 && tile_points != 4) || have16,
                 "hm_sdf_fwd: tile_points 4 / 8 / 16 need w_packed_m16 in every layer");
    if (n == 0) return HM_OK;
    HM_CHECK_ARG(x && out && (emb_stride > 0 || (table && B_fourier)), "hm_sdf_fwd: NULL pointer");
    // small batches: 16-point tiles spread the call over the whole chip (see sdf_small_body), 8- and 4-point
    // tiles below kSdfTiny / kSdfMini live points (one tile per CU), 64-point tiles above kSdfSmall.
    // With a device-side count the host cannot know the batch size: both kernels are enqueued and
    // each returns at once unless the live count falls in its range.
    const int64_t kBig = (int64_t)1 << 62;
    bool run16 = false, run64 = false;
    int64_t lo16 = 0, hi16 = kBig, lo64 = 0, hi64 = kBig;
    if (tile_points == -1) {   // small counts only: n > kSdfSmall is another launch's job (bf16 coarse kernel)
        HM_CHECK_ARG(have16, "hm_sdf_fwd: tile_points -1 needs w_packed_m16 in every layer");
        run16 = true; hi16 = kSdfSmall;
    }
    else if (tile_points == 4 || tile_points == 8 || tile_points == 16) run16 = true;
    else if (tile_points == 64 || !have16) run64 = true;
    else if (!n_dev) { run16 = n <= kSdfSmall; run64 = !run16; }
    else if (n <= kSdfSmall) run16 = true;
    else { run16 = run64 = true; hi16 = kSdfSmall; lo64 = kSdfSmall + 1; }
    const int64_t cap = max_workgroups > 0 ? max_workgroups : 256;  // one resident workgroup per CU
    if (run16) {
        const size_t lds = sdf_lds_small(net, lv.E, kPts16).bytes();
        HM_CHECK_ARG(lds <= kLds16Max, "hm_sdf_fwd: network does not fit the 16-point LDS tile");
        const SmallTiles t = sdf_small_tiles(tile_points);
        const unsigned grid = sdf_small_grid(n < hi16 ? n : hi16, t, cap);
        const int rc = sdf_dispatch(mode, [&](auto frac) {
            // (two activation images of 32 KB + the embedding = 70 KB at 512-wide layers)
            constexpr auto kernel = sdf_fwd_small_kernel<decltype(frac)::value>;
            const int rc = hm_allow_dynamic_lds<kernel>(96 * 1024);
            if (rc == HM_OK)
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreadsSdf), lds, as_stream(stream), lv, net, x, n, table,
                                   B_fourier, out, out_stride, out_cols, n_dev, lo16, hi16, t.m8_max, t.m4_max);
            return rc;
        });
        if (rc != HM_OK) return rc;
    }
    // big batches: one 64-point workgroup per CU
    if (run64) {
        const size_t lds = sdf_lds64(net).bytes();
        HM_CHECK_ARG(lds <= kLds64Max, "hm_sdf_fwd: network does not fit the 160 KB LDS tile");
        // (up to cap * 32 points: one 32-point half tile per workgroup - or one quarter tile of 16)
        const int64_t tiles = quarter ? (n + 15) / 16 : (n + 31) / 32;
        const int64_t grid = tiles < cap ? tiles : cap;
        // filler tiles only where every launch of the chain applies the same lower bound (fill_quota's run_min)
        const SdfFillArgs none = {nullptr, nullptr, nullptr, nullptr, 0, 0};
        const SdfFillArgs fa = (fill && lo64 == kSdfSmall + 1 && out_cols == 1 && out_stride == 1) ? *fill : none;
        if (grid64_out && fa.n_dev) *grid64_out = (int)grid;
        const auto launch = [&](auto frac, auto q) {
            constexpr auto kernel = sdf_fwd_kernel<decltype(frac)::value, decltype(q)::value>;
            const int rc = hm_allow_dynamic_lds<kernel>(160 * 1024);
            if (rc == HM_OK)
                hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kThreadsSdf), lds, as_stream(stream), lv, net, x, n,
                                   table, B_fourier, out, out_stride, out_cols, n_dev, lo64, hi64, fa);
            return rc;
        };
        const int rc = sdf_dispatch(mode, [&](auto frac) {
            return quarter ? launch(frac, std::true_type{}) : launch(frac, std::false_type{});
        });
        if (rc != HM_OK) return rc;
    }
    HM_CHECK_LAUNCH("hm_sdf_fwd");
    return HM_OK;
}

int hm_sdf_net_fits(const hm_mlp_desc *mlp, int emb_width, int family) {
    HM_CHECK_ARG(mlp && emb_width >= 1 && emb_width <= 512, "hm_sdf_net_fits: bad descriptor or embedding width");
    HM_CHECK_ARG(family == HM_SDF_FP32 || family == HM_SDF_BF16 || family == HM_SDF_SPLIT, "hm_sdf_net_fits: bad family");
    const int rc = family == HM_SDF_FP32   ? sdf_fp32_fits(mlp, emb_width)
                   : family == HM_SDF_BF16 ? sdf_bf16_fits(mlp, emb_width, nullptr)
                                           : sdf_split_fits(mlp, emb_width, nullptr);
    return rc == HM_OK ? 1 : 0;
}

int hm_diag_sdf_lds(const hm_mlp_desc *mlp, int emb_width, int family, int tile_points, int32_t *regions) {
    HM_CHECK_ARG(mlp && regions && emb_width >= 1 && emb_width <= 512, "hm_diag_sdf_lds: bad descriptor, embedding width or NULL");
    if (family == HM_SDF_BF16) return sdf_bf16_fits(mlp, emb_width, regions);
    if (family == HM_SDF_SPLIT) return sdf_split_fits(mlp, emb_width, regions);
    HM_CHECK_ARG(family == HM_SDF_FP32 && (tile_points == 64 || tile_points == 16 || tile_points == 8),
                 "hm_diag_sdf_lds: bad family or tile_points");
    HmLevels lv = {};
    lv.E = emb_width;
    SdfNet net;
    const int rc = sdf_net_fp32("hm_diag_sdf_lds", lv, mlp, 0, tile_points == 64 ? kImgM16Optional : kImgM16, net);
    if (rc != HM_OK) return rc;
    sdf_lds_report(tile_points == 64 ? sdf_lds64(net) : sdf_lds_small(net, emb_width, tile_points), regions);
    return HM_OK;
}

}  // extern "C"
