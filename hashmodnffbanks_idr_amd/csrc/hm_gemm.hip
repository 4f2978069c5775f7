// hm_gemm.hip - exact-fp32 MFMA GEMM for the grad-enabled path of the SDF / rendering MLPs
// (forward X*W^T+b, backward dY*W and dY^T*X, and the same three shapes again in the
// double-backward pass that ImplicitNetwork.gradient(create_graph=True) needs;
// reference: model/implicit_differentiable_renderer.py:102,116-128,211-221).
//
// C[M,N] (+)= op(A)[M,K] * op(B)[K,N] (+ bias[N]);  row-major with leading dimensions, any M/N/K
// (the MLP has K = 67, N = 445 and 257, M = number of points), guarded loads, optional split-K
// with fp32 atomics for the weight-gradient shape (small M x N, K = number of points).
//
// v_mfma_f32_32x32x2_f32 (exact fp32 fma chain); 4 waves per workgroup as 2 x 2, each owning
// TM x TN tiles of 32 x 32; both operands are staged through LDS in the k-grouped image
// [k/4][row][4] (rows XOR-swizzled by the k-group) so that both the 16-B staging stores and the
// MFMA operand fetches (ds_read_b128) are bank-conflict free; K is staged 128 deep for the 64x64
// tile so that one stage of MFMAs covers the L2 latency of the next stage's loads.
#include "hm_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));


struct GemmArgs {
    const float *A, *B, *bias;
    float *C;
    int32_t M, N, K;
    int32_t transA, transB;  // op(A) = A^T if transA (A stored [K,M]); op(B) = B^T if transB (B stored [N,K])
    int32_t vec_out;  // pipelined kernel: outputs and epilogue operands go as aligned 16-B accesses (gemm_store_quads);
                      // (sits in what was padding before the 64-bit fields: the other members keep their offsets)
    int64_t lda, ldb, ldc;
    int32_t k_chunk;  // K range handled by one blockIdx.z
    int32_t atomic;   // accumulate with atomics (split-K, or beta = 1)
    int32_t vecA, vecB;  // operand may be fetched with aligned 16-B loads
    int32_t nrecA, nrecB;  // pipelined kernel: bytes of the operands' buffer descriptors (reads beyond them return 0)
    hm_gemm_epilogue ep;  // fused elementwise epilogue (mode HM_EPI_NONE = plain store)
};

// LDS image of an operand tile: S[kg][row][4] (kg = k/4) with the row XOR-swizzled by kg so that both
// the 16-B staging stores (lanes = consecutive kg of one row) and the MFMA fragment loads (lanes =
// consecutive rows of one kg) are bank-conflict free.
template <int ROWS>
__device__ __forceinline__ int lds_slot(int kg, int row) {
    return (kg * ROWS + (row ^ (kg & 7))) * 4;
}

// Fetch one ROWS x BK operand tile into registers as float4 k-groups.
//   k-contiguous source (element (row,k) at P[row*ld + k]): lanes walk the k-groups of a row -> one
//   coalesced 16-B load per k-group (VEC) or four dword loads;
//   row-contiguous source (element (row,k) at P[k*ld + row]): lanes walk rows -> four coalesced dword
//   loads (k, k+1, k+2, k+3) per k-group.
// Every load is UNCONDITIONAL on a clamped in-range address and masked afterwards: a load under a
// per-element branch makes hipcc wait vmcnt(0) per element and serialises the stage's L2 round trips.
template <int ROWS, int BK, int NT, bool VEC>
__device__ __forceinline__ void load_tile(const float *__restrict__ P, int64_t ld, bool kcontig, int row0,
                                          int nrows, int k0, int kend, int tid, float4 (&r)[ROWS * BK / 4 / NT]) {
    constexpr int PER = ROWS * BK / 4 / NT;
    constexpr int KG = BK / 4;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int e = tid + NT * i;
        const int row = kcontig ? e / KG : e % ROWS;
        const int kg = kcontig ? e % KG : e / ROWS;
        const int gr = row0 + row, gk = k0 + kg * 4;
        const int rc = min(gr, nrows - 1);
        const bool rv = gr < nrows;
        float4 v;
        if (VEC) {  // k-contiguous, kend % 4 == 0, 16-B aligned rows
            const int kk = min(gk, kend - 4);
            v = *reinterpret_cast<const float4 *>(P + (int64_t)rc * ld + kk);
            const bool ok = rv && gk < kend;
            v.x = ok ? v.x : 0.0f; v.y = ok ? v.y : 0.0f; v.z = ok ? v.z : 0.0f; v.w = ok ? v.w : 0.0f;
        } else {
            const int64_t sr = kcontig ? ld : 1, sk = kcontig ? 1 : ld;
            const float *base = P + (int64_t)rc * sr;
            const int c0 = min(gk, kend - 1), c1 = min(gk + 1, kend - 1), c2 = min(gk + 2, kend - 1),
                      c3 = min(gk + 3, kend - 1);
            const float x0 = base[(int64_t)c0 * sk], x1 = base[(int64_t)c1 * sk], x2 = base[(int64_t)c2 * sk],
                        x3 = base[(int64_t)c3 * sk];
            v.x = (rv && gk < kend) ? x0 : 0.0f;
            v.y = (rv && gk + 1 < kend) ? x1 : 0.0f;
            v.z = (rv && gk + 2 < kend) ? x2 : 0.0f;
            v.w = (rv && gk + 3 < kend) ? x3 : 0.0f;
        }
        r[i] = v;
    }
}

template <int ROWS, int BK, int NT>
__device__ __forceinline__ void store_tile(float *__restrict__ S, bool kcontig, int tid,
                                           const float4 (&r)[ROWS * BK / 4 / NT]) {
    constexpr int PER = ROWS * BK / 4 / NT;
    constexpr int KG = BK / 4;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int e = tid + NT * i;
        int row, kg;
        if (kcontig) { row = e / KG; kg = e % KG; } else { kg = e / ROWS; row = e % ROWS; }
        *reinterpret_cast<float4 *>(S + lds_slot<ROWS>(kg, row)) = r[i];
    }
}

// Store one 32x32 accumulator tile: lane holds column n, registers hold rows mrow0 + (r&3) + 8(r>>2)
// (mrow0 already includes the lane half's +4).  EP selects the fused Softplus epilogues (include/hashmod.h).
// PART: deterministic split-K - the tile is k part kz's partial and goes with plain stores to the workspace slab
// g.C + kz * M * ldc (ldc = N); gemm_part_reduce_kernel sums the slabs in k-part order.
// The epilogue is written out here and again in gemm_store_oct and gemm_store_quads (through gemm_epi_elem) on purpose:
// built from gemm_store_oct, or from gemm_epi_elem alone, this function computes the same values, but hipcc then grows the
// epilogue instances of the generic and big-tile kernels by 11 - 15 % in instructions (for example 12618 -> 14368 lines).
template <bool EP, bool PART = false>
__device__ __forceinline__ void gemm_store_tile(const GemmArgs &g, const f32x16 &acc, int n, int mrow0, bool add_bias,
                                                int kz = 0) {
    const float bv = add_bias ? g.bias[n] : 0.0f;
    const int mode = EP ? g.ep.mode : (int)HM_EPI_NONE;
    // epilogue operands first, all 16 (+16) loads in flight together on clamped addresses: a load under
    // a per-row guard would be waited for one at a time
#pragma unroll
    for (int half = 0; half < 2; ++half) {
    float zv[8], gv[8];
    if (mode == HM_EPI_S1MUL || mode == HM_EPI_ADJOINT || mode == HM_EPI_RELUMASK) {
        const int nc = mode != HM_EPI_ADJOINT ? min(n, g.ep.nz - 1) : n;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 8 * half + q;
            const int mc = min(mrow0 + (r & 3) + 8 * (r >> 2), g.M - 1);
            zv[q] = g.ep.z[(int64_t)mc * g.ep.ldz + nc];
        }
        if (g.ep.g) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int r = 8 * half + q;
                const int mc = min(mrow0 + (r & 3) + 8 * (r >> 2), g.M - 1);
                gv[q] = g.ep.g[(int64_t)mc * g.ep.ldg + nc];
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) gv[q] = 0.0f;
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int r = 8 * half + q;
        const int m = mrow0 + (r & 3) + 8 * (r >> 2);
        if (m >= g.M) continue;
        float v = acc[r] + bv;
        if (mode != HM_EPI_NONE) v *= g.ep.scale;
        if (PART) {
            g.C[((int64_t)kz * g.M + m) * g.ldc + n] = v;
        } else if (g.C) {
            float *dst = g.C + (int64_t)m * g.ldc + n;
            if (g.atomic)
                atomicAdd(dst, v);
            else
                *dst = v;
        }
        if (mode == HM_EPI_SOFTPLUS) {
            g.ep.out1[(int64_t)m * g.ep.ld1 + n] = hm_softplus_fwd(v, g.ep.beta, g.ep.threshold);
        } else if (mode == HM_EPI_RELU) {
            g.ep.out1[(int64_t)m * g.ep.ld1 + n] = fmaxf(v, 0.0f);
        } else if (mode == HM_EPI_RELUMASK) {
            if (n < g.ep.nz) g.ep.out1[(int64_t)m * g.ep.ld1 + n] = (zv[q] > 0.0f ? v : 0.0f) + gv[q];
        } else if (mode == HM_EPI_S1MUL) {
            if (n < g.ep.nz)
                g.ep.out1[(int64_t)m * g.ep.ld1 + n] =
                    v * hm_sp_deriv(zv[q], g.ep.beta, g.ep.threshold).s1 + gv[q];
        } else if (mode == HM_EPI_ADJOINT) {
            const SpDeriv d = hm_sp_deriv(zv[q], g.ep.beta, g.ep.threshold);
            g.ep.out1[(int64_t)m * g.ep.ld1 + n] = v * d.s1;
            g.ep.out2[(int64_t)m * g.ep.ld2 + n] = v * gv[q] * d.s2;
            if (g.ep.out3) g.ep.out3[(int64_t)m * g.ep.ld3 + n] = gv[q] * d.s1;
        }
    }
    }
}

// The fused epilogue of ONE element (include/hashmod.h): v = (acc + bias) * scale is what goes to C; z / gv are the element's
// epilogue operands (unused by the modes that have none).  o1 / o2 / o3 go to ep.out1 / out2 / out3.
struct GemmEpiOut {
    float o1, o2, o3;
};
__device__ __forceinline__ GemmEpiOut gemm_epi_elem(const hm_gemm_epilogue &ep, int mode, float v, float z, float gv) {
    GemmEpiOut o;
    o.o1 = o.o2 = o.o3 = 0.0f;
    if (mode == HM_EPI_SOFTPLUS) {
        o.o1 = hm_softplus_fwd(v, ep.beta, ep.threshold);
    } else if (mode == HM_EPI_RELU) {
        o.o1 = fmaxf(v, 0.0f);
    } else if (mode == HM_EPI_RELUMASK) {
        o.o1 = (z > 0.0f ? v : 0.0f) + gv;
    } else if (mode == HM_EPI_S1MUL) {
        o.o1 = v * hm_sp_deriv(z, ep.beta, ep.threshold).s1 + gv;
    } else if (mode == HM_EPI_ADJOINT) {
        const SpDeriv d = hm_sp_deriv(z, ep.beta, ep.threshold);
        o.o1 = v * d.s1;
        o.o2 = v * gv * d.s2;
        o.o3 = gv * d.s1;
    }
    return o;
}

// The pipelined kernels' form of gemm_store_tile, for the HALF tile a wave finishes: eight rows of one column, lane holds
// column n, a[q] is row mrow0 + (q&3) + 8(q>>2).  EP and PART as above.
template <bool EP, bool PART = false>
__device__ __forceinline__ void gemm_store_oct(const GemmArgs &g, const float (&a)[8], int n, int mrow0, bool add_bias,
                                               int kz = 0) {
    const float bv = add_bias ? g.bias[n] : 0.0f;
    const int mode = EP ? g.ep.mode : (int)HM_EPI_NONE;
    // epilogue operands first, all 8 (+8) loads in flight together on clamped addresses: a load under
    // a per-row guard would be waited for one at a time
    float zv[8] = {}, gv[8] = {};
    if (mode == HM_EPI_S1MUL || mode == HM_EPI_ADJOINT || mode == HM_EPI_RELUMASK) {
        const int nc = mode != HM_EPI_ADJOINT ? min(n, g.ep.nz - 1) : n;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int mc = min(mrow0 + (q & 3) + 8 * (q >> 2), g.M - 1);
            zv[q] = g.ep.z[(int64_t)mc * g.ep.ldz + nc];
        }
        if (g.ep.g) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int mc = min(mrow0 + (q & 3) + 8 * (q >> 2), g.M - 1);
                gv[q] = g.ep.g[(int64_t)mc * g.ep.ldg + nc];
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) gv[q] = 0.0f;
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int m = mrow0 + (q & 3) + 8 * (q >> 2);
        if (m >= g.M) continue;
        float v = a[q] + bv;
        if (mode != HM_EPI_NONE) v *= g.ep.scale;
        if (PART) {
            g.C[((int64_t)kz * g.M + m) * g.ldc + n] = v;
        } else if (g.C) {
            float *dst = g.C + (int64_t)m * g.ldc + n;
            if (g.atomic)
                atomicAdd(dst, v);
            else
                *dst = v;
        }
        if (mode == HM_EPI_NONE) continue;
        const GemmEpiOut o = gemm_epi_elem(g.ep, mode, v, zv[q], gv[q]);
        const bool masked = mode == HM_EPI_S1MUL || mode == HM_EPI_RELUMASK;   // out1 has nz columns
        if (!masked || n < g.ep.nz) g.ep.out1[(int64_t)m * g.ep.ld1 + n] = o.o1;
        if (mode == HM_EPI_ADJOINT) {
            g.ep.out2[(int64_t)m * g.ep.ld2 + n] = o.o2;
            if (g.ep.out3) g.ep.out3[(int64_t)m * g.ep.ld3 + n] = o.o3;
        }
    }
}

// The 16-byte form of gemm_store_oct: the lane holds columns n .. n+3 (n % 4 == 0) of rows m and m + 8.  The host takes it
// (GemmArgs::vec_out) when N, every leading dimension and every base the epilogue touches are multiples of 16 bytes and
// nothing is accumulated, so a quad is whole - inside N and inside nz, or outside - and every access is one dwordx4.
template <bool EP, bool PART = false>
__device__ __forceinline__ void gemm_store_quads(const GemmArgs &g, const float4 (&a)[2], int n, int m0, bool add_bias,
                                                 int kz = 0) {
    const int mode = EP ? g.ep.mode : (int)HM_EPI_NONE;
    float bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (add_bias) {
#pragma unroll
        for (int c = 0; c < 4; ++c) bv[c] = g.bias[n + c];
    }
    // epilogue operands first, on clamped addresses (see gemm_store_oct)
    float4 zq[2] = {}, gq[2] = {};
    if (mode == HM_EPI_S1MUL || mode == HM_EPI_ADJOINT || mode == HM_EPI_RELUMASK) {
        const int nc = mode != HM_EPI_ADJOINT ? min(n, g.ep.nz - 4) : n;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int mc = min(m0 + 8 * i, g.M - 1);
            zq[i] = *reinterpret_cast<const float4 *>(g.ep.z + (int64_t)mc * g.ep.ldz + nc);
            gq[i] = g.ep.g ? *reinterpret_cast<const float4 *>(g.ep.g + (int64_t)mc * g.ep.ldg + nc)
                           : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + 8 * i;
        if (m >= g.M) continue;
        const float av[4] = {a[i].x, a[i].y, a[i].z, a[i].w};
        const float zv[4] = {zq[i].x, zq[i].y, zq[i].z, zq[i].w}, gv[4] = {gq[i].x, gq[i].y, gq[i].z, gq[i].w};
        float v[4], o1[4], o2[4], o3[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            v[c] = av[c] + bv[c];
            if (mode != HM_EPI_NONE) v[c] *= g.ep.scale;
            const GemmEpiOut o = gemm_epi_elem(g.ep, mode, v[c], zv[c], gv[c]);
            o1[c] = o.o1; o2[c] = o.o2; o3[c] = o.o3;
        }
        auto put = [](float *dst, const float (&x)[4]) {
            *reinterpret_cast<float4 *>(dst) = make_float4(x[0], x[1], x[2], x[3]);
        };
        if (PART)
            put(g.C + ((int64_t)kz * g.M + m) * g.ldc + n, v);
        else if (g.C)
            put(g.C + (int64_t)m * g.ldc + n, v);
        if (mode == HM_EPI_NONE) continue;
        const bool masked = mode == HM_EPI_S1MUL || mode == HM_EPI_RELUMASK;   // out1 has nz columns
        if (!masked || n < g.ep.nz) put(g.ep.out1 + (int64_t)m * g.ep.ld1 + n, o1);
        if (mode == HM_EPI_ADJOINT) {
            put(g.ep.out2 + (int64_t)m * g.ep.ld2 + n, o2);
            if (g.ep.out3) put(g.ep.out3 + (int64_t)m * g.ep.ld3 + n, o3);
        }
    }
}

// KS = intra-workgroup K split: 4*KS waves, wave group g multiplies octets [g*BK/8/KS, (g+1)*BK/8/KS) of every
// stage, partial tiles are summed through LDS at the end.  Two waves per SIMD keep the matrix pipe busy
// while the next stage's loads are in flight even when the grid has only one workgroup per CU.
// EP: compiled with the fused epilogues (kept out of the plain instantiation: its extra registers would drop the
// 64x64 configuration from two resident workgroups per CU to one).  The 8-wave configuration is held to 128 VGPRs
// (4 waves per SIMD = two workgroups per CU).
// WM: wave rows of the tile (2 -> 64*TM rows); the wave columns are always 2.
// PART: the deterministic split-K form (no epilogue): k part blockIdx.z's partial tile goes to its workspace slab
// (gemm_store_tile<false, true>).  As a parameter of this kernel it is free for the PART = false instances: their
// instruction streams and descriptors stay line for line what they were while the PART form was a copy of this kernel
// (scripts/kernel_isa_diff.py shows that without a GPU).  Sharing the body the other way - a __device__ __forceinline__
// template with both kernels as three-line wrappers - was not: it moved every instance, the plain big-tile NN one from
// 2862 to 3112 instructions, the big-tile epilogue ones from 11.9 - 12.7 k to 14.2 - 15.4 k.
template <int TM, int TN, int BK, int KS, bool VA, bool VB, bool EP, int WM = 2, bool PART = false>
__global__ __launch_bounds__(128 * WM * KS, (WM * KS == 4 ? 4 : 1)) void gemm_f32_kernel(GemmArgs g) {
    constexpr int BM = 32 * WM * TM, BN = 64 * TN, NT = 128 * WM * KS, WG = 2 * WM;  // WG = waves per k part
    __shared__ __align__(16) float smem[BK * (BM + BN)];
    float *As = smem, *Bs = smem + BK * BM;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int kpart = wave / WG, wsub = wave % WG;
    const int wm = wsub >> 1, wn = wsub & 1;
    const int j = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int kbeg = blockIdx.z * g.k_chunk;
    const int kend = min(g.K, kbeg + g.k_chunk);
    const bool a_kc = (g.transA == 0);  // A[m*lda + k]
    const bool b_kc = (g.transB != 0);  // B stored [N,K]: B[n*ldb + k]

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

    float4 ra[BM * BK / 4 / NT], rb[BN * BK / 4 / NT];
    if (kbeg < kend) {   // (K = 0: the clamped prologue addresses would lie before the operands, which may be NULL)
        load_tile<BM, BK, NT, VA>(g.A, g.lda, a_kc, m0, g.M, kbeg, kend, tid, ra);
        load_tile<BN, BK, NT, VB>(g.B, g.ldb, b_kc, n0, g.N, kbeg, kend, tid, rb);
    }
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
        __syncthreads();  // previous stage fully consumed
        store_tile<BM, BK, NT>(As, a_kc, tid, ra);
        store_tile<BN, BK, NT>(Bs, b_kc, tid, rb);
        __syncthreads();
        if (k0 + BK < kend) {  // prefetch the next stage into registers while this one is multiplied
            load_tile<BM, BK, NT, VA>(g.A, g.lda, a_kc, m0, g.M, k0 + BK, kend, tid, ra);
            load_tile<BN, BK, NT, VB>(g.B, g.ldb, b_kc, n0, g.N, k0 + BK, kend, tid, rb);
        }
        constexpr int OCT = BK / 8 / KS;
#pragma unroll
        for (int oo = 0; oo < OCT; ++oo) {
            float4 a[TM], b[TN];
            const int kg = 2 * (kpart * OCT + oo) + h;
#pragma unroll
            for (int t = 0; t < TM; ++t)
                a[t] = *reinterpret_cast<const float4 *>(As + lds_slot<BM>(kg, wm * 32 * TM + t * 32 + j));
#pragma unroll
            for (int t = 0; t < TN; ++t)
                b[t] = *reinterpret_cast<const float4 *>(Bs + lds_slot<BN>(kg, wn * 32 * TN + t * 32 + j));
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn) {
                        const float av = s == 0 ? a[tm].x : s == 1 ? a[tm].y : s == 2 ? a[tm].z : a[tm].w;
                        const float bv = s == 0 ? b[tn].x : s == 1 ? b[tn].y : s == 2 ? b[tn].z : b[tn].w;
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[tm][tn], 0, 0, 0);
                    }
        }
    }

    if (KS > 1) {
        // sum the wave groups' partial tiles through LDS (the staging buffers are free now)
        static_assert(KS == 1 || (TM == 1 && TN == 1), "intra-workgroup K split is built for the 64x64 tile");
        __syncthreads();
        float *red = smem;  // (KS-1) * WG waves * 16 regs * 64 lanes floats
        static_assert((KS - 1) * WG * 16 * 64 <= BK * (BM + BN), "K-split reduction does not fit the staging buffers");
        if (kpart > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) red[(((kpart - 1) * WG + wsub) * 16 + r) * 64 + lane] = acc[0][0][r];
        }
        __syncthreads();
        if (kpart > 0) return;
#pragma unroll
        for (int p = 0; p < KS - 1; ++p)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][0][r] += red[((p * WG + wsub) * 16 + r) * 64 + lane];
    }

    // epilogue: lane holds column n, registers hold rows (r&3) + 8(r>>2) + 4h
    const bool add_bias = (g.bias != nullptr) && (blockIdx.z == 0);
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int n = n0 + wn * 32 * TN + tn * 32 + j;
            if (n >= g.N) continue;
            const int mrow0 = m0 + wm * 32 * TM + tm * 32 + 4 * h;
            if constexpr (PART)
                gemm_store_tile<false, true>(g, acc[tm][tn], n, mrow0, add_bias, blockIdx.z);
            else
                gemm_store_tile<EP>(g, acc[tm][tn], n, mrow0, add_bias);
        }
}

// ---------------------------------------------------------------------------------------------------------
// Pipelined 64x64 tile for the training shapes (M = 2048...4096 rows, N = K = 512: 256-512 tiles, i.e. ONE or two
// workgroups per CU, 6.8 us of matrix work each).  With so little work per tile the steady state of the software
// pipeline has to be tight: 32-deep K stages (16 of them at K = 512), global loads issued kPipeD-1 stages ahead into
// a register ring, two LDS buffers, and the MFMA operands of a stage held in registers (two sets) so that the LDS
// round trip of stage s+1 - store, the ONE barrier of the stage, fragment reads - is issued in the middle of stage
// s's MFMAs.  (A wave that has passed the barrier of stage s has read the fragments of stage s-1's buffer long
// before, so that buffer is free to refill.)  The loop body has NO conditionals - the K range is a whole number of
// kPipeD-stage groups (a K tail is rounded up, see gemm_pipe2_body), partial edge tiles clamp their offsets once,
// before the loop - because with the
// generic kernel's guards in it hipcc keeps the accumulators in VGPRs across the back edge and copies all 32 of
// them to AGPRs and back every stage.
// AKC / BKC: operand is k-contiguous (one dwordx4 per k-group), else row-contiguous (four dwords).
constexpr int kPipeBK = 32, kPipeD = 4;

// Phase stamps of ONE tile (probe builds only, scripts/gemm_phase_probe.py): workgroup (0, 0, 0) / thread 0 writes the
// 100 MHz wall clock at [0] entry, [1] first operands in LDS, [2] end of the K loop, [3] after the wave groups' exchange,
// [4] after its last epilogue store has completed; [5] is the time it spent in the K loop's barriers.
#ifdef HM_GEMM_PHASE_PROBE
__device__ unsigned long long hm_gemm_probe_ts[8];
#define HM_GEMM_PROBE_ON (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0)
#define HM_GEMM_STAMP(i_)                                                                            \
    do {                                                                                             \
        if ((i_) == 4) __builtin_amdgcn_s_waitcnt(0);   /* vmcnt(0): the stores have left */          \
        if (HM_GEMM_PROBE_ON) hm_gemm_probe_ts[(i_)] = wall_clock64();                               \
    } while (0)
#define HM_GEMM_LOOP_BARRIER()                                                                       \
    do {                                                                                             \
        const unsigned long long t_ = wall_clock64();                                                \
        __syncthreads();                                                                             \
        probe_wait += wall_clock64() - t_;                                                           \
    } while (0)
#else
#define HM_GEMM_STAMP(i_) do { } while (0)
#define HM_GEMM_LOOP_BARRIER() __syncthreads()
#endif

// one stage's operand k-groups through a buffer descriptor: voff = the thread's byte offset (loop invariant), soff = the
// stage's byte offset (scalar)
template <bool KC, int PER>
__device__ __forceinline__ void pipe_fetch_buf(const __amdgpu_buffer_rsrc_t &rs, const int (&voff)[PER], int soff, int ld4,
                                               float4 (&x)[PER]) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        if (KC) {
            const auto u = __builtin_amdgcn_raw_buffer_load_b128(rs, voff[i], soff, 0);
            x[i] = make_float4(__uint_as_float(u[0]), __uint_as_float(u[1]), __uint_as_float(u[2]), __uint_as_float(u[3]));
        } else {
            x[i] = make_float4(__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff[i], soff, 0)),
                               __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff[i], soff + ld4, 0)),
                               __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff[i], soff + 2 * ld4, 0)),
                               __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff[i], soff + 3 * ld4, 0)));
        }
    }
}

// K tail: zero the elements k >= K of a k-contiguous operand's k-groups (klim = K - the group's first k within the chunk,
// k0 = the stage's first k).  Applied when the ring slot goes to LDS - its loads have landed by then - not at the fetch,
// where the select would wait for them.
template <bool KC, int PER>
__device__ __forceinline__ void pipe_mask_tail(float4 (&x)[PER], const int (&klim)[PER], int k0) {
    if (!KC) return;   // k is the slow dimension: the buffer descriptor returns zeros beyond K
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int l = klim[i] - k0;
        x[i].x = l > 0 ? x[i].x : 0.0f;
        x[i].y = l > 1 ? x[i].y : 0.0f;
        x[i].z = l > 2 ? x[i].z : 0.0f;
        x[i].w = l > 3 ? x[i].w : 0.0f;
    }
}

// Addends of the grouped TN form (gemm_f32_pipe2_group_add_kernel): rows k in [a_k0, a_k1) of A are used as
// A[k] + A2[k - a_k0], likewise B.  The kernel sees each addend as a buffer descriptor over EXACTLY its rows (nrec bytes
// from A2 / B2; 0 = no addend) and the row offset of k = 0 relative to it, so that every k-group outside the range -
// a negative offset is a huge unsigned one - reads zeros and the K loop needs no condition: the trick of the K tail.
struct GemmAddend {
    const float *A2, *B2;
    int32_t lda2, ldb2;      // leading dimensions (floats)
    int32_t a_k0, b_k0;      // first row of A / B the addend covers (multiples of 4: whole k-groups)
    int32_t a_k1, b_k1;      // end of the range (== k0: no addend)
    int32_t nrecA2, nrecB2;  // bytes of the descriptors: 4 * ((k1 - k0 - 1) * ld2 + rows of the tile's dimension)
};

// one stage's addend k-groups (k the slow dimension: four dwords).  The range check must see the STAGE's offset too, so
// it is added to the thread's offset on the VALU (one add per operand and stage) and only the k-group's own rows -
// 0 .. 3 * ld, which never leave a range of whole k-groups - go to the scalar offset.
template <int PER>
__device__ __forceinline__ void pipe_fetch_add(const __amdgpu_buffer_rsrc_t &rs, const int (&voff)[PER], int stage_off,
                                               int ld4, float4 (&x)[PER]) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int v = voff[i] + stage_off;
        x[i] = make_float4(__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, v, 0, 0)),
                           __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, v, ld4, 0)),
                           __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, v, 2 * ld4, 0)),
                           __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, v, 3 * ld4, 0)));
    }
}
// operand + addend, one fp32 add per element, where the ring slot goes to LDS (like pipe_mask_tail).  The empty asm
// statement pins the add to this place: without it hipcc adds each addend in the stage after its fetch - that frees the
// addend's registers early, and waits vmcnt(0) for loads issued one stage before instead of three.
template <int PER>
__device__ __forceinline__ void pipe_add(float4 (&x)[PER], float4 (&q)[PER]) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        asm volatile("" : "+v"(q[i].x), "+v"(q[i].y), "+v"(q[i].z), "+v"(q[i].w));
        x[i].x = __fadd_rn(x[i].x, q[i].x);
        x[i].y = __fadd_rn(x[i].y, q[i].y);
        x[i].z = __fadd_rn(x[i].z, q[i].z);
        x[i].w = __fadd_rn(x[i].w, q[i].w);
    }
}

template <int OCT, int AROWS>
__device__ __forceinline__ void pipe_read_ops(const float *as, const float *bs, int arow, int brow, int h,
                                              float4 (&xa)[OCT], float4 (&xb)[OCT]) {
#pragma unroll
    for (int oo = 0; oo < OCT; ++oo) {
        const int kg = 2 * oo + h;
        xa[oo] = *reinterpret_cast<const float4 *>(as + lds_slot<AROWS>(kg, arow));
        xb[oo] = *reinterpret_cast<const float4 *>(bs + lds_slot<64>(kg, brow));
    }
}
__device__ __forceinline__ void pipe_mfma_oct(const float4 &a, const float4 &b, f32x16 &c) {
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, c, 0, 0, 0);
}


// The pipeline runs on EIGHT waves: two wave groups split the octets of every stage (two waves per SIMD hide each
// other's barrier / LDS turnarounds), partial tiles are summed through LDS at the end.
// WM = 3: a 96 x 64 tile on TWELVE waves (two groups of 3 x 2), for row counts whose 64-row grid is between one and two
// rounds of the chip: M = 3072, N = 512 are 384 tiles of 64 x 64 - a CU with two of them takes twice as long as the one
// with one - but exactly 256 of 96 x 64.  The B panel is staged by the first 512 threads.
// KT: the K range has a tail (see the descriptors below); the k-contiguous operand's k >= K elements are zeroed before
// they go to LDS.  A separate instantiation, so that the K-whole loop keeps its instructions.
// ADD: the operands have addends over row ranges (*ad, see GemmAddend; both operands row-contiguous), fetched into a ring
// of their own beside the operands' and added when the slot goes to LDS.  Bit 0: A has one, bit 1: B has one - separate
// instantiations for the same reason, and so that a workgroup whose k part meets only one operand's range (the caller
// chooses, gemm_group_body) issues only that operand's extra loads.  These instances stage through the launch's DYNAMIC
// LDS (2 * BK * (BM + BN) floats), which the instances inlined into one kernel share; the others keep their static arrays.
template <bool AKC, bool BKC, bool EP, int WM = 2, bool PART = false, bool KT = false, int ADD = 0>
__device__ __forceinline__ void gemm_pipe2_body(const GemmArgs &g, int bx, int by, int bz, const GemmAddend *ad = nullptr) {
    constexpr int BM = 32 * WM, BN = 64, BK = kPipeBK, NT = 256 * WM, NTB = 512, PER = BM * BK / 4 / NT, KG = BK / 4,
                  OCT = BK / 8 / 2;   // OCT: octets of a stage per wave group
    static_assert(PER == 1 && BN * BK / 4 / NTB == 1, "one k-group per thread and operand");
    __shared__ __align__(16) float As_static[ADD ? 1 : 2][ADD ? 4 : BK * BM];
    __shared__ __align__(16) float Bs_static[ADD ? 1 : 2][ADD ? 4 : BK * BN];
    float (*As)[BK * BM], (*Bs)[BK * BN];
    if constexpr (ADD != 0) {
        extern __shared__ __align__(16) float hm_pipe_dyn_lds[];
        As = reinterpret_cast<float (*)[BK * BM]>(hm_pipe_dyn_lds);
        Bs = reinterpret_cast<float (*)[BK * BN]>(hm_pipe_dyn_lds + 2 * BK * BM);
    } else {
        As = As_static;
        Bs = Bs_static;
    }
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int kpart = wave / (2 * WM), wsub = wave % (2 * WM);   // two wave groups split the octets of every stage
    const int wm = wsub >> 1, wn = wsub & 1;
    const int j = lane & 31, h = lane >> 5;
    const int m0 = bx * BM, n0 = by * BN;
    const int kbeg = bz * g.k_chunk;
    const int stages = g.k_chunk / BK;   // multiple of kPipeD (host)
#ifdef HM_GEMM_PHASE_PROBE
    unsigned long long probe_wait = 0;
#endif
    HM_GEMM_STAMP(0);

    // operand fetches are BUFFER loads: descriptor on the matrix (SGPRs), the thread's own byte offset in ONE loop-invariant
    // VGPR, the stage's offset scalar - no 64-bit address arithmetic on the VALU inside the loop (VALU instructions are
    // serial with the MFMAs of every wave on the SIMD; the fused SDF kernels gained 3 - 11 % from the same change).
    // The host takes this kernel only for operands below 2 GB.
    // The descriptors end at the operands' last element: a K range that is no multiple of the stage group (K = 445, 257)
    // runs to the next multiple, the operand whose k is the SLOW dimension returns zeros beyond its end.  The k-contiguous
    // one reads on into its pad columns or its next row - values that may be NaN or Inf, and 0 * NaN is NaN - so the KT
    // instantiation zeroes them (the host admits a K tail only with split == 1 and at most one k-contiguous operand).
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.A), 0, g.nrecA, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.B), 0, g.nrecB, 0x00020000);
    int va[PER], vb[PER];
    int kla[PER], klb[PER];   // KT only (the grouped kernels set g.K = 0 and never reach it)
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int e = tid + NT * i;
        const int eb = (tid % NTB) + NTB * i;   // (WM = 3: threads 512.. fetch a B k-group again and do not stage it)
        // rows / columns past the edge of a partial tile are clamped HERE, once (they compute values nobody stores)
        const int am = min(m0 + (AKC ? e / KG : e % BM), g.M - 1), bn = min(n0 + (BKC ? eb / KG : eb % BN), g.N - 1);
        va[i] = (int)(4 * (AKC ? (int64_t)am * g.lda + kbeg + (e % KG) * 4
                               : (int64_t)(kbeg + (e / BM) * 4) * g.lda + am));
        vb[i] = (int)(4 * (BKC ? (int64_t)bn * g.ldb + kbeg + (eb % KG) * 4
                               : (int64_t)(kbeg + (eb / BN) * 4) * g.ldb + bn));
        if (KT) {
            kla[i] = g.K - kbeg - (e % KG) * 4;
            klb[i] = g.K - kbeg - (eb % KG) * 4;
        }
    }
    // ADD: the addends' descriptors and the threads' offsets into them at k = kbeg (negative in front of the range)
    __amdgpu_buffer_rsrc_t rsA2 = rsA, rsB2 = rsB;
    int va2[PER], vb2[PER];
    int sa2 = 0, sb2 = 0, lda24 = 0, ldb24 = 0;
    if constexpr (ADD != 0) {
        static_assert(!AKC && !BKC && !KT, "addends are built for the grouped TN form");
        rsA2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(ad->A2), 0, ad->nrecA2, 0x00020000);
        rsB2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(ad->B2), 0, ad->nrecB2, 0x00020000);
        lda24 = 4 * ad->lda2;
        ldb24 = 4 * ad->ldb2;
        sa2 = BK * lda24;
        sb2 = BK * ldb24;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = tid + NT * i;
            const int eb = (tid % NTB) + NTB * i;
            const int am = min(m0 + e % BM, g.M - 1), bn = min(n0 + eb % BN, g.N - 1);
            va2[i] = 4 * ((kbeg + (e / BM) * 4 - ad->a_k0) * ad->lda2 + am);   // (|.| < 2^31: host)
            vb2[i] = 4 * ((kbeg + (eb / BN) * 4 - ad->b_k0) * ad->ldb2 + bn);
        }
    }
#define HM_PIPE_MASK(S_, N_)                                                                        \
    do {                                                                                            \
        if (KT) {                                                                                   \
            pipe_mask_tail<AKC, PER>(ra##N_, kla, (S_) * BK);                                       \
            pipe_mask_tail<BKC, PER>(rb##N_, klb, (S_) * BK);                                       \
        }                                                                                           \
        if constexpr ((ADD & 1) != 0) pipe_add<PER>(ra##N_, qa##N_);                                \
        if constexpr ((ADD & 2) != 0) pipe_add<PER>(rb##N_, qb##N_);                                \
    } while (0)
    const bool stage_b = NT == NTB || tid < NTB;
    const int sa = 4 * (AKC ? BK : BK * (int)g.lda), sb = 4 * (BKC ? BK : BK * (int)g.ldb);   // bytes per stage
    const int lda4 = 4 * (int)g.lda, ldb4 = 4 * (int)g.ldb;
    f32x16 acc, acc2;   // even / odd k-octets: two independent MFMA chains for the one wave on each SIMD
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = acc2[r] = 0.0f;
    // the four ring slots and the two operand sets are separate named arrays (an array indexed by (u+3)%4 inside
    // the unrolled loop was demoted to scratch memory by hipcc)
    static_assert(kPipeD == 4, "the stage macro below is written out for a 4-deep ring (8-deep measured no faster)");
    float4 ra0[PER], ra1[PER], ra2[PER], ra3[PER], rb0[PER], rb1[PER], rb2[PER], rb3[PER];
    float4 qa0[PER], qa1[PER], qa2[PER], qa3[PER], qb0[PER], qb1[PER], qb2[PER], qb3[PER];   // ADD: the addends' ring
    float4 opa0[OCT], opa1[OCT], opb0[OCT], opb1[OCT];
#define HM_PIPE_FETCH(S_, F_)                                                                       \
    do {                                                                                            \
        const int sc_ = min((S_), stages - 1); /* past the end: re-read the last stage, never multiplied */ \
        pipe_fetch_buf<AKC, PER>(rsA, va, sc_ * sa, lda4, ra##F_);                                  \
        pipe_fetch_buf<BKC, PER>(rsB, vb, sc_ * sb, ldb4, rb##F_);                                  \
        if constexpr ((ADD & 1) != 0) pipe_fetch_add<PER>(rsA2, va2, sc_ * sa2, lda24, qa##F_);     \
        if constexpr ((ADD & 2) != 0) pipe_fetch_add<PER>(rsB2, vb2, sc_ * sb2, ldb24, qb##F_);     \
    } while (0)
    HM_PIPE_FETCH(0, 0);
    HM_PIPE_FETCH(1, 1);
    HM_PIPE_FETCH(2, 2);
    HM_PIPE_MASK(0, 0);
    store_tile<BM, BK, NT>(As[0], AKC, tid, ra0);
    if (stage_b) store_tile<BN, BK, NTB>(Bs[0], BKC, tid, rb0);
    __syncthreads();
    HM_GEMM_STAMP(1);
    pipe_read_ops<OCT, BM>(As[0], Bs[0], wm * 32 + j, wn * 32 + j, h + 4 * kpart, opa0, opb0);
// one stage: multiply from operand set C, meanwhile fetch stage s+D-1 into ring slot F and move ring slot N (stage
// s+1) through LDS buffer NB into operand set X
#define HM_PIPE_STAGE(S_, F_, N_, C_, X_, NB_)                                                      \
    do {                                                                                            \
        HM_PIPE_FETCH((S_) + kPipeD - 1, F_);                                                       \
        pipe_mfma_oct(opa##C_[0], opb##C_[0], acc);                                                 \
        HM_PIPE_MASK((S_) + 1, N_);                                                                 \
        store_tile<BM, BK, NT>(As[NB_], AKC, tid, ra##N_);                                          \
        if (stage_b) store_tile<BN, BK, NTB>(Bs[NB_], BKC, tid, rb##N_);                            \
        HM_GEMM_LOOP_BARRIER();                                                                     \
        pipe_read_ops<OCT, BM>(As[NB_], Bs[NB_], wm * 32 + j, wn * 32 + j, h + 4 * kpart, opa##X_, opb##X_);        \
        pipe_mfma_oct(opa##C_[1], opb##C_[1], acc2);                                                \
    } while (0)
    static_assert(OCT == 2, "HM_PIPE_STAGE is written for 2 octets per stage and wave group");
    for (int s0 = 0; s0 < stages; s0 += kPipeD) {
        HM_PIPE_STAGE(s0 + 0, 3, 1, 0, 1, 1);
        HM_PIPE_STAGE(s0 + 1, 0, 2, 1, 0, 0);
        HM_PIPE_STAGE(s0 + 2, 1, 3, 0, 1, 1);
        HM_PIPE_STAGE(s0 + 3, 2, 0, 1, 0, 0);
    }
#undef HM_PIPE_STAGE
#undef HM_PIPE_MASK
#undef HM_PIPE_FETCH
    HM_GEMM_STAMP(2);
#ifdef HM_GEMM_PHASE_PROBE
    if (HM_GEMM_PROBE_ON) hm_gemm_probe_ts[5] = probe_wait;
#endif
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] += acc2[r];
    // The two wave groups hold partial sums of the same tile.  Each FINISHES half of it: group 0 the rows of registers
    // 0..7 (rows 0..15 of the wave's 32), group 1 those of registers 8..15; the other eight registers go to the partner
    // wave through the staging buffers (free now).  Every element is group 0's sum + group 1's, in either group (fp32
    // addition commutes), and all waves share the epilogue's loads, transcendentals and stores.
    float fin[8];
    float *red = &As[0][0];   // 4 WM waves * 8 registers * 64 lanes floats == 2 * BK * BM
    static_assert(2 * BK * BM == 4 * WM * 8 * 64, "exchange buffer");
    float *const mine = red + (kpart * 2 * WM + wsub) * 512, *const theirs = red + ((1 - kpart) * 2 * WM + wsub) * 512;
    {
        float give[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            fin[q] = kpart ? acc[8 + q] : acc[q];
            give[q] = kpart ? acc[q] : acc[8 + q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) mine[q * 64 + lane] = give[q];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) fin[q] += theirs[q * 64 + lane];
    }
    HM_GEMM_STAMP(3);
    const int mrow = m0 + wm * 32 + 16 * kpart;   // first of the wave's 16 rows
    const bool add_bias = (g.bias != nullptr) && (bz == 0);
    if (g.vec_out) {
        // 16-byte form: the accumulator layout has the lane on ONE column, so the wave turns its 16 x 32 block through
        // LDS - `theirs`, which only this wave reads and has read - into row-major quads: 8 lanes span a row's 32 columns
        // (128 B), the wave 8 rows per access.  Row pairs share a 64-float line; the halves swap with bit 2 of the row so
        // that the two lane halves (rows r and r + 4) write different banks.
        auto slot = [](int row, int col) { return (row >> 1) * 64 + (((row ^ (row >> 2)) & 1) * 32) + col; };
#pragma unroll
        for (int q = 0; q < 8; ++q) theirs[slot((q & 3) + 8 * (q >> 2) + 4 * h, j)] = fin[q];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int row = lane >> 3, col = (lane & 7) * 4;
        float4 quad[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) quad[i] = *reinterpret_cast<const float4 *>(theirs + slot(row + 8 * i, col));
        const int n = n0 + wn * 32 + col;
        if (n < g.N) gemm_store_quads<EP, PART>(g, quad, n, mrow + row, add_bias, bz);
    } else {
        const int n = n0 + wn * 32 + j;
        if (n < g.N) gemm_store_oct<EP, PART>(g, fin, n, mrow + 4 * h, add_bias, bz);
    }
    HM_GEMM_STAMP(4);
}

template <bool AKC, bool BKC, bool EP>
__global__ __launch_bounds__(512, 4) void gemm_f32_pipe2_kernel(GemmArgs g) {
    gemm_pipe2_body<AKC, BKC, EP>(g, blockIdx.x, blockIdx.y, blockIdx.z);
}
template <bool AKC, bool BKC, bool EP>
__global__ __launch_bounds__(768, 3) void gemm_f32_pipe2_m96_kernel(GemmArgs g) {
    gemm_pipe2_body<AKC, BKC, EP, 3>(g, blockIdx.x, blockIdx.y, blockIdx.z);
}
template <bool AKC, bool BKC, bool EP>
__global__ __launch_bounds__(512, 4) void gemm_f32_pipe2_ktail_kernel(GemmArgs g) {
    gemm_pipe2_body<AKC, BKC, EP, 2, false, true>(g, blockIdx.x, blockIdx.y, blockIdx.z);
}
template <bool AKC, bool BKC, bool EP>
__global__ __launch_bounds__(768, 3) void gemm_f32_pipe2_m96_ktail_kernel(GemmArgs g) {
    gemm_pipe2_body<AKC, BKC, EP, 3, false, true>(g, blockIdx.x, blockIdx.y, blockIdx.z);
}
template <bool AKC, bool BKC>
__global__ __launch_bounds__(512, 4) void gemm_f32_pipe2_part_kernel(GemmArgs g) {
    gemm_pipe2_body<AKC, BKC, false, 2, true>(g, blockIdx.x, blockIdx.y, blockIdx.z);
}
template <bool AKC, bool BKC>
__global__ __launch_bounds__(768, 3) void gemm_f32_pipe2_m96_part_kernel(GemmArgs g) {
    gemm_pipe2_body<AKC, BKC, false, 3, true>(g, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Grouped form for the weight gradients of one backward pass: C_p += A_p^T B_p for up to HM_GEMM_GROUP_MAX problems in ONE
// launch (A_p [K_p, M_p], B_p [K_p, N_p] row-major: both operands row-contiguous, the shape of  dW = [u; z-bar]^T [v-bar; a]).
// Launched one by one these GEMMs are 64 tiles each and need an 8-way split-K (and a zeroing launch) to fill the chip
// at all: 33 - 45 us per layer for 14 - 20 us of matrix work.  Here every (problem, tile, k part) is a workgroup of
// the same grid: ~1000 of them, four resident per CU, so that one problem's tail overlaps the next one's head.
struct GemmGroupEntry {
    const float *A, *B;
    float *C;
    int64_t lda, ldb, ldc;
    int32_t M, N, k_chunk, tiles_m, tiles_n, split;
};
struct GemmGroupTable {
    GemmGroupEntry e[HM_GEMM_GROUP_MAX];
    int32_t start[HM_GEMM_GROUP_MAX + 1];
    int32_t n;
};
// PART: deterministic form - every problem's E.C is its workspace slab base (E.ldc = N), partials go there with plain
// stores and gemm_part_reduce_kernel adds them to the real C in k-part order.
// the grouped form with addends: the same table plus one GemmAddend per problem
struct GemmGroupAddTable {
    GemmGroupTable t;
    GemmAddend ad[HM_GEMM_GROUP_MAX];
};
template <bool PART, bool ADD = false>
__device__ __forceinline__ void gemm_group_body(const GemmGroupTable &t, const GemmAddend *ads = nullptr) {
    int p = 0;
    while (p + 1 < t.n && (int)blockIdx.x >= t.start[p + 1]) ++p;       // (uniform: <= 16 problems)
    const GemmGroupEntry &E = t.e[p];
    int local = (int)blockIdx.x - t.start[p];
    const int bz = local % E.split;
    local /= E.split;
    const int by = local % E.tiles_n, bx = local / E.tiles_n;
    GemmArgs g;
    g.A = E.A; g.B = E.B; g.bias = nullptr; g.C = E.C;
    g.M = E.M; g.N = E.N; g.K = 0;
    g.transA = 1; g.transB = 0;
    g.lda = E.lda; g.ldb = E.ldb; g.ldc = E.ldc;
    g.k_chunk = E.k_chunk;
    g.atomic = 1;
    g.vecA = g.vecB = 0;
    g.vec_out = 0;   // (atomics, or the slabs of the deterministic form: dword stores)
    g.nrecA = g.nrecB = 0x7fffffff;
    g.ep.mode = HM_EPI_NONE;
    if constexpr (ADD) {
        // which addend can this workgroup's k part meet?  Uniform, decided in front of the K loop: on the training step
        // A's range (z-bar rows) and B's (v-bar rows) lie in different k parts, so a workgroup fetches one of them
        const GemmAddend &D = ads[p];
        const int kbeg = bz * E.k_chunk, kend = kbeg + E.k_chunk;
        const bool oa = D.a_k0 < kend && D.a_k1 > kbeg, ob = D.b_k0 < kend && D.b_k1 > kbeg;
        if (oa && ob)
            gemm_pipe2_body<false, false, false, 2, PART, false, 3>(g, bx, by, bz, &D);
        else if (ob)
            gemm_pipe2_body<false, false, false, 2, PART, false, 2>(g, bx, by, bz, &D);
        else   // (neither: A's descriptor is empty or never met - zeros)
            gemm_pipe2_body<false, false, false, 2, PART, false, 1>(g, bx, by, bz, &D);
    } else
        gemm_pipe2_body<false, false, false, 2, PART>(g, bx, by, bz);
}
__global__ __launch_bounds__(512, 4) void gemm_f32_pipe2_group_kernel(GemmGroupTable t) {
    gemm_group_body<false>(t);
}
__global__ __launch_bounds__(512, 4) void gemm_f32_pipe2_group_part_kernel(GemmGroupTable t) {
    gemm_group_body<true>(t);
}
__global__ __launch_bounds__(512, 4) void gemm_f32_pipe2_group_add_kernel(GemmGroupAddTable t) {
    gemm_group_body<false, true>(t.t, t.ad);
}
__global__ __launch_bounds__(512, 4) void gemm_f32_pipe2_group_add_part_kernel(GemmGroupAddTable t) {
    gemm_group_body<true, true>(t.t, t.ad);
}

// Deterministic split-K, second pass: C = C_old + (((p0 + p1) + p2) + ...) (accumulate) or C = ((p0 + p1) + ...),
// the partials p_k read from the workspace slabs of gemm_*_part_kernel in k-part order - the summation order depends
// on the shape only.  One launch serves every problem of a call: thread i of problem p owns element i - start[p].
struct GemmReduceEntry {
    const float *P;   // split slabs of M x N floats
    float *C;
    int64_t ldc, start;   // start: first flat element of this problem in the launch
    int32_t M, N, split, accumulate;
};
struct GemmReduceTable {
    GemmReduceEntry e[HM_GEMM_GROUP_MAX];
    int64_t end;
    int32_t n;
};
__global__ __launch_bounds__(256) void gemm_part_reduce_kernel(GemmReduceTable t) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= t.end) return;
    int p = 0;
    while (p + 1 < t.n && i >= t.e[p + 1].start) ++p;
    const GemmReduceEntry &E = t.e[p];
    const int64_t e = i - E.start, mn = (int64_t)E.M * E.N;
    const int64_t m = e / E.N, n = e - m * E.N;
    float s = E.P[e];
    for (int k = 1; k < E.split; ++k) s = __fadd_rn(s, E.P[k * mn + e]);
    float *dst = E.C + m * E.ldc + n;
    *dst = E.accumulate ? __fadd_rn(*dst, s) : s;
}

// zero an M x N window of C (split-K accumulates with atomics); a plain kernel instead of
// hipMemset2DAsync so that the call can be recorded into a HIP graph on every ROCm version
__global__ __launch_bounds__(256) void zero_window_kernel(float *C, int64_t ldc, int64_t M, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * N) return;
    const int64_t m = i / N, n = i - m * N;
    C[m * ldc + n] = 0.0f;
}

constexpr unsigned kGroupAddLds = 4 * 2 * kPipeBK * (64 + 64);   // dynamic LDS of the grouped addend kernels (bytes)
constexpr int64_t kSplitTarget = 512;   // split-K: workgroups to aim for when the tile grid alone leaves the chip idle

}  // namespace

// Tile, kernel and split-K decomposition of one GEMM: a function of the shape (and, for the 16-byte loads of the
// generic and big kernels, of the operands' alignment), so that the deterministic workspace query
// (hm_gemm_f32_det_workspace_bytes), the launch and hm_diag_gemm_plan agree.
struct GemmPlan {
    bool big, use_pipe, pipe_ok, m96;
    bool k_tail;        // pipelined kernel on a K that is no multiple of the stage group (KT instantiation)
    bool vecA, vecB;    // generic / big kernel: 16-byte operand loads
    int64_t bm, bn, split, k_chunk;
    int64_t bytesA, bytesB;   // extent of each operand from its base (the pipelined kernels' buffer descriptors)
};
static GemmPlan gemm_plan(int transA, int transB, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda,
                          const void *B, int64_t ldb, bool has_ep) {
    GemmPlan P;
    const bool a_kc = !transA, b_kc = transB != 0;
    // operands may be fetched with 16-B loads when every k-group of every row is 16-B aligned
    // (and the K range ends on a multiple of 4, so no k-group straddles the end)
    P.vecA = a_kc && K % 4 == 0 && lda % 4 == 0 && (reinterpret_cast<uintptr_t>(A) & 15u) == 0;
    P.vecB = b_kc && K % 4 == 0 && ldb % 4 == 0 && (reinterpret_cast<uintptr_t>(B) & 15u) == 0;
    // tile choice: big tiles only when they still fill the chip
    const int64_t t128 = ((M + 127) / 128) * ((N + 127) / 128);
    P.big = t128 >= 256;
    // (128x64 / 64x128 tiles and a forced 128x128 tile were measured too: 30-45 % slower on M = 1750...4822; 32-row tiles
    // for row counts whose 64-row grid gives a CU fewer than two workgroups made the training step 2 % SLOWER - twice the
    // B-panel traffic outweighs the extra overlap)
    const int64_t t64 = ((M + 63) / 64) * ((N + 63) / 64);
    // the pipelined kernel fetches through buffer descriptors with 32-bit offsets, so it takes operands below 2 GB only
    // (every other operand runs on the generic kernel, which addresses rows in 64 bits), and K ranges that are a whole
    // number of 128-deep groups per split (partial edge tiles are fine: clamped rows, guarded stores).  Its 16-byte loads
    // need dword alignment only (unaligned buffer_load_dwordx4 returns the right dwords: the misaligned and padded operand
    // views of tests/test_gemm_paths_gpu.py run here and are bit-exact), so k-contiguous operands with any leading
    // dimension qualify, and a K TAIL is admitted when one operand has k as its slow dimension: the K range runs to the
    // next multiple of the stage group, that operand's descriptor returns zeros beyond its end and the KT instantiation
    // zeroes the other's k >= K elements (K = 445 and 257 of the backward sweeps: 27 - 43 us on the generic kernel).
    P.bytesA = 4 * ((transA ? K - 1 : M - 1) * lda + (transA ? M : K));
    P.bytesB = 4 * ((transB ? N - 1 : K - 1) * ldb + (transB ? K : N));
    const bool buf_ok = P.bytesA < (1ll << 31) && P.bytesB < (1ll << 31);
    const bool k_whole = K % (kPipeBK * kPipeD) == 0;
    // (K >= 192: below that the rounded-up range costs more than the generic kernel's guards - K = 72 of the filter banks)
    // (and only where the generic kernel would not split K over workgroups: a tail runs as ONE chunk, so the small
    //  M x N weight-gradient shapes of the eager path - K = number of points - keep their split-K launch)
    const bool k_tail_ok = (!a_kc || !b_kc) && K >= 192 && (has_ep || t64 >= 256);
    P.use_pipe = !P.big && K > 0 && buf_ok && (k_whole || k_tail_ok);
    // 96-row tiles when they need fewer rounds of the chip per row of the tile (M = 3072, N = 512: 384 tiles of 64 rows -
    // the slowest CU runs two = 128 rows' worth - against 256 tiles of 96)
    const int64_t t96 = ((M + 95) / 96) * ((N + 63) / 64);
    P.m96 = P.use_pipe && ((t96 + 255) / 256) * 96 < ((t64 + 255) / 256) * 64;
    P.bm = P.big ? 128 : (P.m96 ? 96 : 64);
    P.bn = P.big ? 128 : 64;
    const int64_t kBK = P.big ? 32 : (P.use_pipe ? kPipeBK * kPipeD : 128);
    const int64_t tiles = ((M + P.bm - 1) / P.bm) * ((N + P.bn - 1) / P.bn);
    int64_t split = 1;
    if (tiles < 256 && K >= 256 && !has_ep && !(P.use_pipe && !k_whole)) {   // (a nonlinear epilogue needs the
                                                                             // full sum; a K tail is not split)
        split = (kSplitTarget + tiles - 1) / tiles;
        const int64_t max_split = K / 128;
        if (split > max_split) split = max_split;
        if (split < 1) split = 1;
    }
    int64_t k_chunk = (K + split - 1) / split;
    k_chunk = ((k_chunk + kBK - 1) / kBK) * kBK;
    if (k_chunk == 0) k_chunk = kBK;
    // the pipelined kernel has no K tail: grow the chunk until it divides K (K = 6144 over 10 splits: 640 -> 768)
    while (P.use_pipe && k_whole && K % k_chunk != 0 && k_chunk < K) k_chunk += kBK;
    P.split = K > 0 ? (K + k_chunk - 1) / k_chunk : 1;
    P.k_chunk = k_chunk;
    // (whole K: the chunks divide it; K tail: ONE chunk of the rounded-up K, zeros beyond the slow operand's end)
    P.pipe_ok = P.use_pipe && (k_whole ? K % k_chunk == 0 : P.split == 1);
    P.k_tail = P.pipe_ok && !k_whole;
    return P;
}

// May the pipelined kernel's tail use 16-byte accesses (gemm_store_quads)?  Nothing accumulated with atomics, N (and nz) a
// multiple of 4 so that no quad straddles an edge, and every pointer and row stride the tail touches 16-byte aligned - true of
// the 512-wide chain tensors and of the row slices of the stacked buffers, not of the 445- / 257- / 67-column ones.
static bool gemm_vec_out(const GemmArgs &g, bool part) {
    auto ok = [](const void *p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && ld % 4 == 0; };
    if ((g.atomic && !part) || g.N % 4 != 0 || !ok(g.C, g.ldc)) return false;   // (a NULL C is never touched)
    const hm_gemm_epilogue &e = g.ep;
    if (e.mode == HM_EPI_NONE) return true;
    const bool masked = e.mode == HM_EPI_S1MUL || e.mode == HM_EPI_RELUMASK;
    const bool has_z = masked || e.mode == HM_EPI_ADJOINT;
    if (!ok(e.out1, e.ld1) || (masked && e.nz % 4 != 0)) return false;
    if (has_z && (!ok(e.z, e.ldz) || (e.g && !ok(e.g, e.ldg)))) return false;
    if (e.mode == HM_EPI_ADJOINT && (!ok(e.out2, e.ld2) || (e.out3 && !ok(e.out3, e.ld3)))) return false;
    return true;
}

// deterministic split-K: bytes of k-part slabs a call needs (0 when K is not split)
static int64_t gemm_det_bytes(const GemmPlan &P, int64_t M, int64_t N) {
    return P.split > 1 ? 4 * P.split * M * N : 0;
}

static int launch_part_reduce(const GemmReduceTable &t, hipStream_t st) {
    if (t.end == 0) return HM_OK;
    HM_CHECK_ARG((t.end + 255) / 256 < (1ll << 31), "hm_gemm_f32_det: too many elements for one reduce launch");
    hipLaunchKernelGGL(gemm_part_reduce_kernel, dim3((unsigned)((t.end + 255) / 256)), dim3(256), 0, st, t);
    return HM_OK;
}

// det: a split K goes through k-part slabs in ws (ws_bytes >= gemm_det_bytes) and gemm_part_reduce_kernel instead of
// atomics; an unsplit K is the default launch (one adder per element)
static int gemm_impl(int transA, int transB, int64_t M, int64_t N, int64_t K, const float *A, int64_t lda,
                     const float *B, int64_t ldb, const float *bias, float *C, int64_t ldc, int accumulate,
                     const hm_gemm_epilogue *ep, void *stream, bool det = false, float *ws = nullptr,
                     int64_t ws_bytes = 0) {
    HM_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "hm_gemm_f32: negative dimension");
    HM_CHECK_ARG(M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31), "hm_gemm_f32: dimension too large");
    if (M == 0 || N == 0) return HM_OK;
    HM_CHECK_ARG(C != nullptr || (ep && ep->mode != HM_EPI_NONE), "hm_gemm_f32: C is NULL");
    HM_CHECK_ARG(K == 0 || (A && B), "hm_gemm_f32: NULL operand");
    HM_CHECK_ARG(lda >= (transA ? M : K) && ldb >= (transB ? K : N) && (!C || ldc >= N), "hm_gemm_f32: leading dimension");
    GemmArgs g;
    g.ep = hm_gemm_epilogue{};
    if (ep && ep->mode != HM_EPI_NONE) {
        HM_CHECK_ARG(!accumulate, "hm_gemm_f32_ep: an epilogue cannot be combined with accumulate");
        HM_CHECK_ARG(ep->mode >= HM_EPI_SOFTPLUS && ep->mode <= HM_EPI_RELUMASK, "hm_gemm_f32_ep: unknown epilogue mode");
        const bool masked = ep->mode == HM_EPI_S1MUL || ep->mode == HM_EPI_RELUMASK;   // out1 has nz columns
        HM_CHECK_ARG(ep->out1 && ep->ld1 >= (masked ? ep->nz : N), "hm_gemm_f32_ep: out1");
        if (ep->mode != HM_EPI_SOFTPLUS && ep->mode != HM_EPI_RELU) {
            const int64_t nzc = masked ? ep->nz : N;
            HM_CHECK_ARG(ep->z && ep->ldz >= nzc, "hm_gemm_f32_ep: z");
            HM_CHECK_ARG(!masked || (ep->nz >= 1 && ep->nz <= N), "hm_gemm_f32_ep: nz out of range");
            HM_CHECK_ARG(!ep->g || ep->ldg >= nzc, "hm_gemm_f32_ep: g");
        }
        if (ep->mode == HM_EPI_ADJOINT) {
            HM_CHECK_ARG(ep->g && ep->out2 && ep->ld2 >= N && (!ep->out3 || ep->ld3 >= N), "hm_gemm_f32_ep: ADJOINT operands");
        }
        g.ep = *ep;
    }
    g.A = A; g.B = B; g.bias = bias; g.C = C;
    g.M = (int)M; g.N = (int)N; g.K = (int)K;
    g.transA = transA; g.transB = transB;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    const GemmPlan P = gemm_plan(transA, transB, M, N, K, A, lda, B, ldb, g.ep.mode != HM_EPI_NONE);
    g.vecA = P.vecA ? 1 : 0;
    g.vecB = P.vecB ? 1 : 0;
    const bool big = P.big, m96 = P.m96, pipe_ok = P.pipe_ok;
    const int64_t bm = P.bm, bn = P.bn, split = P.split;
    g.nrecA = (int32_t)(P.bytesA < 0x7fffffff ? P.bytesA : 0x7fffffff);
    g.nrecB = (int32_t)(P.bytesB < 0x7fffffff ? P.bytesB : 0x7fffffff);
    g.k_chunk = (int)P.k_chunk;
    const bool part = det && split > 1;
    if (part) {
        HM_CHECK_ARG(ws != nullptr && ws_bytes >= gemm_det_bytes(P, M, N), "hm_gemm_f32_det: workspace too small");
        g.C = ws;
        g.ldc = N;
    }
    g.atomic = (accumulate || split > 1) ? 1 : 0;
    g.vec_out = gemm_vec_out(g, part) ? 1 : 0;
    if (split > 1 && !accumulate && !part) {
        // split-K accumulates with atomics into a zeroed C
        hipLaunchKernelGGL(zero_window_kernel, dim3((unsigned)((M * N + 255) / 256)), dim3(256), 0, as_stream(stream),
                           C, ldc, M, N);
    }
    dim3 grid((unsigned)((M + bm - 1) / bm), (unsigned)((N + bn - 1) / bn), (unsigned)split);
    HM_CHECK_ARG(grid.y <= 65535u && grid.z <= 65535u, "hm_gemm_f32: N or split too large for one launch");
    hipStream_t st = as_stream(stream);
    const bool ep_on = g.ep.mode != HM_EPI_NONE;
    // every kernel instance is named once below: the run-time choices become template values, one launch form
    auto launch = [&](auto kernel, unsigned threads) { hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, st, g); };
    if (big || !pipe_ok) {   // tile kernels: 16-byte operand loads are template values
        hm_bool_dispatch(P.vecA, [&](auto va) {
            hm_bool_dispatch(P.vecB, [&](auto vb) {
                constexpr bool VA = decltype(va)::value, VB = decltype(vb)::value;
                // (big tiles are never split: they are taken only when the tile grid alone fills the chip)
                if (part) return launch(gemm_f32_kernel<1, 1, 128, 2, VA, VB, false, 2, true>, 512);
                hm_bool_dispatch(ep_on, [&](auto ep_c) {
                    constexpr bool EP = decltype(ep_c)::value;
                    if (big) launch(gemm_f32_kernel<2, 2, 32, 1, VA, VB, EP, 2>, 256);
                    else launch(gemm_f32_kernel<1, 1, 128, 2, VA, VB, EP, 2>, 512);
                });
            });
        });
    } else {   // pipelined kernels: which operands are k-contiguous
        hm_bool_dispatch(!transA, [&](auto akc) {
            hm_bool_dispatch(transB != 0, [&](auto bkc) {
                constexpr bool AKC = decltype(akc)::value, BKC = decltype(bkc)::value;
                if (part) {
                    if (m96) launch(gemm_f32_pipe2_m96_part_kernel<AKC, BKC>, 768);
                    else launch(gemm_f32_pipe2_part_kernel<AKC, BKC>, 512);
                    return;
                }
                hm_bool_dispatch(ep_on, [&](auto ep_c) {
                    constexpr bool EP = decltype(ep_c)::value;
                    // (a K tail has at most one k-contiguous operand; with none, the descriptors alone zero the
                    // k >= K products, so the K-tail instances exist for exactly one k-contiguous operand)
                    if constexpr (AKC != BKC) {
                        if (P.k_tail) {
                            if (m96) launch(gemm_f32_pipe2_m96_ktail_kernel<AKC, BKC, EP>, 768);
                            else launch(gemm_f32_pipe2_ktail_kernel<AKC, BKC, EP>, 512);
                            return;
                        }
                    }
                    if (m96) launch(gemm_f32_pipe2_m96_kernel<AKC, BKC, EP>, 768);
                    else launch(gemm_f32_pipe2_kernel<AKC, BKC, EP>, 512);
                });
            });
        });
    }
    if (part) {
        GemmReduceTable t;
        t.n = 1;
        t.end = M * N;
        t.e[0] = GemmReduceEntry{ws, C, ldc, 0, (int32_t)M, (int32_t)N, (int32_t)split, accumulate ? 1 : 0};
        const int rc = launch_part_reduce(t, st);
        if (rc != HM_OK) return rc;
    }
    HM_CHECK_LAUNCH("hm_gemm_f32");
    return HM_OK;
}

extern "C" {

int hm_gemm_f32(int transA, int transB, int64_t M, int64_t N, int64_t K, const float *A, int64_t lda,
                const float *B, int64_t ldb, const float *bias, float *C, int64_t ldc, int accumulate,
                void *stream) {
    return gemm_impl(transA, transB, M, N, K, A, lda, B, ldb, bias, C, ldc, accumulate, nullptr, stream);
}

int64_t hm_gemm_f32_det_workspace_bytes(int transA, int transB, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return gemm_det_bytes(gemm_plan(transA, transB, M, N, K, nullptr, lda, nullptr, ldb, false), M, N);
}

int hm_diag_gemm_plan(int transA, int transB, int64_t M, int64_t N, int64_t K, const float *A, int64_t lda,
                      const float *B, int64_t ldb, int has_epilogue, int deterministic, hm_gemm_plan_info *info) {
    HM_CHECK_ARG(info != nullptr, "hm_diag_gemm_plan: info is NULL");
    HM_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "hm_diag_gemm_plan: negative dimension");
    *info = hm_gemm_plan_info{};
    if (M == 0 || N == 0) return HM_OK;   // HM_GEMM_KERNEL_NONE: gemm_impl launches nothing
    const GemmPlan P = gemm_plan(transA, transB, M, N, K, A, lda, B, ldb, has_epilogue != 0);
    info->kernel = P.big ? HM_GEMM_KERNEL_BIG
                 : P.pipe_ok ? (P.m96 ? HM_GEMM_KERNEL_PIPE96 : HM_GEMM_KERNEL_PIPE64) : HM_GEMM_KERNEL_GENERIC;
    info->k_tail = P.k_tail ? 1 : 0;
    info->vec_a = P.vecA ? 1 : 0;
    info->vec_b = P.vecB ? 1 : 0;
    info->part = (deterministic && P.split > 1) ? 1 : 0;
    info->split = P.split;
    info->k_chunk = P.k_chunk;
    return HM_OK;
}

int hm_gemm_f32_det(int transA, int transB, int64_t M, int64_t N, int64_t K, const float *A, int64_t lda,
                    const float *B, int64_t ldb, const float *bias, float *C, int64_t ldc, int accumulate,
                    void *workspace, int64_t workspace_bytes, void *stream) {
    return gemm_impl(transA, transB, M, N, K, A, lda, B, ldb, bias, C, ldc, accumulate, nullptr, stream, true,
                     static_cast<float *>(workspace), workspace_bytes);
}

}  // extern "C"

// The grouped calls: ONE routine builds the problem table, so that the deterministic mode sums the partials of the very
// k parts the default mode adds with atomics.  Default (det = false): every table of up to HM_GEMM_GROUP_MAX problems
// is one gemm_f32_pipe2_group_kernel launch that adds into the callers' C (overlapping C windows are fine: atomics).
// Deterministic: partials go to workspace slabs (one launch), then one gemm_part_reduce_kernel launch serves all
// problems of the table.  With run = false only the workspace need is computed
// (hm_gemm_f32_group_tn_det_workspace_bytes): the largest table's slabs, or the largest need of a problem that goes
// alone - the launches of a call follow each other on one stream, so they share the buffer.  who: the entry point.
// Item = hm_gemm_group_add_item: the same routine for items with addends (hm_gemm_f32_group_tn_add*); a table in which
// some problem has a non-empty addend range goes to the kernels' addend instances, every other table to the plain ones.
template <class Item>
static int group_tn(const char *who, const Item *items, int n_items, bool det, float *ws, int64_t ws_bytes,
                    void *stream, bool run, int64_t *need) {
    constexpr bool ADD = std::is_same<Item, hm_gemm_group_add_item>::value;
    HM_CHECK_ARG(n_items >= 0 && (n_items == 0 || items), std::string(who) + ": bad argument");
    *need = 0;
    // byte window of a problem's C: the reduce kernel gives every C element ONE thread, so two problems of one table
    // must not overlap - a problem that overlaps one already in the table starts the next table (the two sums are then
    // added in item order, by two launches)
    auto window = [](const Item &it, uintptr_t &w0, uintptr_t &w1) {
        w0 = reinterpret_cast<uintptr_t>(it.C);
        w1 = w0 + 4 * ((it.M - 1) * it.ldc + it.N);
    };
    int in_table[HM_GEMM_GROUP_MAX];   // item index of every table entry
    GemmGroupAddTable ta;   // (ta.ad is used by the addend form only)
    GemmGroupTable &t = ta.t;
    GemmReduceTable r;
    bool table_adds = false;   // some problem of the current table has a non-empty addend range
    int64_t off = 0;   // floats of workspace the current table uses (deterministic)
    t.n = r.n = 0;
    t.start[0] = 0;
    r.end = 0;
    hipStream_t st = as_stream(stream);
    auto flush = [&]() -> int {
        if (4 * off > *need) *need = 4 * off;
        if (t.n > 0 && run) {
            if (det) {
                HM_CHECK_ARG(ws != nullptr && ws_bytes >= 4 * off, std::string(who) + ": workspace too small");
                for (int p = 0; p < t.n; ++p) t.e[p].C = ws + reinterpret_cast<uintptr_t>(t.e[p].C);   // slab offsets -> pointers
                for (int p = 0; p < r.n; ++p) r.e[p].P = ws + reinterpret_cast<uintptr_t>(r.e[p].P);
                if (table_adds)
                    hipLaunchKernelGGL(gemm_f32_pipe2_group_add_part_kernel, dim3((unsigned)t.start[t.n]), dim3(512), kGroupAddLds, st, ta);
                else
                    hipLaunchKernelGGL(gemm_f32_pipe2_group_part_kernel, dim3((unsigned)t.start[t.n]), dim3(512), 0, st, t);
                const int rc = launch_part_reduce(r, st);
                if (rc != HM_OK) return rc;
            } else if (table_adds)
                hipLaunchKernelGGL(gemm_f32_pipe2_group_add_kernel, dim3((unsigned)t.start[t.n]), dim3(512), kGroupAddLds, st, ta);
            else
                hipLaunchKernelGGL(gemm_f32_pipe2_group_kernel, dim3((unsigned)t.start[t.n]), dim3(512), 0, st, t);
            HM_CHECK_LAUNCH(who);
        }
        table_adds = false;
        t.n = r.n = 0;
        t.start[0] = 0;
        r.end = 0;
        off = 0;
        return HM_OK;
    };
    // deterministic: does the problem's C window overlap one of a problem waiting in the table?
    auto overlaps_table = [&](const Item &it) {
        for (int p = 0; det && p < t.n; ++p) {
            uintptr_t a0, a1, b0, b1;
            window(it, a0, a1);
            window(items[in_table[p]], b0, b1);
            if (!(a1 <= b0 || b1 <= a0)) return true;
        }
        return false;
    };
    for (int i = 0; i < n_items; ++i) {
        const Item &it = items[i];
        HM_CHECK_ARG(it.M >= 0 && it.N >= 0 && it.K >= 0 && it.M < (1ll << 31) && it.N < (1ll << 31) && it.K < (1ll << 31),
                     std::string(who) + ": bad dimension");
        if (it.M == 0 || it.N == 0 || it.K == 0) continue;
        HM_CHECK_ARG(!run || (it.A && it.B && it.C && it.lda >= it.M && it.ldb >= it.N && it.ldc >= it.N),
                     std::string(who) + ": NULL operand or leading dimension");
        const bool grouped = !(it.K % (kPipeBK * kPipeD) != 0 || 4 * it.lda * it.K >= (1ll << 31) || 4 * it.ldb * it.K >= (1ll << 31));
        bool add_a = false, add_b = false;
        if constexpr (ADD) {
            HM_CHECK_ARG(it.a_k0 >= 0 && it.a_k0 <= it.a_k1 && it.a_k1 <= it.K && it.b_k0 >= 0 && it.b_k0 <= it.b_k1 &&
                         it.b_k1 <= it.K, std::string(who) + ": addend range outside [0, K]");
            add_a = it.a_k1 > it.a_k0;
            add_b = it.b_k1 > it.b_k0;
            // an addend runs in the grouped kernel only, over whole k-groups and with 32-bit offsets (the caller pre-adds
            // what does not qualify: ops.gemm_group_tn_add)
            auto ok = [&](bool on, const float *P2, int64_t ld2, int64_t rows, int64_t k0, int64_t k1) {
                return !on || (grouped && (!run || P2) && ld2 >= rows && k0 % 4 == 0 && k1 % 4 == 0 && 4 * ld2 * it.K < (1ll << 31));
            };
            HM_CHECK_ARG(ok(add_a, it.A2, it.lda2, it.M, it.a_k0, it.a_k1) && ok(add_b, it.B2, it.ldb2, it.N, it.b_k0, it.b_k1),
                         std::string(who) + ": addend on an item the grouped kernel does not take, range no multiple of 4, or "
                                            "leading dimension");
        }
        if (!grouped) {
            // no K tail in the pipelined kernel, 32-bit operand offsets: such a problem goes alone, at once - so the
            // table goes first when this problem adds into the C of a problem waiting in it (item order)
            if (overlaps_table(it)) {
                const int rc = flush();
                if (rc != HM_OK) return rc;
            }
            if (det) {
                const int64_t b = gemm_det_bytes(gemm_plan(1, 0, it.M, it.N, it.K, nullptr, it.lda, nullptr, it.ldb, false), it.M, it.N);
                if (b > *need) *need = b;
            }
            if (run) {
                const int rc = gemm_impl(1, 0, it.M, it.N, it.K, it.A, it.lda, it.B, it.ldb, nullptr, it.C, it.ldc, 1,
                                         nullptr, stream, det, ws, ws_bytes);
                if (rc != HM_OK) return rc;
            }
            continue;
        }
        if (t.n == HM_GEMM_GROUP_MAX || overlaps_table(it)) {
            const int rc = flush();
            if (rc != HM_OK) return rc;
        }
        in_table[t.n] = i;
        // k parts of >= 1024 (eight 128-deep groups) that divide K
        int64_t split = it.K / 1024;
        if (split < 1) split = 1;
        if (split > 4) split = 4;
        while (split > 1 && (it.K % split != 0 || (it.K / split) % (kPipeBK * kPipeD) != 0)) --split;
        GemmGroupEntry &E = t.e[t.n];
        E.A = it.A; E.B = it.B;
        E.C = det ? reinterpret_cast<float *>(static_cast<uintptr_t>(off)) : it.C;   // (slab offset until flush)
        E.lda = it.lda; E.ldb = it.ldb; E.ldc = det ? it.N : it.ldc;
        E.M = (int32_t)it.M; E.N = (int32_t)it.N;
        E.tiles_m = (int32_t)((it.M + 63) / 64);
        E.tiles_n = (int32_t)((it.N + 63) / 64);
        E.split = (int32_t)split;
        E.k_chunk = (int32_t)(it.K / split);
        if constexpr (ADD) {
            // no addend: an empty descriptor on the operand itself - every read through it returns zero
            GemmAddend &D = ta.ad[t.n];
            D.A2 = add_a ? it.A2 : it.A;
            D.B2 = add_b ? it.B2 : it.B;
            D.lda2 = add_a ? (int32_t)it.lda2 : 0;
            D.ldb2 = add_b ? (int32_t)it.ldb2 : 0;
            D.a_k0 = add_a ? (int32_t)it.a_k0 : 0;
            D.b_k0 = add_b ? (int32_t)it.b_k0 : 0;
            D.a_k1 = add_a ? (int32_t)it.a_k1 : 0;
            D.b_k1 = add_b ? (int32_t)it.b_k1 : 0;
            D.nrecA2 = add_a ? (int32_t)(4 * ((it.a_k1 - it.a_k0 - 1) * it.lda2 + it.M)) : 0;
            D.nrecB2 = add_b ? (int32_t)(4 * ((it.b_k1 - it.b_k0 - 1) * it.ldb2 + it.N)) : 0;
            table_adds = table_adds || add_a || add_b;
        }
        t.start[t.n + 1] = t.start[t.n] + E.tiles_m * E.tiles_n * E.split;
        ++t.n;
        if (det) {
            r.e[r.n] = GemmReduceEntry{reinterpret_cast<const float *>(static_cast<uintptr_t>(off)), it.C, it.ldc, r.end,
                                       (int32_t)it.M, (int32_t)it.N, (int32_t)split, 1};
            r.end += it.M * it.N;
            off += split * it.M * it.N;
            ++r.n;
        }
    }
    return flush();
}

extern "C" {

int hm_gemm_f32_group_tn(const hm_gemm_group_item *items, int n_items, void *stream) {
    int64_t need = 0;
    return group_tn("hm_gemm_f32_group_tn", items, n_items, false, nullptr, 0, stream, true, &need);
}

int64_t hm_gemm_f32_group_tn_det_workspace_bytes(const hm_gemm_group_item *items, int n_items) {
    int64_t need = 0;
    if (group_tn("hm_gemm_f32_group_tn_det", items, n_items, true, nullptr, 0, nullptr, false, &need) != HM_OK) return -1;
    return need;
}

int hm_gemm_f32_group_tn_det(const hm_gemm_group_item *items, int n_items, void *workspace, int64_t workspace_bytes,
                             void *stream) {
    int64_t need = 0;
    return group_tn("hm_gemm_f32_group_tn_det", items, n_items, true, static_cast<float *>(workspace), workspace_bytes,
                    stream, true, &need);
}

int hm_gemm_f32_group_tn_add(const hm_gemm_group_add_item *items, int n_items, void *stream) {
    int64_t need = 0;
    return group_tn("hm_gemm_f32_group_tn_add", items, n_items, false, nullptr, 0, stream, true, &need);
}

int64_t hm_gemm_f32_group_tn_add_det_workspace_bytes(const hm_gemm_group_add_item *items, int n_items) {
    int64_t need = 0;
    if (group_tn("hm_gemm_f32_group_tn_add_det", items, n_items, true, nullptr, 0, nullptr, false, &need) != HM_OK) return -1;
    return need;
}

int hm_gemm_f32_group_tn_add_det(const hm_gemm_group_add_item *items, int n_items, void *workspace, int64_t workspace_bytes,
                                 void *stream) {
    int64_t need = 0;
    return group_tn("hm_gemm_f32_group_tn_add_det", items, n_items, true, static_cast<float *>(workspace), workspace_bytes,
                    stream, true, &need);
}

#ifdef HM_GEMM_PHASE_PROBE
HM_API int hm_gemm_probe_read(unsigned long long *out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(hm_gemm_probe_ts), sizeof(unsigned long long) * (size_t)(n < 8 ? n : 8)) == hipSuccess ? 0 : -1;
}
#endif

int hm_gemm_f32_ep(int transA, int transB, int64_t M, int64_t N, int64_t K, const float *A, int64_t lda,
                   const float *B, int64_t ldb, const float *bias, float *C, int64_t ldc,
                   const hm_gemm_epilogue *ep, void *stream) {
    HM_CHECK_ARG(ep != nullptr, "hm_gemm_f32_ep: epilogue is NULL");
    return gemm_impl(transA, transB, M, N, K, A, lda, B, ldb, bias, C, ldc, 0, ep, stream);
}

}  // extern "C"
