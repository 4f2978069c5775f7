// hm_nn.hip - exact 1-nearest-neighbour of fp32 points on a uniform grid (the nearest-neighbour step of the
// reference's DTU Chamfer evaluation, evaluation/dtu_eval; contract: include/hashmod.h).
//
//   hm_nn_build   nn_key         key[i] = cell of point i, (cx*gy + cy)*gz + cz
//                 hm_sort_pairs_i32 (stable)  ->  the points of one cell are one run, in ascending original index
//                 nn_records     record r = (x, y, z, original index) of the r-th sorted point, 16 bytes
//                 nn_cell_start  cell_start[c] = first sorted position whose key is >= c (binary search, plain stores)
//   hm_nn_query   nn_key + sort  the queries ordered by their (clamped) cell
//                 nn_query       one wave per 64 consecutive sorted queries, see below
//
// nn_query.  The wave's box is the cell box of its lanes' cells grown by a ring.  Along z the cells of a column
// (cx, cy) are one contiguous run of records, so the box is (x-extent) x (y-extent) ranges.  The lanes look the ranges
// up 64 at a time, a wave prefix sum lays them end to end, and the records are copied to LDS kChunk at a time with one
// coalesced 16-byte load per lane; then EVERY lane tests EVERY staged record, read from LDS at a wave-uniform address
// (a broadcast, no divergent gather).  The result of a lane is therefore the argmin over a superset of what it needs,
// under the total order (d2, original index): it does not depend on which wave or box the query fell into.
// Lanes that are not finished (stopping rule at nn_face_low) make the wave grow the box on all sides by a doubling
// ring; only the new shell is scanned.  A box that covers the grid has no faces left and ends the search.
// The grid record, the cell function, the host-side grid check, the key and cell-table kernels and the stopping rule's
// checked faces (nn_face_low) are in hm_nn_dev.h, shared with hm_nn_radius.hip and hm_mesh_dist.hip.
#include <math.h>

#include "hm_block_dev.h"
#include "hm_nn_dev.h"

namespace {

constexpr int kChunk = 256;   // records staged in LDS per pass (4 KiB)
constexpr int32_t kNoIndex = 0x7fffffff;

__global__ __launch_bounds__(kNT) void nn_records_kernel(const float *__restrict__ p, int64_t n,
                                                         const int64_t *__restrict__ perm, float4 *__restrict__ rec) {
    const int64_t r = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (r >= n) return;
    int64_t i = perm[r];
    if ((uint64_t)i >= (uint64_t)n) i = 0;
    rec[r] = make_float4(p[i * 3], p[i * 3 + 1], p[i * 3 + 2], __int_as_float((int32_t)i));
}

__global__ __launch_bounds__(64) void nn_query_kernel(const float *__restrict__ query, int64_t m,
                                                      const int64_t *__restrict__ qperm,
                                                      const float4 *__restrict__ rec, int64_t n,
                                                      const int32_t *__restrict__ cell_start, NnGrid G, float max_d2,
                                                      float *__restrict__ d2_out, int32_t *__restrict__ idx_out,
                                                      unsigned long long *n_tests) {
    __shared__ float4 stage[kChunk];
    __shared__ int32_t it_beg[64];
    __shared__ int32_t it_off[65];
    const int lane = threadIdx.x;
    const int64_t first_q = (int64_t)blockIdx.x * 64;
    const bool live = first_q + lane < m;
    // a lane past the end repeats the wave's first query, so that it does not widen the box
    int64_t src = qperm[live ? first_q + lane : first_q];
    if ((uint64_t)src >= (uint64_t)m) src = 0;
    const float qx = query[src * 3], qy = query[src * 3 + 1], qz = query[src * 3 + 2];
    bool done = !live || !nn_finite3(qx, qy, qz);

    const int32_t gx = G.g[0], gy = G.g[1], gz = G.g[2];
    const int32_t cx = nn_cell(qx, G.lo[0], G.h, gx), cy = nn_cell(qy, G.lo[1], G.h, gy),
                  cz = nn_cell(qz, G.lo[2], G.h, gz);
    // the box [b0, b1] per axis (wave-uniform), and the box scanned so far [o0, o1]
    int32_t b0x = max(hm_wave_reduce(cx, HmMin{}) - 1, 0), b1x = min(hm_wave_reduce(cx, HmMax{}) + 1, gx - 1);
    int32_t b0y = max(hm_wave_reduce(cy, HmMin{}) - 1, 0), b1y = min(hm_wave_reduce(cy, HmMax{}) + 1, gy - 1);
    int32_t b0z = max(hm_wave_reduce(cz, HmMin{}) - 1, 0), b1z = min(hm_wave_reduce(cz, HmMax{}) + 1, gz - 1);
    int32_t o0x = 0, o1x = -1, o0y = 0, o1y = -1, o0z = 0, o1z = -1;
    int32_t ring = 1;

    float best = INFINITY;
    int32_t best_i = kNoIndex;
    unsigned long long staged = 0;   // records this wave has tested (every lane tests each of them)

    for (;;) {
        const int32_t ny = b1y - b0y + 1;
        const int64_t n_items = (int64_t)(b1x - b0x + 1) * ny * 2;   // two z-ranges per column: below / above the old box
        for (int64_t base = 0; base < n_items; base += 64) {
            const int64_t it = base + lane;
            int32_t s = 0, e = 0;
            if (it < n_items) {
                const int32_t col = (int32_t)(it >> 1), part = (int32_t)(it & 1);
                const int32_t x = b0x + col / ny, y = b0y + col % ny;
                const bool seen = x >= o0x && x <= o1x && y >= o0y && y <= o1y;
                int32_t z0, z1;
                if (!seen) {
                    z0 = part ? 1 : b0z;
                    z1 = part ? 0 : b1z;
                } else {
                    z0 = part ? o1z + 1 : b0z;
                    z1 = part ? b1z : o0z - 1;
                }
                if (z0 <= z1) {
                    const int64_t k = ((int64_t)x * gy + y) * gz;
                    s = cell_start[k + z0];
                    e = cell_start[k + z1 + 1];
                    s = min(max(s, 0), (int32_t)n);
                    e = min(max(e, s), (int32_t)n);
                }
            }
            // the ranges of one group are disjoint parts of [0, n): their lengths sum to < 2^31
            int32_t incl = e - s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int32_t up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            __syncthreads();
            it_beg[lane] = s;
            it_off[lane + 1] = incl;
            if (lane == 0) it_off[0] = 0;
            __syncthreads();
            const int32_t total = it_off[64];
            staged += (unsigned long long)total;
            for (int32_t t0 = 0; t0 < total; t0 += kChunk) {
                const int32_t cnt = min(kChunk, total - t0);
#pragma unroll
                for (int u = 0; u < kChunk / 64; ++u) {
                    const int32_t slot = u * 64 + lane;
                    if (slot < cnt) {
                        const int32_t t = t0 + slot;
                        int a = 0, b = 64;   // the item j with it_off[j] <= t < it_off[j + 1]
                        while (a < b) {
                            const int mid = (a + b) >> 1;
                            if (it_off[mid + 1] <= t) a = mid + 1;
                            else b = mid;
                        }
                        stage[slot] = rec[(int64_t)it_beg[a] + (t - it_off[a])];
                    }
                }
                __syncthreads();
#pragma unroll 4
                for (int32_t c = 0; c < cnt; ++c) {
                    const float4 p = stage[c];
                    const float dx = __fsub_rn(qx, p.x), dy = __fsub_rn(qy, p.y), dz = __fsub_rn(qz, p.z);
                    const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                    const int32_t pi = __float_as_int(p.w);
                    const bool better = d < best || (d == best && pi < best_i);
                    best = better ? d : best;
                    best_i = better ? pi : best_i;
                }
                __syncthreads();
            }
        }

        // the stopping rule (see nn_face_low)
        float b2 = INFINITY;
        if (b0x > 0) {
            const float b = fmaxf(__fsub_rn(qx, nn_face_low(G.lo[0], G.h, gx, b0x)), 0.0f);
            b2 = fminf(b2, __fmul_rn(b, b));
        }
        if (b1x < gx - 1) {
            const float b = fmaxf(__fsub_rn(nn_face_high(G.lo[0], G.h, gx, b1x), qx), 0.0f);
            b2 = fminf(b2, __fmul_rn(b, b));
        }
        if (b0y > 0) {
            const float b = fmaxf(__fsub_rn(qy, nn_face_low(G.lo[1], G.h, gy, b0y)), 0.0f);
            b2 = fminf(b2, __fmul_rn(b, b));
        }
        if (b1y < gy - 1) {
            const float b = fmaxf(__fsub_rn(nn_face_high(G.lo[1], G.h, gy, b1y), qy), 0.0f);
            b2 = fminf(b2, __fmul_rn(b, b));
        }
        if (b0z > 0) {
            const float b = fmaxf(__fsub_rn(qz, nn_face_low(G.lo[2], G.h, gz, b0z)), 0.0f);
            b2 = fminf(b2, __fmul_rn(b, b));
        }
        if (b1z < gz - 1) {
            const float b = fmaxf(__fsub_rn(nn_face_high(G.lo[2], G.h, gz, b1z), qz), 0.0f);
            b2 = fminf(b2, __fmul_rn(b, b));
        }
        // everything beyond the box is at d2 >= b2: no better minimum and no tie when best < b2, nothing to report
        // when b2 > max_d2
        done = done || best < b2 || b2 > max_d2;
        const bool covers = b0x == 0 && b0y == 0 && b0z == 0 && b1x == gx - 1 && b1y == gy - 1 && b1z == gz - 1;
        if (covers || __all(done)) break;

        o0x = b0x, o1x = b1x, o0y = b0y, o1y = b1y, o0z = b0z, o1z = b1z;
        b0x = max(b0x - ring, 0), b1x = (int32_t)min((int64_t)b1x + ring, (int64_t)gx - 1);
        b0y = max(b0y - ring, 0), b1y = (int32_t)min((int64_t)b1y + ring, (int64_t)gy - 1);
        b0z = max(b0z - ring, 0), b1z = (int32_t)min((int64_t)b1z + ring, (int64_t)gz - 1);
        ring = min(ring * 2, 1 << 20);
    }

    if (n_tests && lane == 0) atomicAdd(n_tests, staged * 64ull);   // diagnostic only: an integer count
    if (live) {
        const bool hit = best_i != kNoIndex && best <= max_d2;   // false for a NaN distance
        d2_out[src] = hit ? best : INFINITY;
        idx_out[src] = hit ? best_i : -1;
    }
}

}  // namespace

extern "C" {

int64_t hm_nn_workspace_bytes(int64_t n) {
    if (n < 0 || n >= ((int64_t)1 << 31))
        return hm_fail(HM_ERR_INVALID, "hm_nn_workspace_bytes: n must be in [0, 2^31)");
    return hm_keysort_layout(nullptr, n).bytes;
}

int hm_nn_build(const float *points, int64_t n, const float *lo, float h, const int32_t *g, int32_t *cell_start,
                float *records, void *workspace, int64_t workspace_bytes, int32_t *status, void *stream) {
    HM_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "hm_nn_build: n must be in [1, 2^31)");
    NnGrid G;
    int64_t cells;
    if (int rc = nn_grid(lo, h, g, "hm_nn_build", G, cells)) return rc;
    HM_CHECK_ARG(points && cell_start && records && workspace && status, "hm_nn_build: NULL pointer");
    HM_CHECK_ARG(workspace_bytes >= hm_nn_workspace_bytes(n), "hm_nn_build: workspace too small");
    const HmKeySortWs w = hm_keysort_layout(workspace, n);
    hipStream_t st = as_stream(stream);
    if (int rc = nn_sorted_keys(points, n, G, cells, w, status, 1, stream)) return rc;
    hipLaunchKernelGGL(nn_records_kernel, dim3(hm_grid(n, kNT)), dim3(kNT), 0, st, points, n,
                       static_cast<const int64_t *>(w.perm), reinterpret_cast<float4 *>(records));
    hipLaunchKernelGGL(nn_cell_start_kernel, dim3(hm_grid(cells + 1, kNT)), dim3(kNT), 0, st,
                       static_cast<const int32_t *>(w.keys_sorted), n, cells, cell_start);
    HM_CHECK_LAUNCH("hm_nn_build");
    return HM_OK;
}

int hm_nn_query(const float *query, int64_t m, const float *records, int64_t n, const int32_t *cell_start,
                const float *lo, float h, const int32_t *g, float max_dist2, float *d2, int32_t *index, void *workspace,
                int64_t workspace_bytes, int32_t *status, uint64_t *n_tests, void *stream) {
    HM_CHECK_ARG(m >= 0 && m < ((int64_t)1 << 31), "hm_nn_query: m must be in [0, 2^31)");
    HM_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "hm_nn_query: n must be in [1, 2^31)");
    NnGrid G;
    int64_t cells;
    if (int rc = nn_grid(lo, h, g, "hm_nn_query", G, cells)) return rc;
    HM_CHECK_ARG(!(max_dist2 != max_dist2) && max_dist2 >= 0.0f, "hm_nn_query: max_dist2 must be >= 0 (inf for none)");
    if (m == 0) return HM_OK;
    HM_CHECK_ARG(query && records && cell_start && d2 && index && workspace && status, "hm_nn_query: NULL pointer");
    HM_CHECK_ARG(workspace_bytes >= hm_nn_workspace_bytes(m), "hm_nn_query: workspace too small");
    const HmKeySortWs w = hm_keysort_layout(workspace, m);
    if (int rc = nn_sorted_keys(query, m, G, cells, w, status, 2, stream)) return rc;
    hipLaunchKernelGGL(nn_query_kernel, dim3(hm_grid(m, 64)), dim3(64), 0, as_stream(stream), query, m,
                       static_cast<const int64_t *>(w.perm), reinterpret_cast<const float4 *>(records), n, cell_start,
                       G, max_dist2, d2, index, reinterpret_cast<unsigned long long *>(n_tests));
    HM_CHECK_LAUNCH("hm_nn_query");
    return HM_OK;
}

}  // extern "C"
