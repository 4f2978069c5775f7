// hm_nn_radius.hip - DTU's greedy radius down-sampling of a point cloud on the grid hm_nn_build made (the thinning
// step of the reference's evaluation/dtu_eval; contract: include/hashmod.h).
//
// The reference walks the points in index order: a point that is still marked removes every neighbour within the
// radius.  A point is therefore kept exactly when none of its LOWER-index neighbours is kept (when `curr` is still
// marked all its lower neighbours have been removed already, so the loop changes nothing below `curr`): the
// lexicographically first maximal independent set of the radius graph, which is unique.  Here it is computed in rounds
// over state[r] (r the sorted position of hm_nn_build's records; 0 undecided, 1 kept, 2 removed):
//     an undecided point with a kept lower-index neighbour        -> removed
//     an undecided point whose lower-index neighbours are removed -> kept
//     any other undecided point                                   -> waits for the next round
// j is a neighbour of i when the library's fp32 d2 = (dx*dx + dy*dy) + dz*dz (hm_nn_query's expression, symmetric in
// i and j because fl(a - b) = -fl(b - a)) is <= radius2; the priority is the original index in the record's 4th word.
//
//   hm_nn_radius_begin    nr_begin    state = 0, list = 0 .. n-1 (sorted positions: neighbouring lanes read the same cells)
//   hm_nn_radius_rounds   per round:  nr_round    one lane per listed point: decide (nr_decide), count the block's waiting
//                                     nr_scan     one workgroup: exclusive scan of the blocks' counts, the next count
//                                     nr_scatter  the waiting points, in order, to the other list at offset + rank
//                         or, for <= kTail listed points, nr_tail: one workgroup loops over the rounds
//   hm_nn_radius_finish   nr_finish   keep[original index] = (state == kept)
// The positions of the next list come from prefix sums (block counts, then ranks inside a block); no atomic decides a
// position, and there are no atomic read-modify-writes at all.  No thread waits for another workgroup: a point that
// cannot be decided is left for the next launch.
//
// (a) THE SCAN REACHES EVERY NEIGHBOUR, for any cell edge.  Per axis the lane scans the cells nn_cell(L) .. nn_cell(H)
//     with L = nr_low(p), H = nr_high(p).  nr_low returns an L <= p that it has CHECKED to satisfy
//     fl(fl(p - L)^2) > radius2 (or -inf).  For a point with coordinate q < L, rounding being monotone:
//     fl(p - q) >= fl(p - L) >= 0, fl(dx*dx) >= fl(fl(p - L)^2) > radius2, and adding the non-negative fl(dy*dy),
//     fl(dz*dz) never rounds below the first term: its d2 > radius2, it is no neighbour.  So every neighbour has q >= L,
//     and nn_cell being monotone (hm_nn_dev.h) its cell is >= nn_cell(L) wherever the rounding of the cell assignment
//     put it - a point exactly on a cell face included.  nr_high mirrors this.  Nothing assumes h >= radius: a fine grid
//     gives a wide cell range, one cell gives the whole cloud.  The starting guess p -+ bound (bound: the host's
//     estimate of the radius, rounded outward) is nudged by doubling steps until the check holds; if it never does the
//     end is put at infinity, which the cell function clamps to the grid's first or last cell.
// (b) THE RESULT IS THE SEQUENTIAL LOOP'S, for any thread order.  A state moves only from undecided to a final value.
//     Induction over the index: a point is decided only from FINAL states of lower-index neighbours - removed when one
//     of them is kept, kept when all are removed - and those are the loop's values by induction, so its own value is
//     the loop's.  A lane may read a state while another lane writes it: it sees undecided or the final value; the
//     fresher value only saves a round.
// (c) AT MOST n ROUNDS.  All lower-index neighbours of the lowest-index undecided point are decided before a round
//     starts, so that round decides it: every round with a non-empty list shortens it.  The driver (ops.py) loops until
//     the count it reads is 0 and has no other exit; nr_tail's loop runs at most as many rounds as it has points, which
//     by the same argument is enough.
#include "hm_block_dev.h"
#include "hm_nn_dev.h"

namespace {

constexpr int kTail = 1024;    // a list this short is finished by one workgroup
constexpr int kScanT = 1024;
constexpr uint8_t kUndecided = 0, kKept = 1, kRemoved = 2;

struct NrWs {
    uint8_t *state;      // [n] by sorted position
    int32_t *list[2];    // [n] each: the undecided sorted positions, ascending
    int32_t *bcnt;       // [ceil(n / kNT)] waiting points per block of the round, then their exclusive prefix sum
    int64_t bytes;
};

NrWs nr_layout(void *ws, int64_t n) {
    HmCarve c(ws);
    NrWs w;
    w.state = c.take<uint8_t>(n);
    w.list[0] = c.take<int32_t>(n);
    w.list[1] = c.take<int32_t>(n);
    w.bcnt = c.take<int32_t>((n + kNT - 1) / kNT);
    w.bytes = c.bytes;
    return w;
}

struct NrQuery {
    const float4 *rec;
    const int32_t *cell_start;
    uint8_t *state;
    int64_t n;
    NnGrid G;
    float radius2, bound;
};

__device__ __forceinline__ uint8_t nr_load(uint8_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void nr_store(uint8_t *p, uint8_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a >= b: is a point at b (or beyond it, seen from a) outside the radius by this axis alone?  See (a).
__device__ __forceinline__ bool nr_beyond(float a, float b, float radius2) {
    const float e = __fsub_rn(a, b);
    return __fmul_rn(e, e) > radius2;
}
__device__ __forceinline__ float nr_low(float p, float bound, float radius2) {
    float L = __fsub_rn(p, bound);
    float step = fmaxf(fabsf(p), bound) * 2.3841858e-7f;
    for (int it = 0; it < 48 && !nr_beyond(p, L, radius2); ++it) {
        L = __fsub_rn(L, step);
        step = __fmul_rn(step, 2.0f);
    }
    return nr_beyond(p, L, radius2) ? L : -INFINITY;
}
__device__ __forceinline__ float nr_high(float p, float bound, float radius2) {
    float H = __fadd_rn(p, bound);
    float step = fmaxf(fabsf(p), bound) * 2.3841858e-7f;
    for (int it = 0; it < 48 && !nr_beyond(H, p, radius2); ++it) {
        H = __fadd_rn(H, step);
        step = __fmul_rn(step, 2.0f);
    }
    return nr_beyond(H, p, radius2) ? H : INFINITY;
}

// the new state of the undecided point at sorted position r
__device__ uint8_t nr_decide(const NrQuery &Q, int32_t r) {
    const float4 p = Q.rec[r];
    const int32_t pi = __float_as_int(p.w);
    const NnGrid &G = Q.G;
    const int32_t x0 = nn_cell(nr_low(p.x, Q.bound, Q.radius2), G.lo[0], G.h, G.g[0]);
    const int32_t x1 = nn_cell(nr_high(p.x, Q.bound, Q.radius2), G.lo[0], G.h, G.g[0]);
    const int32_t y0 = nn_cell(nr_low(p.y, Q.bound, Q.radius2), G.lo[1], G.h, G.g[1]);
    const int32_t y1 = nn_cell(nr_high(p.y, Q.bound, Q.radius2), G.lo[1], G.h, G.g[1]);
    const int32_t z0 = nn_cell(nr_low(p.z, Q.bound, Q.radius2), G.lo[2], G.h, G.g[2]);
    const int32_t z1 = nn_cell(nr_high(p.z, Q.bound, Q.radius2), G.lo[2], G.h, G.g[2]);
    bool wait = false;
    for (int32_t x = x0; x <= x1; ++x) {
        for (int32_t y = y0; y <= y1; ++y) {
            // along z the cells of a column are one contiguous run of records
            const int64_t k = ((int64_t)x * G.g[1] + y) * G.g[2];
            int32_t s = Q.cell_start[k + z0], e = Q.cell_start[k + z1 + 1];
            s = min(max(s, 0), (int32_t)Q.n);
            e = min(max(e, s), (int32_t)Q.n);
            for (int32_t j = s; j < e; ++j) {
                const float4 q = Q.rec[j];
                if (__float_as_int(q.w) >= pi) continue;
                const float dx = __fsub_rn(p.x, q.x), dy = __fsub_rn(p.y, q.y), dz = __fsub_rn(p.z, q.z);
                const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                if (!(d <= Q.radius2)) continue;
                const uint8_t st = nr_load(Q.state + j);
                if (st == kKept) return kRemoved;
                wait = wait || st == kUndecided;
            }
        }
    }
    return wait ? kUndecided : kKept;
}

__global__ __launch_bounds__(kNT) void nr_begin_kernel(uint8_t *__restrict__ state, int32_t *__restrict__ list,
                                                       int64_t n, int32_t *__restrict__ info) {
    const int64_t t = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (t < 4) info[t] = t == 0 ? (int32_t)n : 0;
    if (t >= n) return;
    state[t] = kUndecided;
    list[t] = (int32_t)t;
}

__device__ __forceinline__ int32_t nr_count(const int32_t *count, int64_t n) {
    return (int32_t)min((int64_t)max(*count, 0), n);
}

__global__ __launch_bounds__(kNT) void nr_round_kernel(NrQuery Q, const int32_t *__restrict__ list,
                                                       const int32_t *__restrict__ count, int32_t *__restrict__ bcnt) {
    const int64_t t = (int64_t)blockIdx.x * kNT + threadIdx.x;
    bool waiting = false;
    if (t < nr_count(count, Q.n)) {
        const int32_t r = list[t];
        if ((uint32_t)r < (uint64_t)Q.n && nr_load(Q.state + r) == kUndecided) {
            const uint8_t s = nr_decide(Q, r);
            if (s != kUndecided) nr_store(Q.state + r, s);
            waiting = s == kUndecided;
        }
    }
    const int c = __syncthreads_count(waiting);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = c;
}

// bcnt[0 .. nb) -> its exclusive prefix sum; *count_out = the total; one productive round more when *count_in > 0
__global__ __launch_bounds__(kScanT) void nr_scan_kernel(int32_t *__restrict__ bcnt, int64_t nb,
                                                         const int32_t *__restrict__ count_in,
                                                         int32_t *__restrict__ count_out, int32_t *__restrict__ rounds) {
    __shared__ int32_t wsum[kScanT / 64];
    int32_t carry = 0;
    for (int64_t base = 0; base < nb; base += kScanT) {
        const int64_t b = base + threadIdx.x;
        const int32_t v = b < nb ? bcnt[b] : 0;
        int32_t total;
        const int32_t incl = hm_block_scan<kScanT>(v, wsum, total);
        if (b < nb) bcnt[b] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) {
        *count_out = carry;
        if (*count_in > 0) *rounds += 1;
    }
}

__global__ __launch_bounds__(kNT) void nr_scatter_kernel(const int32_t *__restrict__ list,
                                                         const int32_t *__restrict__ count, uint8_t *state, int64_t n,
                                                         const int32_t *__restrict__ boff,
                                                         int32_t *__restrict__ list_out) {
    __shared__ int32_t wsum[kNT / 64];
    const int64_t t = (int64_t)blockIdx.x * kNT + threadIdx.x;
    int32_t r = -1;
    if (t < nr_count(count, n)) r = list[t];
    const bool waiting = (uint32_t)r < (uint64_t)n && nr_load(state + r) == kUndecided;
    int32_t total;
    const int32_t incl = hm_block_scan<kNT>(waiting ? 1 : 0, wsum, total);
    const int64_t dst = (int64_t)boff[blockIdx.x] + incl - 1;
    if (waiting && dst >= 0 && dst < n) list_out[dst] = r;
}

// one workgroup finishes a list of <= kTail points: a round per loop turn, at most as many turns as points, see (c)
__global__ __launch_bounds__(kTail) void nr_tail_kernel(NrQuery Q, const int32_t *__restrict__ list, int32_t *count,
                                                        int32_t *rounds) {
    const int32_t cnt = min(nr_count(count, Q.n), kTail);
    int32_t r = -1;
    if ((int32_t)threadIdx.x < cnt) r = list[threadIdx.x];
    bool waiting = (uint32_t)r < (uint64_t)Q.n && nr_load(Q.state + r) == kUndecided;
    int32_t turns = 0;
    for (int32_t it = 0; it < cnt; ++it) {
        if (!__syncthreads_or(waiting)) break;
        ++turns;
        if (waiting) {
            const uint8_t s = nr_decide(Q, r);
            if (s != kUndecided) nr_store(Q.state + r, s);
            waiting = s == kUndecided;
        }
        __threadfence_block();
    }
    const int left = __syncthreads_count(waiting);
    if (threadIdx.x == 0) {
        *count = left;
        *rounds += turns;
    }
}

__global__ __launch_bounds__(kNT) void nr_finish_kernel(const float4 *__restrict__ rec, int64_t n,
                                                        const uint8_t *__restrict__ state, uint8_t *__restrict__ keep) {
    const int64_t r = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (r >= n) return;
    const int32_t i = __float_as_int(rec[r].w);
    if ((uint32_t)i < (uint64_t)n) keep[i] = state[r] == kKept ? 1 : 0;
}

}  // namespace

extern "C" {

int64_t hm_nn_radius_workspace_bytes(int64_t n) {
    if (n < 0 || n >= ((int64_t)1 << 31))
        return hm_fail(HM_ERR_INVALID, "hm_nn_radius_workspace_bytes: n must be in [0, 2^31)");
    return nr_layout(nullptr, n).bytes;
}

int hm_nn_radius_begin(int64_t n, void *workspace, int64_t workspace_bytes, int32_t *info, void *stream) {
    HM_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "hm_nn_radius_begin: n must be in [1, 2^31)");
    HM_CHECK_ARG(workspace && info, "hm_nn_radius_begin: NULL pointer");
    HM_CHECK_ARG(workspace_bytes >= nr_layout(nullptr, n).bytes, "hm_nn_radius_begin: workspace too small");
    const NrWs w = nr_layout(workspace, n);
    hipLaunchKernelGGL(nr_begin_kernel, dim3(hm_grid(n, kNT)), dim3(kNT), 0, as_stream(stream), w.state, w.list[0], n,
                       info);
    HM_CHECK_LAUNCH("hm_nn_radius_begin");
    return HM_OK;
}

int hm_nn_radius_rounds(const float *records, int64_t n, const int32_t *cell_start, const float *lo, float h,
                        const int32_t *g, float radius2, float bound, int64_t capacity, int64_t round0,
                        int32_t n_rounds, void *workspace, int64_t workspace_bytes, int32_t *info, void *stream) {
    HM_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "hm_nn_radius_rounds: n must be in [1, 2^31)");
    NnGrid G;
    int64_t cells;
    if (int rc = nn_grid(lo, h, g, "hm_nn_radius_rounds", G, cells)) return rc;
    HM_CHECK_ARG(radius2 >= 0.0f, "hm_nn_radius_rounds: radius2 must be >= 0");
    HM_CHECK_ARG(std::isfinite(bound) && bound > 0.0f, "hm_nn_radius_rounds: bound must be positive and finite");
    HM_CHECK_ARG(capacity >= 1 && capacity <= n, "hm_nn_radius_rounds: capacity must be in [1, n]");
    HM_CHECK_ARG(round0 >= 0 && n_rounds >= 1 && n_rounds <= 64, "hm_nn_radius_rounds: round0 >= 0, 1 <= n_rounds <= 64");
    HM_CHECK_ARG(records && cell_start && workspace && info, "hm_nn_radius_rounds: NULL pointer");
    HM_CHECK_ARG(workspace_bytes >= nr_layout(nullptr, n).bytes, "hm_nn_radius_rounds: workspace too small");
    const NrWs w = nr_layout(workspace, n);
    hipStream_t st = as_stream(stream);
    NrQuery Q;
    Q.rec = reinterpret_cast<const float4 *>(records);
    Q.cell_start = cell_start;
    Q.state = w.state;
    Q.n = n;
    Q.G = G;
    Q.radius2 = radius2;
    Q.bound = bound;
    if (capacity <= kTail) {
        const int cur = (int)(round0 & 1);
        hipLaunchKernelGGL(nr_tail_kernel, dim3(1), dim3(kTail), 0, st, Q, static_cast<const int32_t *>(w.list[cur]),
                           info + cur, info + 2);
        HM_CHECK_LAUNCH("hm_nn_radius_rounds");
        return HM_OK;
    }
    const unsigned nb = hm_grid(capacity, kNT);
    for (int32_t i = 0; i < n_rounds; ++i) {
        const int cur = (int)((round0 + i) & 1);
        hipLaunchKernelGGL(nr_round_kernel, dim3(nb), dim3(kNT), 0, st, Q, static_cast<const int32_t *>(w.list[cur]),
                           static_cast<const int32_t *>(info + cur), w.bcnt);
        hipLaunchKernelGGL(nr_scan_kernel, dim3(1), dim3(kScanT), 0, st, w.bcnt, (int64_t)nb,
                           static_cast<const int32_t *>(info + cur), info + (cur ^ 1), info + 2);
        hipLaunchKernelGGL(nr_scatter_kernel, dim3(nb), dim3(kNT), 0, st, static_cast<const int32_t *>(w.list[cur]),
                           static_cast<const int32_t *>(info + cur), w.state, n,
                           static_cast<const int32_t *>(w.bcnt), w.list[cur ^ 1]);
    }
    HM_CHECK_LAUNCH("hm_nn_radius_rounds");
    return HM_OK;
}

int hm_nn_radius_finish(const float *records, int64_t n, void *workspace, int64_t workspace_bytes, uint8_t *keep,
                        void *stream) {
    HM_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "hm_nn_radius_finish: n must be in [1, 2^31)");
    HM_CHECK_ARG(records && workspace && keep, "hm_nn_radius_finish: NULL pointer");
    HM_CHECK_ARG(workspace_bytes >= nr_layout(nullptr, n).bytes, "hm_nn_radius_finish: workspace too small");
    const NrWs w = nr_layout(workspace, n);
    hipLaunchKernelGGL(nr_finish_kernel, dim3(hm_grid(n, kNT)), dim3(kNT), 0, as_stream(stream),
                       reinterpret_cast<const float4 *>(records), n, static_cast<const uint8_t *>(w.state), keep);
    HM_CHECK_LAUNCH("hm_nn_radius_finish");
    return HM_OK;
}

}  // extern "C"
