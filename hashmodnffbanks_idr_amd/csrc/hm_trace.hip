// hm_trace.hip - sync-free ray/surface intersection search for gfx950: IDR's bidirectional
// sphere tracing, sign-change sampler + secant refinement and the closest-approach search,
// restated as PER-RAY STATE MACHINES driven by small update kernels around the fused SDF kernel.
//
// Replaces RayTracing.forward / sphere_tracing / ray_sampler / secant / minimal_sdf_points
// (reference: model/ray_tracing.py:26-298).  Every update in the reference is gated by a per-ray
// mask, so each ray can run its own state machine; the reference's
// host-side control flow (>= 9 device->host syncs, boolean-mask gathers with data-dependent
// shapes) disappears: each round is  [advance rays, append the points they need to a compact
// buffer with an atomic cursor]  ->  [fused SDF kernel over min(capacity, *cursor) points, the
// count read on the device].  One C call enqueues the whole search; nothing synchronises.
//
// Arithmetic is kept bit-compatible with the reference's elementwise fp32 expressions
// (p = cam + t*dir as mul-then-add, t +/- sdf, the secant formula's evaluation order); the file
// is compiled with -ffp-contract=off.
#include "hm_common.h"
#include "hm_trace_host.h"   // the fused launches of hm_sdf.hip

#include <stdlib.h>
#include <string.h>

namespace {

constexpr int kTB = 256;

#include "hm_trace_dev.h"

// round 0: both sphere intersections of every ray that hits the bounding sphere (ray_tracing.py:101-128)
__global__ __launch_bounds__(kTB) void trace_init_kernel(TraceArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= a.n) return;
    trace_init_ray(a, i, a.w.cnt + C_ROUND0, 0);
}

// one round of the per-ray sphere-tracing state machine (ray_tracing.py:130-186): the points it appends are evaluated
// by the next round's SDF launch
__global__ __launch_bounds__(kTB) void trace_advance_kernel(TraceArgs a, int round) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= a.n) return;
    trace_advance_ray(a, i, a.w.cnt + C_ROUND0 + round, 0);
}

// after the march: network mask, provisional outputs, hand unconverged rays to the sampler
__global__ __launch_bounds__(kTB) void trace_finalize_kernel(TraceArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= a.n) return;
    const TraceWs &w = a.w;
    if (w.stage[i] != ST_DONE) atomicAdd(w.cnt + C_UNFINISHED, 1);
    const float t_s = w.t_s[i], t_e = w.t_e[i];
    a.out_mask[i] = t_s < t_e;
    a.out_t[i] = t_s;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    // the reference recomputes cam + t*dir for ALL rays once its loop has run at least one iteration
    if (a.hit[i] || w.cnt[C_ANY_LIVE]) along(a, i, t_s, px, py, pz);
    a.out_pts[i * 3] = px; a.out_pts[i * 3 + 1] = py; a.out_pts[i * 3 + 2] = pz;
    const bool samp = w.live_s[i] != 0;
    w.is_samp[i] = samp;
    if (samp) w.list_samp[atomicAdd(w.cnt + C_NSAMP, 1)] = (int32_t)i;
}

// n_steps samples along every listed ray: t = lo + f*(hi - lo)  (ray_tracing.py:198-206, 277-286)
// c_base >= 0: the points are appended behind the cnt[c_base] points already in the buffer (one SDF launch then
// evaluates both sets); cnt[C_BIG_PTS] receives the total.
//
// Lazy sampler (a.head > 0): the reference reads, of a sampler ray's n_steps values, only those up to its FIRST negative
// sample (argmin of sign * (n, n-1, ..), ray_tracing.py:212-218, plus the sample before it - or the last one when the
// first sample is negative - for the secant bracket, :238-243) unless the ray falls back to the minimal sample
// (:221-226), which needs all of them.  per_ray < n_steps selects the first pass: samples 0..head-1 and n_steps-1.
__global__ __launch_bounds__(kTB) void ray_samples_kernel(TraceArgs a, const int32_t *list, int c_n, int c_npts,
                                                          const float *lo_arr, const float *hi_arr,
                                                          const float *fr, int c_base, int per_ray) {
    const int64_t gid = (int64_t)blockIdx.x * kTB + threadIdx.x;
    const TraceWs &w = a.w;
    const int32_t n_list = w.cnt[c_n];
    const int64_t base = c_base == -2 ? a.sel_off : (c_base >= 0 ? w.cnt[c_base] : 0);   // (-2: the region of its own)
    if (gid == 0) {
        w.cnt[c_npts] = n_list * per_ray;
        if (c_base != -2) w.cnt[C_BIG_PTS] = (int32_t)base + n_list * per_ray;
    }
    const int64_t m = gid / per_ray;
    if (m >= n_list) return;
    int s = (int)(gid - m * per_ray);
    if (per_ray < a.n_steps && s == per_ray - 1) s = a.n_steps - 1;
    const int64_t i = list[m];
    const float lo = lo_arr[i], hi = hi_arr[i];
    const float t = __fadd_rn(lo, __fmul_rn(fr[s], __fsub_rn(hi, lo)));
    float px, py, pz;
    along(a, i, t, px, py, pz);
    const int64_t o = base + gid;
    w.pts[o * 3] = px; w.pts[o * 3 + 1] = py; w.pts[o * 3 + 2] = pz;
}

// lazy sampler, between the passes: a ray is resolved by its head samples iff one of them is negative and the ray is
// inside the object mask; every other ray joins the second pass (samples head..n_steps-2)
__global__ __launch_bounds__(kTB) void sampler_head_kernel(TraceArgs a) {
    const int64_t m = (int64_t)blockIdx.x * kTB + threadIdx.x;
    const TraceWs &w = a.w;
    if (m >= w.cnt[C_NSAMP]) return;
    const int64_t i = w.list_samp[m];
    const float *v = w.vals + m * (a.head + 1);
    bool neg = false;
    for (int s = 0; s < a.head; ++s) neg = neg || (v[s] < 0.0f);
    const bool resolved = neg && a.obj[i] != 0;
    w.tail_slot[m] = resolved ? -1 : atomicAdd(w.cnt + C_NSAMP2, 1);
}

__global__ __launch_bounds__(kTB) void sampler_tail_points_kernel(TraceArgs a) {
    const int64_t gid = (int64_t)blockIdx.x * kTB + threadIdx.x;
    const TraceWs &w = a.w;
    const int per = a.n_steps - a.head - 1;
    if (gid == 0) {
        w.cnt[C_TAIL_PTS] = w.cnt[C_NSAMP2] * per;
        w.cnt[C_NSAMP_PTS] = w.cnt[C_HEAD_PTS] + w.cnt[C_NSAMP2] * per;     // statistics: sampler evaluations
    }
    const int64_t m = gid / per;
    if (m >= w.cnt[C_NSAMP]) return;
    const int32_t q = w.tail_slot[m];
    if (q < 0) return;
    const int j = (int)(gid - m * per);
    const int64_t i = w.list_samp[m];
    const float lo = w.t_s[i], hi = w.t_e[i];
    const float t = __fadd_rn(lo, __fmul_rn(a.fracs[a.head + j], __fsub_rn(hi, lo)));
    float px, py, pz;
    along(a, i, t, px, py, pz);
    const int64_t o = a.tail_off + (int64_t)q * per + j;
    w.pts[o * 3] = px; w.pts[o * 3 + 1] = py; w.pts[o * 3 + 2] = pz;
}

// first sign change / minimal sample per sampler ray, secant bracket set-up (ray_tracing.py:212-247)
__global__ __launch_bounds__(kTB) void sampler_reduce_kernel(TraceArgs a) {
    const int64_t m = (int64_t)blockIdx.x * kTB + threadIdx.x;
    const TraceWs &w = a.w;
    if (m >= w.cnt[C_NSAMP]) return;
    const int64_t i = w.list_samp[m];
    const int n = a.n_steps;
    // value of sample s: one [n_steps] row (single pass) or head row + second-pass row (lazy sampler)
    const bool lazy = a.head > 0;
    const int32_t tq = lazy ? w.tail_slot[m] : 0;    // second-pass slot, -1 = resolved by the head samples
    const float *v_head = lazy ? w.vals + m * (a.head + 1) : w.vals + m * n;
    const float *v_tail = lazy ? w.vals + a.tail_off + (int64_t)(tq < 0 ? 0 : tq) * (n - a.head - 1) - a.head : v_head;
    const int head = a.head;
    auto v = [&](int s) -> float {
        if (!lazy) return v_head[s];
        if (s < head) return v_head[s];
        return s == n - 1 ? v_head[head] : v_tail[s];
    };
    // a ray resolved by its head samples has its first negative sample there: later samples cannot change `first`
    // (their sign * rank is larger) and nothing else is read from them
    const int n_scan = (lazy && tq < 0) ? head : n;
    int first = 0, amin = 0, bad = 0;
    float best_tmp = 0.0f, best_v = 0.0f;
    auto visit = [&](int s, float x) {
        bad += !isfinite(x);
        const float sg = (x > 0.0f) ? 1.0f : ((x < 0.0f) ? -1.0f : 0.0f);
        const float tmp = sg * (float)(n - s);  // sign(sdf) * arange(n, 0, -1)
        if (s == 0 || tmp < best_tmp) { best_tmp = tmp; first = s; }
        if (s == 0 || x < best_v) { best_v = x; amin = s; }
    };
    if (!lazy && (n & 3) == 0 && (reinterpret_cast<uintptr_t>(v_head) & 15u) == 0) {
        // single-pass rows are n contiguous floats: 16-byte loads, several in flight - the scalar loop below waits for
        // one 4-byte load per sample (a serial L2 round trip each: 42 us for 1281 rays of 100 samples)
        const float4 *row = reinterpret_cast<const float4 *>(v_head);
#pragma unroll 5
        for (int g4 = 0; g4 < n / 4; ++g4) {
            const float4 x4 = row[g4];
            visit(4 * g4, x4.x); visit(4 * g4 + 1, x4.y); visit(4 * g4 + 2, x4.z); visit(4 * g4 + 3, x4.w);
        }
    } else {
        for (int s = 0; s < n_scan; ++s) visit(s, v(s));
    }
    const float lo = w.t_s[i], hi = w.t_e[i];
    auto t_at = [&](int s) { return __fadd_rn(lo, __fmul_rn(a.fracs[s], __fsub_rn(hi, lo))); };
    const float v_first = v(first);
    const bool net_hit = v_first < 0.0f;
    const bool true_obj = a.obj[i] != 0;
    const int pick = (true_obj && net_hit) ? first : amin;
    float t_out = t_at(pick);
    float px, py, pz;
    along(a, i, t_out, px, py, pz);
    a.out_mask[i] = net_hit;
    const bool sec = a.training ? (net_hit && true_obj) : net_hit;
    if (sec) {
        const int lo_idx = first > 0 ? first - 1 : n - 1;  // index -1 wraps to the last sample, as in the reference
        const float z_hi = t_at(first), v_hi = v_first, z_lo = t_at(lo_idx), v_lo = v(lo_idx);
        if (lazy && tq < 0 && lo_idx == n - 1 && !isfinite(v_lo)) ++bad;   // (outside the scanned range)
        const float z = secant_z(v_lo, v_hi, z_lo, z_hi);
        const int32_t q = atomicAdd(w.cnt + C_NSEC, 1);
        w.list_sec[q] = (int32_t)i;
        w.z_lo[q] = z_lo; w.z_hi[q] = z_hi; w.v_lo[q] = v_lo; w.v_hi[q] = v_hi; w.z[q] = z;
        if (a.n_secant == 0) {  // no refinement rounds: the initial secant estimate is the answer
            t_out = z;
            along(a, i, z, px, py, pz);
        }
    }
    if (bad) atomicAdd(w.cnt + C_NONFINITE, bad);
    a.out_t[i] = t_out;
    w.t_s[i] = t_out;
    a.out_pts[i * 3] = px; a.out_pts[i * 3 + 1] = py; a.out_pts[i * 3 + 2] = pz;
}

// p_mid = cam + z*dir for every secant ray (the points of the next SDF launch)
__global__ __launch_bounds__(kTB) void secant_points_kernel(TraceArgs a) {
    const int64_t q = (int64_t)blockIdx.x * kTB + threadIdx.x;
    const TraceWs &w = a.w;
    if (q >= w.cnt[C_NSEC]) return;
    float px, py, pz;
    along(a, w.list_sec[q], w.z[q], px, py, pz);
    w.pts[q * 3] = px; w.pts[q * 3 + 1] = py; w.pts[q * 3 + 2] = pz;
}

// one secant iteration (ray_tracing.py:255-266), stand-alone form of secant_advance_ray
__global__ __launch_bounds__(kTB) void secant_advance_kernel(TraceArgs a, int last) {
    const int64_t q = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (q >= a.w.cnt[C_NSEC]) return;
    secant_advance_ray(a, q, last);
}

// training tail, part 1 (ray_tracing.py:71-88): rays that feed the mask loss
__global__ __launch_bounds__(kTB) void tail_prepare_kernel(TraceArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= a.n) return;
    const TraceWs &w = a.w;
    const bool net = a.out_mask[i] != 0, obj = a.obj[i] != 0, samp = w.is_samp[i] != 0, hit = a.hit[i] != 0;
    const bool in_mask = !net && obj && !samp;
    const bool out_mask = !obj && !samp;
    if (!(in_mask || out_mask)) return;
    if (!hit) {
        // the ray never enters the sphere: closest point of the ray to the origin, t = -<dir, cam>
        const float *c = a.cam + (i / a.rays_per_image) * 3;
        const float *d = a.dirs + i * 3;
        const float dot = __fmaf_rn(d[2], c[2], __fmaf_rn(d[1], c[1], __fmul_rn(d[0], c[0])));
        const float t = -dot;
        float px, py, pz;
        along(a, i, t, px, py, pz);
        a.out_t[i] = t;
        w.t_s[i] = t;
        a.out_pts[i * 3] = px; a.out_pts[i * 3 + 1] = py; a.out_pts[i * 3 + 2] = pz;
        return;
    }
    if (net && out_mask) w.t_min[i] = w.t_s[i];
    w.list_sel[atomicAdd(w.cnt + C_NSEL, 1)] = (int32_t)i;
}

// training tail, part 2 (ray_tracing.py:288-296): argmin of the SDF over the shared random fractions
__global__ __launch_bounds__(kTB) void closest_reduce_kernel(TraceArgs a) {
    const int64_t m = (int64_t)blockIdx.x * kTB + threadIdx.x;
    const TraceWs &w = a.w;
    if (m >= w.cnt[C_NSEL]) return;
    const int64_t i = w.list_sel[m];
    const int n = a.n_steps;
    const float *v = w.vals + (a.sel_off >= 0 ? a.sel_off : (int64_t)w.cnt[a.head > 0 ? C_HEAD_PTS : C_NSAMP_PTS]) +
                     m * n;   // a region of their own, or behind the sampler's first pass
    int amin = 0, bad = !isfinite(v[0]);
    float best = v[0];
    if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(v) & 15u) == 0) {   // (16-byte loads: see sampler_reduce_kernel)
        const float4 *row = reinterpret_cast<const float4 *>(v);
        auto visit = [&](int s, float x) {
            if (s == 0) return;
            bad += !isfinite(x);
            if (x < best) { best = x; amin = s; }
        };
#pragma unroll 5
        for (int g4 = 0; g4 < n / 4; ++g4) {
            const float4 x4 = row[g4];
            visit(4 * g4, x4.x); visit(4 * g4 + 1, x4.y); visit(4 * g4 + 2, x4.z); visit(4 * g4 + 3, x4.w);
        }
    } else {
        for (int s = 1; s < n; ++s) {
            bad += !isfinite(v[s]);
            if (v[s] < best) { best = v[s]; amin = s; }
        }
    }
    if (bad) atomicAdd(w.cnt + C_NONFINITE, bad);
    const float lo = w.t_min[i], hi = w.t_max[i];
    const float t = __fadd_rn(__fmul_rn(a.steps_u[amin], __fsub_rn(hi, lo)), lo);
    float px, py, pz;
    along(a, i, t, px, py, pz);
    a.out_t[i] = t;
    a.out_pts[i * 3] = px; a.out_pts[i * 3 + 1] = py; a.out_pts[i * 3 + 2] = pz;
}

// ---- guarded coarse scans (hm_trace_cfg.coarse_bf16 = 3) ------------------------------------------------------------
// A floating-point filter, as in exact geometric predicates: the coarse rows are evaluated on the f16x2 split kernel,
// the samples whose approximate value cannot settle what the reduce kernels read are re-evaluated by the exact-fp32
// kernel (compact refinement region, one launch), the exact values are written over the approximate ones, and the
// reduce kernels run unchanged on the patched rows.
//
// Marking rule.  tau = kGuardTau, a_s = approximate value of sample s.  s is UNCERTAIN if a_s is non-finite or
// |a_s| <= tau; c = first sample with a_s < -tau (if any).  Sampler rows:
//   1. every uncertain sample is marked;
//   2. c is marked, and its predecessor (index 0 wraps to the row's last sample, as lo_idx does);
//   3. the predecessor of every uncertain u before c (of every uncertain u when there is no c) is marked: u may turn out
//      to be `first`, and its bracket partner must then be exact;
//   4. when the arg-min can be read (the ray is outside the object mask, or it has no c): every sample with
//      a_s <= m + 2 tau, m = smallest finite a_s of the row.
// Closest-approach rows: non-finite samples and rule 4.
// The lazy sampler's first pass applies 1-3 to its own row (samples 0..head-1, then n_steps-1: the wrap of rule 2 is
// the row's own); a ray it resolves reads nothing else.  Every other ray is in the second pass, which applies 1-4 to the
// ray's whole row (first-pass samples already patched are exact; marking one again changes nothing).
//
// Why the outputs are those of the all-fp32 scan, given |a_s - exact_s| <= tau:
//   * an unmarked sample has |a_s| > tau, so its sign is the exact one; marked samples are exact.  Hence `first` - and
//     the first pass's "a head sample is negative" - is the fp32 scan's, and v_first, v_lo (rules 2, 3) are exact values;
//   * arg-min over the patched row: an unmarked sample has a_s > m + 2 tau, so its exact value is > m + tau, while the
//     sample that attains m is marked and its exact value is <= m + tau: an unmarked sample never wins.  Every exact
//     minimiser has a_s <= m + 2 tau, so it is marked and carries its exact value; ties resolve by first index as before;
//   * the non-finite counter is unchanged under the ASSUMPTION that a sample whose fp32 value is non-finite is non-finite
//     in f16x2 too (fp16 overflows first): such a sample is marked and patched with its fp32 value.
// |a - exact| <= tau is monitored, not assumed: guard_patch_kernel sees both values of every refined sample; a deviation
// above kGuardTrip = tau / 4 sets the workspace's sticky word, and from then on (the following launches of that call
// included) every sample is marked, i.e. the scans are all-fp32.  The tripping call itself is still exact (tau/4 < tau).
// Where the refinements are co-scheduled (GUARD_COSCHED, GUARD_POOLED) the closest-approach rows are selected BEHIND the
// sampler's patch, on a list and a counter of their own (C_GUARD_NC): a call in which the sampler's patch trips the monitor
// marks every closest-approach sample in that same call already - conservative and still exact; that call's refined count
// is then larger than with HM_TRACE_OVERLAP=1, where both selections run in front of the one patch.
//
// A launch of fewer than min_live points ran on the exact kernel already (the small-tile launch of coarse()): nothing is
// marked for it.  val(s) / slot(s): value and index in vals of the row's sample s; own(s): s was evaluated by this launch,
// own_approx / other_approx: this launch / the row's other launch was an approximate one.
// One wave per row: lanes take samples lane, lane + 64, ... (coalesced), c and m come from wave reductions, every lane
// applies the marking rule to its own samples, and the row's entries go behind ONE atomicAdd in ascending sample order
// (ballot / prefix rank) - the set of marked slots of a row and their order are those of a serial walk over the row.
constexpr int kGuardRows = kTB / 64;     // rows per workgroup
template <class V, class S, class O>
__device__ __forceinline__ void guard_mark_row(const TraceArgs &a, int lane, int n, bool signs, bool min_rule,
                                               bool true_obj, bool all, bool own_approx, bool other_approx, int c_ref,
                                               V val, S slot, O own) {
    const float tau = kGuardTau;
    const int kNone = 1 << 30;
    auto unc = [&](float x) { return !isfinite(x) || fabsf(x) <= tau; };
    int c = kNone;
    float m = INFINITY;
    for (int s = lane; s < n; s += 64) {
        const float x = val(s);
        if (signs && c == kNone && x < -tau) c = s;
        if (isfinite(x) && x < m) m = x;
    }
    for (int d = 32; d > 0; d >>= 1) {
        c = min(c, __shfl_xor(c, d));
        m = fminf(m, __shfl_xor(m, d));
    }
    const bool use_min = min_rule && (!signs || !true_obj || c == kNone);
    const float lim = m + 2.0f * tau;
    // x = a_s, xn = a_next with next = s + 1 (0 behind the last sample)
    auto marked = [&](int s, float x, float xn) -> bool {
        if (!(own(s) ? own_approx : other_approx)) return false;     // an exact launch's value: nothing to refine
        if (all && own(s)) return true;
        if (!isfinite(x)) return true;
        if (use_min && x <= lim) return true;
        if (!signs) return false;
        if (fabsf(x) <= tau || s == c) return true;
        const int nx = s + 1 == n ? 0 : s + 1;
        return nx <= c && (nx == c || unc(xn));
    };
    auto mark_of = [&](int s) -> bool { return s < n && marked(s, val(s), val(s + 1 == n ? 0 : s + 1)); };
    int n_mark = 0;
    for (int s0 = 0; s0 < n; s0 += 64) n_mark += __popcll(__ballot(mark_of(s0 + lane)));
    if (n_mark == 0) return;
    int k0 = 0;
    if (lane == 0) k0 = atomicAdd(a.w.cnt + c_ref, n_mark);
    int64_t k = __shfl(k0, 0);
    for (int s0 = 0; s0 < n; s0 += 64) {
        const int s = s0 + lane;
        const bool mk = mark_of(s);
        const unsigned long long b = __ballot(mk);
        if (mk) {
            const int64_t kk = k + __popcll(b & ((1ull << lane) - 1ull));
            const int64_t o = slot(s);
            a.w.ref_slot[kk] = (int32_t)o;
            a.w.ref_pts[kk * 3] = a.w.pts[o * 3]; a.w.ref_pts[kk * 3 + 1] = a.w.pts[o * 3 + 1];
            a.w.ref_pts[kk * 3 + 2] = a.w.pts[o * 3 + 2];
        }
        k += __popcll(b);
    }
}

// pass 1: the sampler's first (or only) pass; pass 2: the lazy sampler's second pass.  c_live, c_live2: counters of the
// launches that evaluated the row's samples (pass 2 reads first-pass samples too: rule 4 is left to it; -1: none).
__global__ __launch_bounds__(kTB) void guard_select_sampler_kernel(TraceArgs a, int pass, int c_live, int c_live2,
                                                                   int64_t min_live, int c_ref) {
    const int64_t m = (int64_t)blockIdx.x * kGuardRows + (threadIdx.x >> 6);     // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const TraceWs &w = a.w;
    if (m >= w.cnt[C_NSAMP]) return;
    const bool approx = w.cnt[c_live] >= min_live, approx2 = c_live2 >= 0 && w.cnt[c_live2] >= min_live;
    if (!approx && !approx2) return;
    const bool all = *w.guard == kGuardTripped;
    const bool true_obj = a.obj[w.list_samp[m]] != 0;
    const int n = a.n_steps, head = a.head;
    if (pass == 1) {
        const int row = head > 0 ? head + 1 : n;
        const int64_t base = m * row;
        guard_mark_row(a, lane, row, true, head == 0, true_obj, all, true, false, c_ref,
                       [&](int s) { return w.vals[base + s]; }, [&](int s) { return base + s; }, [](int) { return true; });
        return;
    }
    const int32_t tq = w.tail_slot[m];
    if (tq < 0) return;     // resolved by the head samples
    const int64_t b_head = m * (head + 1), b_tail = a.tail_off + (int64_t)tq * (n - head - 1) - head;
    auto slot = [&](int s) -> int64_t { return s < head ? b_head + s : (s == n - 1 ? b_head + head : b_tail + s); };
    guard_mark_row(a, lane, n, true, true, true_obj, all, approx, approx2, c_ref, [&](int s) { return w.vals[slot(s)]; },
                   slot, [&](int s) { return s >= head && s != n - 1; });
}

__global__ __launch_bounds__(kTB) void guard_select_closest_kernel(TraceArgs a, int c_live, int64_t min_live, int c_ref) {
    const int64_t m = (int64_t)blockIdx.x * kGuardRows + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const TraceWs &w = a.w;
    if (m >= w.cnt[C_NSEL] || w.cnt[c_live] < min_live) return;
    const int n = a.n_steps;
    const int64_t base = (a.sel_off >= 0 ? a.sel_off : (int64_t)w.cnt[a.head > 0 ? C_HEAD_PTS : C_NSAMP_PTS]) + m * n;
    guard_mark_row(a, lane, n, false, true, false, *w.guard == kGuardTripped, true, false, c_ref,
                   [&](int s) { return w.vals[base + s]; },
                   [&](int s) { return base + s; }, [](int) { return true; });
}

// exact values over the approximate ones; the monitor (statistics slots 14, 15 and the sticky word)
__global__ __launch_bounds__(kTB) void guard_patch_kernel(TraceArgs a, int c_ref) {
    const int64_t k = (int64_t)blockIdx.x * kTB + threadIdx.x;
    const TraceWs &w = a.w;
    const int32_t n_ref = w.cnt[c_ref];
    if (k == 0 && n_ref > 0) atomicAdd(w.cnt + C_GUARD_REFINED, n_ref);
    if (k >= n_ref) return;
    const int64_t o = w.ref_slot[k];
    const float e = w.ref_vals[k], ap = w.vals[o];
    if (isfinite(e) && isfinite(ap)) {
        const float d = fabsf(ap - e);
        if (d > 0.0f) atomicMax(w.cnt + C_GUARD_MAXDEV, __float_as_int(d));   // (non-negative floats order as their bits)
        if (d > kGuardTrip) *w.guard = kGuardTripped;
    }
    w.vals[o] = e;
}

// HM_TRACE_GUARD_NOISE (tests): worst-case errors of the approximate values of one launch.  nan_k > 0: every nan_k-th
// slot becomes NaN or +Inf in turn; otherwise a pseudo-random offset in [-amp, amp], a function of the slot index.
__global__ __launch_bounds__(kTB) void guard_noise_kernel(float *vals, int64_t off, const int32_t *n_live, int64_t min_live,
                                                          float amp, int nan_k) {
    const int64_t g = (int64_t)blockIdx.x * kTB + threadIdx.x;
    const int64_t n = *n_live;
    if (n < min_live || g >= n) return;
    const int64_t o = off + g;
    if (nan_k > 0) {
        if (o % nan_k == 0) vals[o] = ((o / nan_k) & 1) ? INFINITY : NAN;
        return;
    }
    uint32_t h = (uint32_t)o * 2654435761u;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    const float u = (float)(h >> 8) * (2.0f / 16777216.0f) - 1.0f;     // [-1, 1)
    vals[o] = __fadd_rn(vals[o], __fmul_rn(amp, u));
}

__global__ void count_evals_kernel(int32_t *cnt, int rounds, int n_secant) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t tot = 0;
    for (int r = 0; r < rounds && r < 64; ++r) tot += cnt[C_ROUND0 + r];
    tot += cnt[C_NSAMP_PTS] + (int64_t)cnt[C_NSEC] * n_secant + cnt[C_NSEL_PTS];
    cnt[C_EVALS] = (int32_t)tot;
}

// ---- workspace ------------------------------------------------------------------------------------------------------------
// One description of the per-ray arrays: the workspace's size and the kernels' pointers both follow from these lists, so
// a new array is added here and nowhere else.  Each list is one block of n elements per member.
constexpr float *TraceWs::*kRayFloats[] = {&TraceWs::t_s,   &TraceWs::t_e,   &TraceWs::t_min, &TraceWs::t_max, &TraceWs::cur_s,
                                           &TraceWs::cur_e, &TraceWs::nxt_s, &TraceWs::nxt_e, &TraceWs::z_lo,  &TraceWs::z_hi,
                                           &TraceWs::v_lo,  &TraceWs::v_hi,  &TraceWs::z};
constexpr int32_t *TraceWs::*kRayInts[] = {&TraceWs::slot_s,   &TraceWs::slot_e,   &TraceWs::list_samp,
                                           &TraceWs::list_sec, &TraceWs::list_sel, &TraceWs::tail_slot};
constexpr uint8_t *TraceWs::*kRayBytes[] = {&TraceWs::live_s, &TraceWs::live_e, &TraceWs::stage,
                                            &TraceWs::it,     &TraceWs::k,      &TraceWs::is_samp};
template <class T, size_t K>
void carve_rays(HmCarve &c, TraceWs &w, T *TraceWs::*const (&members)[K], int64_t n) {
    T *p = c.take<T>((int64_t)K * n);
    for (size_t k = 0; k < K; ++k) w.*members[k] = p + (p ? (int64_t)k * n : 0);
}

constexpr int64_t kWsHeader = 256;   // the guard's sticky word: at the same place for every ray count
constexpr int kWsRegions = 3;   // regions of `cap` points in pts / vals: first pass (+ other launches), second pass, closest approach

// [header | per-ray floats | ints | bytes | pts | vals | counters | embedding rows | refinement region]; ws == nullptr: the
// size only
struct TraceLayout { TraceWs w; float *emb_ws; int64_t bytes; };
TraceLayout trace_layout(void *ws, int64_t n, int n_steps, int emb_width, bool guard) {
    TraceLayout L;
    TraceWs &w = L.w;
    HmCarve c(ws);
    w.cap = n * (n_steps > 2 ? n_steps : 2);    // points of one SDF launch
    w.guard = c.take<int32_t>(kWsHeader / (int64_t)sizeof(int32_t));
    carve_rays(c, w, kRayFloats, n);
    carve_rays(c, w, kRayInts, n);
    carve_rays(c, w, kRayBytes, n);
    w.pts = c.take<float>(kWsRegions * 3 * w.cap);
    w.vals = c.take<float>(kWsRegions * w.cap);
    w.cnt = c.take<int32_t>(C_COUNT);
    L.emb_ws = c.take<float>((int64_t)emb_width * w.cap);   // (filter-bank embedders)
    // guarded coarse scans: refinement region for every coarse point of a launch (a tripped guard refines them all):
    // points [cap,3], exact values [cap], slots [cap]
    w.ref_pts = c.take<float>(guard ? 5 * w.cap : 0);
    w.ref_vals = w.ref_pts + (ws ? 3 * w.cap : 0);
    w.ref_slot = reinterpret_cast<int32_t *>(w.ref_vals + (ws ? w.cap : 0));
    L.bytes = c.bytes;
    return L;
}
int nffb_emb_width(int n_levels) { return 3 + 8 + 8 * n_levels; }

// ---- the plan: which launches a call enqueues -------------------------------------------------------------------------------
// Environment switches, read once per call (the tests flip them within one process):
//   HM_TRACE_OVERLAP            A/B, tests.  unset: the default sequences.  0: the closest-approach scan joins the sampler's
//                               launch and the secant runs behind it on a few dozen workgroups (no FILL, no co-scheduling).
//                               1: the default, except that the guarded scans run every launch on its own, with one list
//                               (GUARD_SERIAL).  2: guarded, the whole scan in front of the secant chain (GUARD_COSCHED).
//   HM_TRACE_POOL_CHAIN_TILES   A/B, tests.  k >= 0: the chain hides k split tiles per workgroup instead of
//                               trace_chain_tiles' - 0 leaves the whole scan in front of it.
//   HM_TRACE_CHAIN_TAIL         A/B, tests.  r >= 0: r secant rounds behind the cut of the chain instead of kTraceChainTail,
//                               0 = the chain is not cut.
//   HM_TRACE_TAIL_FIRST         tests.  k >= 1: the march hands over to the persistent kernel after k rounds already.
//   HM_TRACE_GUARD_NOISE        tests.  f (0 < f < 1): worst-case errors of up to f * tau on the approximate values;
//                               nan:K: every K-th of them NaN or +Inf (guard_noise_kernel).
struct TraceSwitches {
    int overlap, chain_tiles, chain_tail;   // -1: unset
    int tail_first;                         // 0: unset
    float noise_amp; int noise_nan;  // 0: none
};
TraceSwitches trace_switches() {
    const auto num = [](const char *name, int unset) {
        const char *e = getenv(name);
        return e ? atoi(e) : unset;
    };
    TraceSwitches s = {num("HM_TRACE_OVERLAP", -1), num("HM_TRACE_POOL_CHAIN_TILES", -1), num("HM_TRACE_CHAIN_TAIL", -1),
                       num("HM_TRACE_TAIL_FIRST", 0), 0.0f, 0};
    const char *e = getenv("HM_TRACE_GUARD_NOISE");
    if (e && strncmp(e, "nan:", 4) == 0) s.noise_nan = atoi(e + 4) > 0 ? atoi(e + 4) : 0;
    else if (e) { const double f_ = atof(e); if (f_ > 0.0 && f_ < 1.0) s.noise_amp = (float)(f_ * kGuardTau); }
    return s;
}

using TracePlan = hm_trace_plan_info;

// Every decision of a call, from its shape alone: no pointer, no stream.
TracePlan trace_plan(const hm_trace_cfg &cfg, int64_t n_rays, int tile_points, bool has_nffb, const TraceSwitches &sw) {
    TracePlan P = {};
    const bool guard = cfg.coarse_bf16 == 3;
    const int n_sec = cfg.n_secant_steps;
    // Closest-approach scan and secant refinement in one launch: training, hash-grid network, tile size left to the
    // library, a batch of small-tile secant launches
    const bool overlap_shape = sw.overlap != 0 && cfg.training && !has_nffb && tile_points == 0 && n_sec > 0 && n_rays <= kSdfSmall;
    const bool fill = overlap_shape && cfg.coarse_bf16 == 0;
    const bool cosched = guard && overlap_shape && sw.overlap != 1;
    const bool pooled = cosched && sw.overlap != 2;
    P.sequence = fill ? HM_TRACE_SEQ_FILL : pooled ? HM_TRACE_SEQ_GUARD_POOLED : cosched ? HM_TRACE_SEQ_GUARD_COSCHED
                 : guard ? HM_TRACE_SEQ_GUARD_SERIAL : HM_TRACE_SEQ_JOINT;
    // Guarded scans take the values of the exact scan they stand for, and which fp32 tile body that scan runs on follows
    // the live count of ITS launch: where the exact mode scans the closest-approach rows in a launch of their own, the
    // guarded mode evaluates them by their own count too (and the secant picks its tiles by the rule of that launch).
    P.sel_own = fill || (guard && overlap_shape);
    // lazy sampler: a first pass over samples 0..head-1 and n_steps-1 only pays when it leaves something out
    P.head = (cfg.sampler_head >= 1 && cfg.sampler_head + 1 < cfg.n_steps) ? cfg.sampler_head : 0;
    P.per_ray = P.head > 0 ? P.head + 1 : cfg.n_steps;
    // (single pass: the first pass IS the sampler's evaluation count; lazy: the second pass adds to it later)
    P.c_first = P.head > 0 ? (int)C_HEAD_PTS : (int)C_NSAMP_PTS;
    // Chains of at most the wanted tail run whole in front of the closest-approach rows' refinement.
    // (The scan's ranges do not follow the cut: the first launch keeps the tiles the whole chain would hide and runs the
    //  ones its shorter chain does not cover as a last round of all its workgroups, ~165 us.  Counting only the rounds in
    //  front of the cut sends them to the refine-scan launch instead, whose fp32 workgroups reach the scan late: +290 us
    //  there on the bench step, profiles/chain_tail_ab.json.)
    const int tail_want = sw.chain_tail >= 0 ? sw.chain_tail : kTraceChainTail;
    P.k_tail = (pooled && tail_want > 0 && n_sec > tail_want) ? tail_want : 0;
    P.chain_tiles = pooled ? trace_chain_tiles(n_sec, sw.chain_tiles >= 0 ? sw.chain_tiles : -1) : 0;
    P.c_ref2 = (pooled && P.head > 0) ? (int)C_GUARD_N2 : -1;
    // the guard's exact launch runs the tile body the exact mode's launch of the same live count runs: the 64-point one
    // with the tile size left to the library (smaller launches were exact already and mark nothing), the caller's otherwise
    P.guard_min = tile_points == 0 ? kSdfSmall + 1 : 1;
    if (guard) { P.noise_amp = sw.noise_amp; P.noise_nan = sw.noise_nan; }
    // The march needs 1 + sphere_tracing_iters rounds when no ray runs a line search, march_rounds when one does in every
    // iteration.  Hash-grid networks with the tile size left to the library (or fixed at 16) run the surplus rounds as
    // ONE persistent launch in which every workgroup carries eight rays to the end (hm_sdf.hip: trace_march_tail_kernel;
    // it returns at once when no ray is left) instead of 30 (empty SDF launch, empty update launch) pairs.
    const int64_t cap = n_rays * (cfg.n_steps > 2 ? cfg.n_steps : 2);
    P.march_rounds = 1 + cfg.sphere_tracing_iters * (1 + cfg.line_step_iters);
    P.march_tail = !has_nffb && (tile_points == 0 || tile_points == 16) && cap >= ((n_rays + 7) / 8) * 16 &&
                   cfg.line_step_iters > 0;
    P.march_launched = P.march_tail ? 1 + cfg.sphere_tracing_iters : P.march_rounds;
    if (P.march_tail && sw.tail_first >= 1 && sw.tail_first < P.march_launched) P.march_launched = sw.tail_first;
    // The secant refinement.  Hash-grid networks with small-tile SDF launches (tile size left to the library, or 4 / 8 / 16)
    // and a batch small enough for them: all iterations as ONE launch in which a tile of secant rays stays with its
    // workgroup (hm_sdf.hip: trace_secant_kernel; the sequences that scan beside the chain have it in their own launches);
    // otherwise an (SDF launch, update launch) pair per iteration
    if (n_sec == 0) P.secant = HM_TRACE_SECANT_NONE;
    else if (fill || cosched) P.secant = HM_TRACE_SECANT_IN_SEQUENCE;
    else if (!has_nffb && (tile_points == 0 || tile_points == 4 || tile_points == 8 || tile_points == 16) &&
             (tile_points != 0 || n_rays <= kSdfSmall))
        P.secant = HM_TRACE_SECANT_PERSISTENT;
    else P.secant = HM_TRACE_SECANT_PER_ITERATION;
    P.scan_rule = P.secant == HM_TRACE_SECANT_PERSISTENT && P.sel_own;
    return P;
}

// ---- the plan's executor: the steps the sequences are made of, then one function per sequence -----------------------------
struct TraceRun {
    HmTraceCtx cx; const hm_trace_cfg *cfg;
    TracePlan P; TraceArgs a;
    float *emb_ws;   // (filter-bank embedders: the embedding rows of a launch, emb_width floats each)
    int emb_width;

    // counters of the launches that evaluate the sampler's first pass / the closest-approach rows
    int c_samp() const { return P.sel_own ? P.c_first : (int)C_BIG_PTS; }
    int c_sel() const { return P.sel_own ? (int)C_NSEL_PTS : (int)C_BIG_PTS; }
    int64_t n_scan() const { return a.n * a.n_steps; }                     // capacity of a coarse launch: a whole pass
    int64_t n_tail() const { return a.n * (a.n_steps - a.head - 1); }      // ... the lazy sampler's second pass

    template <class K, class... A>
    void launch(K kernel, int64_t threads, A... args) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((threads + kTB - 1) / kTB)), dim3(kTB), 0, as_stream(cx.stream), args...);
    }
    template <class K, class... A> void per_ray(K kernel, A... args) { launch(kernel, a.n, a, args...); }
    // (guard select kernels: a wave per ray)
    template <class K, class... A> void per_row(K kernel, A... args) { launch(kernel, a.n * (kTB / kGuardRows), a, args...); }

    // One SDF evaluation of up to `capacity` points (*n_dev live) of the region of pts / vals that starts at point `off`.
    // mode 0: exact fp32, the caller's tile size (march, secant, exact coarse scans); hm_trace_cfg.coarse_bf16 1 / 2 / 3:
    // coarse scans on the 16-bit matrix cores above kSdfSmall live points, exact fp32 small tiles below.
    int eval(int64_t off, int64_t capacity, const int32_t *n_dev, int mode = 0) {
        const float *p = a.w.pts + off * 3;
        float *v = a.w.vals + off;
        const int64_t run_min = kSdfSmall + 1;   // (16-bit coarse kernels: the counts the small-tile launch leaves)
        const int tile = mode ? -1 : cx.tile_points;
        if (cx.nffb) {   // filter-bank embedder: its own fused kernel, then the MLP on the embedding rows
            HM_TRY(hm_nffb_fwd(cx.desc, cx.nffb, p, capacity, cx.table, cx.B_fourier, emb_ws, emb_width, cx.frac_mode, n_dev,
                               cx.stream));
            HM_TRY(hm_sdf_fwd_emb(cx.mlp, emb_ws, emb_width, emb_width, capacity, v, 1, 1, tile, n_dev, 0, cx.stream));
            if (!mode) return HM_OK;
            return mode == 2 ? hm_sdf_fwd_emb_split(cx.mlp, emb_ws, emb_width, emb_width, capacity, v, 1, n_dev, run_min, cx.stream)
                             : hm_sdf_fwd_emb_bf16(cx.mlp, emb_ws, emb_width, emb_width, capacity, v, 1, n_dev, run_min, cx.stream);
        }
        if (mode == 3 && cx.tile_points != 0)   // fixed tile size: every count is approximated (and refined on that tile)
            return hm_sdf_fwd_split(cx.desc, cx.mlp, p, capacity, cx.table, cx.B_fourier, v, 1, cx.frac_mode, n_dev, 1, cx.stream);
        HM_TRY(hm_sdf_fwd(cx.desc, cx.mlp, p, capacity, cx.table, cx.B_fourier, v, 1, 1, cx.frac_mode, tile, n_dev, 0, cx.stream));
        if (!mode) return HM_OK;
        return mode >= 2 ? hm_sdf_fwd_split(cx.desc, cx.mlp, p, capacity, cx.table, cx.B_fourier, v, 1, cx.frac_mode, n_dev, run_min,
                                            cx.stream)
                         : hm_sdf_fwd_bf16(cx.desc, cx.mlp, p, capacity, cx.table, cx.B_fourier, v, 1, cx.frac_mode, n_dev, run_min,
                                           cx.stream);
    }
    // the coarse scans (sampler passes, closest approach)
    int coarse(int64_t off, int64_t capacity, int c_live) { return eval(off, capacity, a.w.cnt + c_live, cfg->coarse_bf16); }

    // The points of the sampler's first pass and of the closest-approach rows.  The mask-loss rays (ray_tracing.py:71-92)
    // are exactly the rays the sampler does NOT touch, so their n_steps random-fraction samples do not depend on the
    // sampler's outcome: they are appended behind the sampler's points (one launch over both sets: one dependent launch
    // and one partial last wave less) or go to a region of their own (sel_own).
    void first_pass_points() {
        if (cfg->training) per_ray(tail_prepare_kernel);
        launch(ray_samples_kernel, a.n * P.per_ray, a, a.w.list_samp, (int)C_NSAMP, P.c_first, a.w.t_s, a.w.t_e, a.fracs, -1,
               P.per_ray);
        if (cfg->training)
            launch(ray_samples_kernel, n_scan(), a, a.w.list_sel, (int)C_NSEL, (int)C_NSEL_PTS, a.w.t_min, a.w.t_max, a.steps_u,
                   P.sel_own ? -2 : P.c_first, a.n_steps);
    }
    // lazy sampler: the remaining samples of the rays the head samples did not resolve
    void second_pass_points() {
        per_ray(sampler_head_kernel);
        launch(sampler_tail_points_kernel, n_scan(), a);
    }

    // The guard's steps.  Behind the approximate launch(es) of a coarse evaluation: [test noise] -> select -> one exact
    // launch over the compact refinement region -> patch.
    void noise(int64_t off, int64_t capacity, int c_live) {
        if (P.noise_amp > 0.0f || P.noise_nan > 0)
            launch(guard_noise_kernel, capacity, a.w.vals, off, a.w.cnt + c_live, P.guard_min, P.noise_amp, P.noise_nan);
    }
    void select_sampler(int pass, int c_live, int c_live2, int c_ref) {
        per_row(guard_select_sampler_kernel, pass, c_live, c_live2, P.guard_min, c_ref);
    }
    void select_closest(int c_live, int c_ref) { per_row(guard_select_closest_kernel, c_live, P.guard_min, c_ref); }
    // the stand-alone exact launch.  quarter: a list of at most 16 points per workgroup runs quarter tiles (the same values in
    // two thirds of the time of the half tiles; only where the launch stands alone - the closest-approach rows' list
    // behind the secant chain)
    int refine(int c_ref, bool quarter = false) {
        return hm_sdf_fwd(cx.desc, cx.mlp, a.w.ref_pts, a.w.cap, cx.table, cx.B_fourier, a.w.ref_vals, 1, 1, cx.frac_mode,
                          cx.tile_points == 0 ? (quarter ? HM_SDF_TILE64_QUARTER : 64) : cx.tile_points, a.w.cnt + c_ref, 0,
                          cx.stream);
    }
    // ... beside its range of the closest-approach rows' split tiles (which = 0 / 1: the launch of the first / second pass)
    int refine_beside_scan(int which) {
        return hm_trace_refine_scan(&cx, &a, C_GUARD_N1, P.c_ref2, which, a.sel_off, n_scan(), P.chain_tiles);
    }
    void patch(int c_ref) { launch(guard_patch_kernel, a.w.cap, a, c_ref); }
    // the lazy sampler's second pass; guarded: its marks see the first pass's (patched) samples too
    int second_pass() {
        if (a.head == 0) return HM_OK;
        second_pass_points();
        HM_TRY(coarse(a.tail_off, n_tail(), C_TAIL_PTS));
        if (cfg->coarse_bf16 != 3) return HM_OK;
        noise(a.tail_off, n_tail(), C_TAIL_PTS);
        select_sampler(2, C_TAIL_PTS, c_samp(), C_GUARD_N2);
        // (pooled: the tiles and values of the stand-alone launch, beside its range of the scan)
        HM_TRY(P.c_ref2 >= 0 ? refine_beside_scan(1) : refine(C_GUARD_N2));
        patch(C_GUARD_N2);
        return HM_OK;
    }
    // The sampler of the co-scheduled and the pooled sequence: the marks of the first pass are refined beside the
    // closest-approach rows' approximate scan (all of it, or the refine-scan launches' share of it).  The closest-approach
    // rows are then selected BEHIND the sampler's patch (see guard_mark_row), on a list of their own.
    int sampler_beside_scan() {
        HM_TRY(coarse(0, n_scan(), c_samp()));
        noise(0, n_scan(), c_samp());
        select_sampler(1, c_samp(), -1, C_GUARD_N1);
        HM_TRY(refine_beside_scan(0));
        patch(C_GUARD_N1);
        HM_TRY(second_pass());
        per_ray(sampler_reduce_kernel);
        per_ray(secant_points_kernel);
        return HM_OK;
    }
    // ... selected here, refined by `refine_launch`, patched and reduced
    template <class F>
    int closest_rows_own_list(F refine_launch) {
        noise(a.sel_off, n_scan(), C_NSEL_PTS);
        select_closest(C_NSEL_PTS, C_GUARD_NC);
        HM_TRY(refine_launch());
        patch(C_GUARD_NC);
        per_ray(closest_reduce_kernel);
        return HM_OK;
    }
    // the secant chain (or a part of it) with the closest-approach rows' refinement list as the launch's scan
    int secant_beside_list(int it_first, int n_iters, int quarter) {
        return hm_trace_scan_secant(&cx, &a, it_first, n_iters, a.n_secant, quarter, a.w.ref_pts, a.w.ref_vals, a.w.cap,
                                    C_GUARD_NC, 0, -1, 0, -1, 0);
    }
    // the sampler's reduction and the secant refinement of the sequences that do not scan beside it
    int reduce_and_secant() {
        per_ray(sampler_reduce_kernel);
        if (P.secant == HM_TRACE_SECANT_NONE) return HM_OK;
        per_ray(secant_points_kernel);
        if (P.secant == HM_TRACE_SECANT_PERSISTENT) return hm_trace_secant_persistent(&cx, &a, a.n_secant, P.scan_rule);
        for (int s = 0; s < a.n_secant; ++s) {
            HM_TRY(eval(0, a.n, a.w.cnt + C_NSEC));
            per_ray(secant_advance_kernel, s == a.n_secant - 1 ? 1 : 0);
        }
        return HM_OK;
    }

    // ---- 1. bidirectional sphere tracing: one state-machine round per SDF launch, the surplus rounds as one launch
    int march() {
        per_ray(trace_init_kernel);
        for (int r = 0; r < P.march_launched; ++r) {
            HM_TRY(eval(0, 2 * a.n, a.w.cnt + C_ROUND0 + r));
            // round r+1 cursor (the last advance appends nothing that is evaluated; it only closes states)
            per_ray(trace_advance_kernel, r + 1 < 64 ? r + 1 : 63);
        }
        if (P.march_tail) HM_TRY(hm_trace_march_tail(&cx, &a, P.march_launched, P.march_rounds));
        per_ray(trace_finalize_kernel);
        return HM_OK;
    }

    // ---- 2. sampler, closest approach (training) and secant refinement: the plan's sequence, behind first_pass_points()
    // JOINT: ONE coarse launch over the sampler's points and the closest-approach points behind them (every precision
    // but the guarded one; the exact mode where the shape or HM_TRACE_OVERLAP=0 rules FILL out).
    int seq_joint() {
        HM_TRY(coarse(0, n_scan(), C_BIG_PTS));
        if (cfg->training) per_ray(closest_reduce_kernel);
        HM_TRY(second_pass());
        return reduce_and_secant();
    }
    // FILL: closest-approach scan and secant refinement as one launch (hm_sdf.hip: sdf_scan_secant_kernel).  The sampler's
    // launches evaluate the sampler's points only - and complete their last round with tiles of the scan (fill_quota).
    int seq_fill() {
        int grid_p1 = 0, grid_p2 = 0;      // grids of the sampler launches that took filler tiles of the scan
        const float *x_fill = a.w.pts + a.sel_off * 3;
        float *out_fill = a.w.vals + a.sel_off;
        HM_TRY(hm_sdf_fwd_fill(&cx, a.w.pts, n_scan(), a.w.vals, a.w.cnt + P.c_first, x_fill, out_fill, a.w.cnt + C_NSEL_PTS,
                               nullptr, 0, &grid_p1));
        if (a.head > 0) {
            second_pass_points();
            HM_TRY(hm_sdf_fwd_fill(&cx, a.w.pts + a.tail_off * 3, n_tail(), a.w.vals + a.tail_off, a.w.cnt + C_TAIL_PTS, x_fill,
                                   out_fill, a.w.cnt + C_NSEL_PTS, a.w.cnt + P.c_first, grid_p1, &grid_p2));
        }
        per_ray(sampler_reduce_kernel);
        per_ray(secant_points_kernel);
        HM_TRY(hm_trace_scan_secant(&cx, &a, 0, a.n_secant, a.n_secant, 0, x_fill, out_fill, n_scan(), C_NSEL_PTS, 1, P.c_first,
                                    grid_p1, C_TAIL_PTS, grid_p2));
        per_ray(closest_reduce_kernel);
        return HM_OK;
    }
    // GUARD_SERIAL: every launch on its own, and ONE list for the first pass's marks and the closest-approach rows'
    // (both selections in front of the one patch).  The closest-approach rows are behind the sampler's points in one
    // launch, or - sel_own: HM_TRACE_OVERLAP=1, the A/B form of the two sequences below - in a launch by their own count.
    int seq_guard_serial() {
        HM_TRY(coarse(0, n_scan(), c_samp()));
        if (P.sel_own) HM_TRY(coarse(a.sel_off, n_scan(), c_sel()));
        noise(0, n_scan(), c_samp());
        if (P.sel_own) noise(a.sel_off, n_scan(), c_sel());
        select_sampler(1, c_samp(), -1, C_GUARD_N1);
        if (cfg->training) select_closest(c_sel(), C_GUARD_N1);
        HM_TRY(refine(C_GUARD_N1));
        patch(C_GUARD_N1);
        if (cfg->training) per_ray(closest_reduce_kernel);
        HM_TRY(second_pass());
        return reduce_and_secant();
    }
    // GUARD_COSCHED (HM_TRACE_OVERLAP=2: A/B, tests).  Guarded scans keep the chip busy through the guard's exact
    // refinements, which are one round of fp32 tiles on a third of the chip each: the refinement of the sampler's marks
    // runs beside the closest-approach rows' split tiles (hm_sdf.hip: sdf_refine_scan_kernel), and the refinement of the
    // closest-approach rows' marks beside the secant chain (sdf_scan_secant_kernel with the list as its scan) - by the
    // workgroups the chain leaves free, on the 64-point body whatever the list's length, as refine() asks.  Same tiles,
    // same values, one stream; the rows of the two lists are disjoint and the sampler's list is patched before the
    // closest-approach rows are selected, so both lists start at the head of the refinement region.
    int seq_guard_cosched() {
        HM_TRY(sampler_beside_scan());
        return closest_rows_own_list([&] { return secant_beside_list(0, a.n_secant, 0); });
    }
    // GUARD_POOLED, the default of the guarded scans: the closest-approach scan is shared out between the launches
    // (hm_sdf.hip: hm_scan_pool.h).  The refinement launches - both passes' of the lazy sampler - take as many of its split
    // tiles as they have idle workgroups, the secant chain's launch (sdf_split_scan_secant_kernel) runs the rest beside the
    // chain, and the closest-approach rows are selected, refined and reduced behind it.
    // The chain is cut in two launches: the first rounds beside ALL remaining tiles of the scan, then - behind the selection
    // of the closest-approach rows - the last k_tail rounds with the one round of exact tiles that refines those rows'
    // marks under them (sdf_scan_secant_kernel<., true>: the tiles and values of refine()'s quarter launch), on the
    // workgroups that own no secant tile.  The chain's state lives in global memory between rounds, so the cut changes no
    // value.  k_tail = 0: the whole chain in front, and the list on the quarter launch alone.
    int seq_guard_pooled() {
        const int n_front = a.n_secant - P.k_tail;
        HM_TRY(sampler_beside_scan());
        HM_TRY(hm_trace_split_scan_secant(&cx, &a, 0, n_front, a.n_secant, C_GUARD_N1, P.c_ref2, a.sel_off, n_scan(),
                                          P.chain_tiles));
        return closest_rows_own_list(
            [&] { return P.k_tail > 0 ? secant_beside_list(n_front, P.k_tail, 1) : refine(C_GUARD_NC, true); });
    }

    int run(int32_t *stats_out) {
        hm_zero_u32_async(a.w.cnt, C_COUNT, as_stream(cx.stream));
        HM_TRY(march());
        first_pass_points();
        switch (P.sequence) {
        case HM_TRACE_SEQ_FILL: HM_TRY(seq_fill()); break;
        case HM_TRACE_SEQ_GUARD_SERIAL: HM_TRY(seq_guard_serial()); break;
        case HM_TRACE_SEQ_GUARD_COSCHED: HM_TRY(seq_guard_cosched()); break;
        case HM_TRACE_SEQ_GUARD_POOLED: HM_TRY(seq_guard_pooled()); break;
        default: HM_TRY(seq_joint()); break;
        }
        hipLaunchKernelGGL(count_evals_kernel, dim3(1), dim3(64), 0, as_stream(cx.stream), a.w.cnt, P.march_rounds + 1, a.n_secant);
        if (stats_out)
            hipLaunchKernelGGL(hm_copy_u32_kernel, dim3(1), dim3(64), 0, as_stream(cx.stream), reinterpret_cast<uint32_t *>(stats_out),
                               reinterpret_cast<const uint32_t *>(a.w.cnt + C_NSAMP), 16);
        HM_CHECK_LAUNCH("hm_trace_forward");
        return HM_OK;
    }
};

}  // namespace

extern "C" {

int64_t hm_trace_workspace_bytes(int64_t n_rays, const hm_trace_cfg *cfg) {
    if (n_rays < 0 || !cfg || cfg->n_steps < 1) return hm_fail(HM_ERR_INVALID, "hm_trace_workspace_bytes: bad argument");
    return trace_layout(nullptr, n_rays, cfg->n_steps, 0, cfg->coarse_bf16 == 3).bytes;
}

int hm_trace_guard_clear(void *workspace, int64_t workspace_bytes, void *stream) {
    HM_CHECK_ARG(workspace && workspace_bytes >= kWsHeader, "hm_trace_guard_clear: no workspace");
    hm_zero_u32_async(reinterpret_cast<int32_t *>(workspace), kWsHeader / sizeof(int32_t), as_stream(stream));
    HM_CHECK_LAUNCH("hm_trace_guard_clear");
    return HM_OK;
}

int hm_trace_guard_tolerances(float *tau, float *tau_trip) {
    HM_CHECK_ARG(tau && tau_trip, "hm_trace_guard_tolerances: NULL pointer");
    *tau = kGuardTau;
    *tau_trip = kGuardTrip;
    return HM_OK;
}

int64_t hm_trace_workspace_bytes_nffb(int64_t n_rays, const hm_trace_cfg *cfg, int n_levels) {
    if (n_rays < 0 || !cfg || cfg->n_steps < 1 || n_levels < 1 || n_levels > HM_MAX_LEVELS)
        return hm_fail(HM_ERR_INVALID, "hm_trace_workspace_bytes_nffb: bad argument");
    return trace_layout(nullptr, n_rays, cfg->n_steps, nffb_emb_width(n_levels), false).bytes;
}

int hm_diag_trace_plan(int64_t n_rays, const hm_trace_cfg *cfg, int tile_points, int has_nffb, hm_trace_plan_info *info) {
    HM_CHECK_ARG(n_rays >= 0 && cfg && info && cfg->n_steps >= 2, "hm_diag_trace_plan: bad argument");
    *info = trace_plan(*cfg, n_rays, tile_points, has_nffb != 0, trace_switches());
    return HM_OK;
}

static int trace_forward_impl(const HmTraceCtx &cx, const hm_trace_cfg *cfg, const float *cam_loc, const float *ray_dirs,
                              const uint8_t *object_mask, const float *t_sphere, const uint8_t *hit_mask, int64_t n_rays,
                              int64_t rays_per_image, const float *sampler_fracs, const float *steps_u, float *out_points,
                              uint8_t *out_net_mask, float *out_dists, void *workspace, int64_t workspace_bytes,
                              int32_t *stats_out) {
    HM_CHECK_ARG(cx.desc && cx.mlp && cfg, "hm_trace_forward: NULL descriptor");
    HM_CHECK_ARG(n_rays >= 0 && rays_per_image >= 1, "hm_trace_forward: bad ray counts");
    HM_CHECK_ARG(cfg->n_steps >= 2 && cfg->n_steps <= 4096, "hm_trace_forward: n_steps out of range");
    HM_CHECK_ARG(cfg->sphere_tracing_iters >= 0 && cfg->sphere_tracing_iters <= 15 && cfg->line_step_iters >= 0 &&
                     cfg->line_step_iters <= 3 &&
                     1 + cfg->sphere_tracing_iters * (1 + cfg->line_step_iters) <= 64,
                 "hm_trace_forward: too many march rounds (sphere_tracing_iters <= 15, line_step_iters <= 3)");
    HM_CHECK_ARG(cfg->n_secant_steps >= 0 && cfg->n_secant_steps <= 64, "hm_trace_forward: n_secant_steps out of range");
    if (n_rays == 0) return HM_OK;
    HM_CHECK_ARG(n_rays * (int64_t)cfg->n_steps < (1ll << 31), "hm_trace_forward: too many rays for one call");
    HM_CHECK_ARG(cx.table && cx.B_fourier && cam_loc && ray_dirs && object_mask && t_sphere && hit_mask && sampler_fracs &&
                     out_points && out_net_mask && out_dists && workspace,
                 "hm_trace_forward: NULL pointer");
    HM_CHECK_ARG(!cfg->training || steps_u, "hm_trace_forward: training mode needs steps_u");
    HM_CHECK_ARG(cfg->coarse_bf16 >= 0 && cfg->coarse_bf16 <= 3, "hm_trace_forward: coarse_bf16 must be 0, 1, 2 or 3");
    const bool guard = cfg->coarse_bf16 == 3;
    HM_CHECK_ARG(!guard || !cx.nffb, "hm_trace_forward: the guarded coarse scans do not cover filter-bank embedders");
    HM_CHECK_ARG(!guard || 3 * n_rays * (int64_t)cfg->n_steps < (1ll << 31), "hm_trace_forward: too many rays for one call");
    TraceRun R;
    R.cx = cx; R.cfg = cfg;
    R.P = trace_plan(*cfg, n_rays, cx.tile_points, cx.nffb != nullptr, trace_switches());
    R.emb_width = cx.nffb ? nffb_emb_width(cx.nffb->n_levels) : 0;
    const TraceLayout L = trace_layout(workspace, n_rays, cfg->n_steps, R.emb_width, guard);
    HM_CHECK_ARG(workspace_bytes >= L.bytes, "hm_trace_forward: workspace too small");
    R.emb_ws = L.emb_ws;
    TraceArgs &a = R.a;
    a.w = L.w;
    a.cam = cam_loc; a.dirs = ray_dirs; a.obj = object_mask; a.t_sphere = t_sphere; a.hit = hit_mask;
    a.fracs = sampler_fracs; a.steps_u = steps_u;
    a.out_pts = out_points; a.out_mask = out_net_mask; a.out_t = out_dists;
    a.n = n_rays; a.rays_per_image = rays_per_image;
    a.thr = cfg->sdf_threshold;
    for (int k = 0; k < 4; ++k) a.back[k] = (float)((1.0 - cfg->line_search_step) / (double)(1 << k));
    a.ls_iters = cfg->line_step_iters; a.max_it = cfg->sphere_tracing_iters; a.n_steps = cfg->n_steps;
    a.n_secant = cfg->n_secant_steps; a.training = cfg->training;
    a.head = R.P.head;
    a.tail_off = a.w.cap;
    a.sel_off = R.P.sel_own ? 2 * a.w.cap : -1;
    return R.run(stats_out);
}

int hm_trace_forward(const hm_grid_desc *desc, const hm_mlp_desc *mlp, const float *table, const float *B_fourier,
                     int frac_mode, int tile_points, const hm_trace_cfg *cfg, const float *cam_loc,
                     const float *ray_dirs, const uint8_t *object_mask, const float *t_sphere,
                     const uint8_t *hit_mask, int64_t n_rays, int64_t rays_per_image, const float *sampler_fracs,
                     const float *steps_u, float *out_points, uint8_t *out_net_mask, float *out_dists,
                     void *workspace, int64_t workspace_bytes, int32_t *stats_out, void *stream) {
    return trace_forward_impl({desc, nullptr, mlp, table, B_fourier, frac_mode, tile_points, stream}, cfg, cam_loc, ray_dirs,
                              object_mask, t_sphere, hit_mask, n_rays, rays_per_image, sampler_fracs, steps_u, out_points,
                              out_net_mask, out_dists, workspace, workspace_bytes, stats_out);
}

int hm_trace_forward_nffb(const hm_grid_desc *desc, const hm_nffb_desc *nffb, const hm_mlp_desc *mlp, const float *table,
                          const float *B_fourier, int frac_mode, int tile_points, const hm_trace_cfg *cfg,
                          const float *cam_loc, const float *ray_dirs, const uint8_t *object_mask, const float *t_sphere,
                          const uint8_t *hit_mask, int64_t n_rays, int64_t rays_per_image, const float *sampler_fracs,
                          const float *steps_u, float *out_points, uint8_t *out_net_mask, float *out_dists,
                          void *workspace, int64_t workspace_bytes, int32_t *stats_out, void *stream) {
    HM_CHECK_ARG(nffb != nullptr, "hm_trace_forward_nffb: NULL embedder descriptor");
    return trace_forward_impl({desc, nffb, mlp, table, B_fourier, frac_mode, tile_points, stream}, cfg, cam_loc, ray_dirs,
                              object_mask, t_sphere, hit_mask, n_rays, rays_per_image, sampler_fracs, steps_u, out_points,
                              out_net_mask, out_dists, workspace, workspace_bytes, stats_out);
}

}  // extern "C"
