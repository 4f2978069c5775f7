// hm_trace_host.h - the host interface between the ray search (hm_trace.hip: which launches go out, in what order) and
// the fused kernels it launches (hm_sdf.hip, where each kernel's comment says what the launch does).  Internal, not
// exported: both files include this header, so a parameter that one side adds and the other does not is a compile error.
// `trace_args` = a TraceArgs of hm_trace_dev.h (each file includes that header in its own anonymous namespace).
#pragma once
#include "hm_common.h"

// What never varies within one call of the tracer.
struct HmTraceCtx {
    const hm_grid_desc *desc;
    const hm_nffb_desc *nffb;    // filter-bank embedder (NULL: hash-grid network)
    const hm_mlp_desc *mlp;
    const float *table, *B_fourier;
    int frac_mode, tile_points;
    void *stream;
};

extern "C" {
// rounds [first, rounds) of the sphere-tracing march as ONE persistent launch (trace_march_tail_kernel); tile_points 16:
// the 16-point body always
int hm_trace_march_tail(const HmTraceCtx *cx, const void *trace_args, int first, int rounds);

// all secant iterations as ONE launch (trace_secant_kernel).  tile_points 0 = the tile size follows the list's length as
// in hm_sdf_fwd; 4 / 8 / 16 = fixed.  scan_rule != 0 (tile_points 0 only): 16-point tiles when the closest-approach scan
// has at least kTraceScanHide points, as hm_trace_scan_secant chooses them.
int hm_trace_secant_persistent(const HmTraceCtx *cx, const void *trace_args, int n_iters, int scan_rule);

// A 64-point-tile scan (scan_capacity points at scan_x, values to scan_out, count cnt[c_scan]) and iterations
// [it_first, it_first + n_iters) of a secant chain of it_total in ONE launch (sdf_scan_secant_kernel).  tile_points = 0 only.
// small_front != 0 - the closest-approach scan of the exact mode: scans of <= kSdfSmall points run on the small-tile launch
// in front of it; 0 - a refinement list of the guarded mode: every count runs on the 64-point body, and no sampler launch
// took tiles of it (c_prev* = -1).  quarter != 0 (a refinement list only): the list on the tile schedule of hm_sdf_fwd
// with HM_SDF_TILE64_QUARTER.
int hm_trace_scan_secant(const HmTraceCtx *cx, const void *trace_args, int it_first, int n_iters, int it_total, int quarter,
                         const float *scan_x, float *scan_out, int64_t scan_capacity, int c_scan, int small_front,
                         int c_prev1, int grid1, int c_prev2, int grid2);

// Guarded coarse scans: the exact refinement of the list ref_pts -> ref_vals and this launch's range (hm_scan_pool.h) of the
// split tiles of the closest-approach scan (scan_capacity points at pts + scan_off, count cnt[C_NSEL_PTS]) in ONE launch
// (sdf_refine_scan_kernel).  tile_points = 0 only.  which = 0: the launch of the list cnt[c_ref1] - the first one, which
// also enqueues the exact small-tile launch for scans of <= kSdfSmall points; which = 1: of cnt[c_ref2], the lazy
// sampler's second pass (c_ref2 < 0: there is no second launch).  chain_tiles: split tiles one workgroup finishes under
// the secant chain (0: the whole scan runs in front of the chain).
int hm_trace_refine_scan(const HmTraceCtx *cx, const void *trace_args, int c_ref1, int c_ref2, int which, int64_t scan_off,
                         int64_t scan_capacity, int64_t chain_tiles);

// Guarded coarse scans: iterations [it_first, it_first + n_iters) of a secant chain of it_total and the split tiles of the
// closest-approach scan that the hm_trace_refine_scan launches in front left over, in ONE launch
// (sdf_split_scan_secant_kernel).  c_ref1 / c_ref2 / scan_off / chain_tiles: as given to those launches.
int hm_trace_split_scan_secant(const HmTraceCtx *cx, const void *trace_args, int it_first, int n_iters, int it_total,
                               int c_ref1, int c_ref2, int64_t scan_off, int64_t scan_capacity, int64_t chain_tiles);

// hm_sdf_fwd for the ray search's sampler launches: the 64-point launch completes its last round with tiles of a second
// point set (fill_quota; x_fill / out_fill / n_fill_dev: the closest-approach scan's points, values and device-side count;
// prev_dev / prev_grid: own-point count and grid of the launch that took filler tiles before this one).
// *grid64_out = the 64-point launch's grid (0: there was none), for the next launch of the chain.
int hm_sdf_fwd_fill(const HmTraceCtx *cx, const float *x, int64_t n, float *out, const int32_t *n_dev, const float *x_fill,
                    float *out_fill, const int32_t *n_fill_dev, const int32_t *prev_dev, int prev_grid, int *grid64_out);
}
