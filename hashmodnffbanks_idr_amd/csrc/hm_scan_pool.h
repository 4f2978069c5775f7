// hm_scan_pool.h - which split tiles of the closest-approach scan each launch of the guarded search owns
// (scan_pool_quota).  Included inside hm_sdf.hip's anonymous namespace, behind hm_trace_dev.h, hm_sdf_tile64.h and
// hm_sdf_split_tile.h (kTraceScanHide, kPts, kPS, kSdfSmall ...).
//
// The scan depends on neither the sampler nor the secant, so its tiles fill what the other launches leave idle:
//   X1  sdf_refine_scan_kernel, refinement list of the sampler's first (or only) pass: one round of fp32 (half) tiles
//   X2  the same kernel with the list of the lazy sampler's second pass (sampler_head > 0 only)
//   Y   sdf_split_scan_secant_kernel: the secant chain, n_iters dependent rounds on a few dozen workgroups
// A launch never continues another launch's cursor (a workgroup that drew an index past its launch's share would lose the
// tile).  As with fill_quota, the ranges are a pure function of device counters that are final before X1 starts, every
// launch evaluates it the same way, and each hands out [first, first + quota) from a cursor of its own that is zero at launch.
//   X1 and X2 take one tile per workgroup that holds no fp32 tile; the last of them in front of the secant chain also
//   takes what does not fit under the chain: capacity = (256 - secant workgroups) * chain_tiles, chain_tiles = the tiles
//   one workgroup finishes while the chain runs (host: floor(n_iters * kScanTilesPerSecantIterPermille / 1000), or
//   HM_TRACE_POOL_CHAIN_TILES).  Y takes the rest.  chain_tiles = 0 (or no secant ray): everything in front of the chain.
//   Where the chain is cut in two launches (hm_trace.hip: k_tail), Y is the FIRST of them: the scan must be complete
//   before the closest-approach rows are selected, which happens between the two, so the second launch (the chain's last
//   rounds beside those rows' refinement list) owns no tile of the scan.  The ranges stay those of the whole chain
//   (n_iters = its length): what Y's shorter chain does not cover is a last round of all of Y's workgroups, which costs
//   less than the same tiles in front of the chain (measured: profiles/chain_tail_ab.json).
// The number of secant rays is not known before the sampler's values are patched and reduced, i.e. behind X1 and X2; the
// rule reads its upper bound, the rays handed to the sampler (cnt[C_NSAMP]; training refines those of them that hit inside
// the object mask), in every launch.
#pragma once

struct ScanPool {
    int64_t first[3], quota[3];    // X1, X2, Y
};

// workgroups of a cursor-scheduled 64-point launch (sdf64_run<FRAC, true>) over n points that get a tile
__host__ __device__ inline int64_t sdf64_busy_workgroups(int64_t n, int64_t grid) {
    if (n <= 0) return 0;
    if (n / kPts >= grid) return grid;                        // at least one full round
    const int64_t step = n <= grid * 32 ? 32 : kPts;          // (the half-tile rule of the remainder round)
    const int64_t tiles = (n + step - 1) / step;
    return tiles < grid ? tiles : grid;
}

// n_scan: points of the closest-approach scan; n_ref1 / n_ref2: points of the refinement lists of X1 / X2 (two_x = 0: there
// is no X2; X1 does not read n_ref2, which is not final when it runs); grid_x: workgroups of the X launches; n_sec_bound:
// upper bound of the secant rays.
__host__ __device__ inline ScanPool scan_pool_quota(int64_t n_scan, int64_t n_ref1, int64_t n_ref2, int two_x,
                                                    int64_t grid_x, int64_t n_sec_bound, int64_t chain_tiles) {
    const int64_t tiles = n_scan > kSdfSmall ? (n_scan + kPS - 1) / kPS : 0;   // (shorter scans: the exact small-tile launch)
    int64_t capacity = 0;
    if (n_sec_bound > 0 && chain_tiles > 0) {
        // the secant's tile rule (sdf_split_scan_secant_kernel) at the bound
        const int pts = n_scan >= kTraceScanHide ? 16 : (n_sec_bound <= kSdfMini ? 4 : (n_sec_bound <= kSdfTiny ? 8 : 16));
        const int64_t sec_tiles = (n_sec_bound + pts - 1) / pts;
        capacity = (256 - (sec_tiles < 256 ? sec_tiles : 256)) * chain_tiles;
    }
    const int64_t over = tiles > capacity ? tiles - capacity : 0;
    const int64_t idle1 = grid_x - sdf64_busy_workgroups(n_ref1, grid_x);
    const int64_t idle2 = grid_x - sdf64_busy_workgroups(n_ref2, grid_x);
    ScanPool p;
    const int64_t want1 = two_x ? idle1 : (idle1 > over ? idle1 : over);
    p.quota[0] = want1 < tiles ? want1 : tiles;
    const int64_t left = tiles - p.quota[0];
    const int64_t over2 = over > p.quota[0] ? over - p.quota[0] : 0;
    const int64_t want2 = two_x ? (idle2 > over2 ? idle2 : over2) : 0;
    p.quota[1] = want2 < left ? want2 : left;
    p.quota[2] = left - p.quota[1];
    p.first[0] = 0;
    p.first[1] = p.quota[0];
    p.first[2] = p.quota[0] + p.quota[1];
    return p;
}
