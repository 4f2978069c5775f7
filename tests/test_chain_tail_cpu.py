"""The secant chain cut in two launches (csrc/hm_trace.hip: k_tail; csrc/hm_scan_pool.h): the first launch runs the chain's
first k rounds beside ALL remaining split tiles of the closest-approach scan, the second its last rounds beside the
closest-approach rows' refinement list.  Asked on the host through hm_trace_scan_pool_plan: over a grid of counts and for
every number k of rounds the rule may be asked with, the ranges of the refine-scan launches (X1, X2) and of the chain's
first launch (Y) partition the scan's tiles exactly - whatever is not in front of the chain belongs to Y, so the launch
behind the cut owns no tile of the scan."""
import ctypes

import pytest

SMALL = 8192          # hm_common.h: kSdfSmall - shorter scans run on the exact small-tile launch
PERMILLE = 875        # hm_trace_dev.h: kScanTilesPerSecantIterPermille

SCAN_TILES = (0, 1, 128, 129, 200, 256, 607, 875, 876, 1133, 1199, 1225, 1226, 1500, 2047, 3000)
LIST_TILES = (0, 1, 60, 115, 190, 220, 256, 257, 400)      # 32-point half tiles of the sampler's list
SAMPLER_RAYS = (0, 1, 16, 960, 1024, 1025, 1281, 2048, 4096)
ROUNDS = tuple(range(9))


@pytest.fixture(scope="module")
def plan():
    from hashmodnffbanks_idr_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()

    def call(n_scan, n_ref1, n_ref2, two_x, n_sec, k, chain=-1):
        first, quota = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
        _lib.check(lib.hm_trace_scan_pool_plan(n_scan, n_ref1, n_ref2, int(two_x), 256, n_sec, k, chain, first, quota))
        return list(first), list(quota)
    return call


@pytest.mark.parametrize("two_x", [False, True], ids=["head0", "head16"])
def test_ranges_partition_the_scan_for_every_cut(plan, two_x):
    for k in ROUNDS:
        for st in SCAN_TILES:
            for n_scan in {64 * st, max(64 * st - 37, 0)}:      # (a ragged last tile too)
                tiles = -(-n_scan // 64) if n_scan > SMALL else 0
                for lt in LIST_TILES:
                    for n_sec in SAMPLER_RAYS:
                        n_ref1 = 32 * lt
                        n_ref2 = (n_ref1 * 7) % 9001 if two_x else 0
                        first, quota = plan(n_scan, n_ref1, n_ref2, two_x, n_sec, k)
                        what = (n_scan, n_ref1, n_ref2, two_x, n_sec, k)
                        # X1, X2 and Y: consecutive, disjoint, and together the whole scan - nothing is left for a launch behind Y
                        assert all(q >= 0 for q in quota), what
                        assert first == [0, quota[0], quota[0] + quota[1]], what
                        assert sum(quota) == tiles, what
                        assert two_x or quota[1] == 0, what
                        if k == 0 or n_sec == 0:
                            assert quota[2] == 0, what          # no round in front of the cut hides a tile
                        else:
                            assert quota[2] <= 256 * (k * PERMILLE // 1000), what


def test_ranges_of_the_bench_step_by_rounds_counted(plan):
    """the bench step (1199 tiles, sampler list 6050 points = 66 idle workgroups in X1, 1281 sampler rays = 81 secant
    workgroups at most).  The cut sequence asks with the whole chain's 8 rounds: the first launch of the chain keeps the
    1133 tiles of the uncut sequence.  Asked with the 6 rounds in front of the cut, the chain would hide
    175 * floor(6 * 0.875) = 875 tiles and X1 keep the other 324 - measured slower (profiles/chain_tail_ab.json), not used"""
    assert plan(1199 * 64, 6050, 0, False, 1281, 8)[1] == [66, 0, 1133]
    assert plan(1199 * 64, 6050, 0, False, 1281, 6)[1] == [324, 0, 875]
    assert plan(1199 * 64, 6050, 0, False, 1281, 7)[1] == [149, 0, 1050]
    assert plan(1199 * 64, 6050, 0, False, 1281, 5)[1] == [499, 0, 700]
    assert plan(1199 * 64, 6050, 0, False, 1281, 1)[1] == [1199, 0, 0]          # floor(0.875) = 0: nothing under one round
    # the override counts tiles per workgroup whatever the cut
    assert plan(1199 * 64, 6050, 0, False, 1281, 6, 7)[1] == [66, 0, 1133]
    # lazy sampler: what does not fit under the shortened chain goes to the second refine-scan launch
    assert plan(1199 * 64, 3000, 6050, True, 1281, 6)[1] == [162, 1199 - 875 - 162, 875]
