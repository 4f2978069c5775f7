"""The closest-approach scan's tile ranges per launch of the guarded ray search (csrc/hm_scan_pool.h: scan_pool_quota, asked
on the host through hm_trace_scan_pool_plan): over a sweep of counts the ranges of the launches - refine-scan launch of the
sampler's first pass (X1), of the lazy sampler's second pass (X2, head > 0 only), secant launch (Y) - partition [0, tiles)
without gap or overlap, equal the rule written out here, and reach its three regimes: everything in front of the chain,
split between the launches, overflow back into the last launch in front of the chain."""
import ctypes
import itertools

import pytest

SMALL, HIDE, MINI, TINY = 8192, 3 * 256 * 64, 1024, 2048     # hm_common.h: kSdfSmall, kTraceScanHide, kSdfMini, kSdfTiny
PERMILLE = 875                                              # hm_trace_dev.h: kScanTilesPerSecantIterPermille


@pytest.fixture(scope="module")
def plan():
    from hashmodnffbanks_idr_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()

    def call(n_scan, n_ref1, n_ref2, two_x, grid, n_sec, n_iters, chain=-1):
        first, quota = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
        _lib.check(lib.hm_trace_scan_pool_plan(n_scan, n_ref1, n_ref2, int(two_x), grid, n_sec, n_iters, chain, first, quota))
        return list(first), list(quota)
    return call


def _busy(n, grid):
    """workgroups of a cursor-scheduled 64-point launch over n points that get a tile (half tiles up to 32 per workgroup)"""
    if n <= 0:
        return 0
    if n // 64 >= grid:
        return grid
    step = 32 if n <= grid * 32 else 64
    return min(grid, -(-n // step))


def _chain_tiles(n_iters, chain):
    if n_iters <= 0:
        return 0
    return chain if chain >= 0 else n_iters * PERMILLE // 1000


def _capacity(n_scan, n_sec, n_iters, chain):
    ct = _chain_tiles(n_iters, chain)
    if n_sec <= 0 or ct <= 0:
        return 0
    pts = 16 if n_scan >= HIDE else (4 if n_sec <= MINI else (8 if n_sec <= TINY else 16))
    return (256 - min(256, -(-n_sec // pts))) * ct


def _expect(n_scan, n_ref1, n_ref2, two_x, grid, n_sec, n_iters, chain=-1):
    tiles = -(-n_scan // 64) if n_scan > SMALL else 0
    over = max(tiles - _capacity(n_scan, n_sec, n_iters, chain), 0)
    idle1, idle2 = grid - _busy(n_ref1, grid), grid - _busy(n_ref2, grid)
    q1 = min(tiles, idle1 if two_x else max(idle1, over))
    q2 = min(tiles - q1, max(idle2, over - q1)) if two_x else 0
    return [0, q1, q1 + q2], [q1, q2, tiles - q1 - q2]


SCANS = (0, 1, 8192, 8193, 8256, 9000, 20000, 49151, 49152, 76700, 76800, 100000, 150000, 204800)
LISTS = (0, 1, 31, 32, 33, 2000, 6000, 8192, 8193, 16384, 20000)
SECS = (0, 1, 16, 960, 1024, 1025, 1281, 2048)


@pytest.mark.parametrize("two_x", [False, True], ids=["head0", "head16"])
@pytest.mark.parametrize("n_iters", [0, 8])
def test_ranges_partition_the_scan(plan, n_iters, two_x):
    seen = set()
    for n_scan, n_ref1, n_sec, grid, chain in itertools.product(SCANS, LISTS, SECS, (256, 64), (-1, 0, 1, 3)):
        n_ref2 = (n_ref1 * 7) % 9001 if two_x else 0
        first, quota = plan(n_scan, n_ref1, n_ref2, two_x, grid, n_sec, n_iters, chain)
        what = (n_scan, n_ref1, n_ref2, two_x, grid, n_sec, n_iters, chain)
        tiles = -(-n_scan // 64) if n_scan > SMALL else 0
        assert all(q >= 0 for q in quota) and sum(quota) == tiles, what
        assert first[0] == 0 and first[1] == quota[0] and first[2] == quota[0] + quota[1], what     # no gap, no overlap
        assert two_x or quota[1] == 0, what
        assert (first, quota) == _expect(*what), what
        if n_sec == 0 or n_iters == 0 or chain == 0:
            assert quota[2] == 0, what      # no chain to hide tiles under: the whole scan in front of it
        if tiles:
            idle = sum(quota[:2]) <= (grid - _busy(n_ref1, grid)) + (grid - _busy(n_ref2, grid) if two_x else 0)
            seen.add("front" if quota[2] == 0 else ("split" if idle else "overflow"))
    assert seen == ({"front"} if n_iters == 0 else {"front", "split", "overflow"}), seen


def test_bench_shape_regimes(plan):
    """the bench step (C2, 2048 rays: scan 76 700 points = 1199 tiles, sampler list ~6 k points = 190 half tiles, 1281
    sampler rays = 81 secant workgroups at most, 8 secant rounds = 7 tiles per workgroup under the chain): capacity
    175 * 7 = 1225; scans below, at and above it"""
    assert _chain_tiles(8, -1) == 7 and _capacity(76700, 1281, 8, -1) == 1225
    idle = 256 - _busy(6050, 256)
    assert idle == 66
    for tiles, want in ((1199, [66, 0, 1133]), (1225 + 66, [66, 0, 1225]), (1225 + 67, [67, 0, 1225]), (1500, [275, 0, 1225])):
        assert plan(tiles * 64, 6050, 0, False, 256, 1281, 8)[1] == want
    # lazy sampler: the overflow belongs to the second launch; the first takes its idle workgroups only
    assert plan(1199 * 64, 3000, 6050, True, 256, 1281, 8)[1] == [256 - 94, 66, 1199 - 162 - 66]
    assert plan(1700 * 64, 3000, 6050, True, 256, 1281, 8)[1] == [162, 1700 - 1225 - 162, 1225]
    # override: 1 tile per workgroup under the chain -> most of the scan flows back; 0 -> all of it; no secant ray -> all
    assert plan(1199 * 64, 6050, 0, False, 256, 1281, 8, 1)[1] == [1199 - 175, 0, 175]
    assert plan(1199 * 64, 6050, 0, False, 256, 1281, 8, 0)[1] == [1199, 0, 0]
    assert plan(1199 * 64, 6050, 0, False, 256, 0, 8)[1] == [1199, 0, 0]
    # a scan of at most 8192 points is the small-tile launch's
    assert plan(8192, 6050, 0, False, 256, 1281, 8)[1] == [0, 0, 0]


def test_bad_arguments(plan):
    from hashmodnffbanks_idr_amd._lib import HashmodArgumentError
    for bad in ((-1, 0, 0, False, 256, 0, 8), (100, 0, 0, False, 0, 0, 8), (100, 0, 0, False, 257, 0, 8),
                (100, 0, 0, False, 256, 0, 8, -2)):
        with pytest.raises(HashmodArgumentError):
            plan(*bad)
