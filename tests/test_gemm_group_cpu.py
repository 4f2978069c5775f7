"""hm_gemm_f32_group_tn_det_workspace_bytes against the host model of tests/gemm_group_cases.py, for every list
tests/test_gemm_group_gpu.py runs, and that the lists together reach every branch of group_tn's walk.  Host only: the
query dereferences nothing, so addresses with the cases' alignments and offsets stand in for device pointers."""
import ctypes

import pytest

import gemm_group_cases as GG
from gemm_cases import LAYOUTS


@pytest.fixture(scope="module")
def lib():
    from hashmodnffbanks_idr_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _items(placed, ab=None):
    from hashmodnffbanks_idr_amd import _lib
    arr = (_lib.GemmGroupItem * max(len(placed), 1))()
    for i, p in enumerate(placed):
        a, b = ab[i] if ab else (0x7f0000100000, 0x7f8000100000)
        arr[i] = _lib.GemmGroupItem(a, b, p.c_ptr, p.M, p.N, p.K, p.lda, p.ldb, p.ldc)
    return arr


def _query(lib, placed, ab=None):
    return lib.hm_gemm_f32_group_tn_det_workspace_bytes(ctypes.cast(_items(placed, ab), ctypes.c_void_p), len(placed))


def _alone_need(lib):
    return lambda M, N, K, lda, ldb: lib.hm_gemm_f32_det_workspace_bytes(1, 0, M, N, K, lda, ldb)


def _walk(lib, case):
    return GG.walk(GG.place(case.items), _alone_need(lib))


@pytest.mark.parametrize("case", GG.CASES, ids=lambda c: c.name)
def test_workspace_query_matches_the_model(lib, case):
    placed = GG.place(case.items)
    got = _query(lib, placed, [GG.fake_ab(it) for it in case.items])
    assert got == GG.expected_need(placed, _alone_need(lib)), case.name


@pytest.mark.parametrize("K", list(GG.K_SPLITS), ids=lambda k: f"K{k}")
def test_k_parts_of_one_tabled_item(lib, K):
    """the split of every K of the table, from the rule and from the library (slabs of a one-item list)"""
    M, N = 65, 63
    assert GG.expected_split(K) == GG.K_SPLITS[K]
    assert not GG.goes_alone(M, N, K, M, N)
    got = _query(lib, GG.place([GG.item(M, N, K)]))
    assert got == 4 * M * N * GG.K_SPLITS[K], f"K = {K}: {got / (4 * M * N)} slabs"


def test_alone_items_need_what_the_plain_planner_needs(lib):
    M, N = 65, 63
    slabs = {}
    for K in GG.ALONE_KS:
        assert GG.goes_alone(M, N, K, M, N)
        got = _query(lib, GG.place([GG.item(M, N, K)]))
        assert got == lib.hm_gemm_f32_det_workspace_bytes(1, 0, M, N, K, M, N) and got % (4 * M * N) == 0
        slabs[K] = got // (4 * M * N)
    # the plain planner splits by the tile grid as well as by K: both a split and an unsplit alone item are covered
    assert max(slabs.values()) > 1 and min(slabs.values()) == 0, slabs


def test_span_rule_boundary(lib):
    """4 ld K >= 2^31 on either operand sends the item alone; one element less stays in the table"""
    M, N, K = 2, 3, 128
    edge = GG.EDGE_LDA
    assert 4 * edge * K == 2 ** 31 - 512 and 4 * (edge + 1) * K == 2 ** 31
    tabled = 4 * M * N                                       # one slab
    alone = lib.hm_gemm_f32_det_workspace_bytes(1, 0, M, N, K, edge + 1, N)
    assert alone != tabled                                   # (an unsplit plain GEMM needs no workspace)
    for which in ("lda", "ldb"):
        for ld, want in ((edge, tabled), (edge + 1, alone)):
            p = GG.Placed(M, N, K, ld if which == "lda" else M, ld if which == "ldb" else N, N + 3, 0x7e0000000000)
            assert GG.goes_alone(M, N, K, p.lda, p.ldb) == (ld > edge)
            assert _query(lib, [p]) == want == GG.expected_need([p], _alone_need(lib)), (which, ld)


def test_seventeen_items_need_sixteen_slabs(lib):
    case = GG.BY_NAME["n17"]
    it = case.items[0]
    assert GG.expected_split(it.K) == 1
    assert _query(lib, GG.place(case.items)) == GG.GROUP_MAX * 4 * it.M * it.N
    assert _query(lib, GG.place(GG.BY_NAME["n16"].items)) == GG.GROUP_MAX * 4 * it.M * it.N


def test_overlap_starts_a_table_and_slices_count_as_overlapping(lib):
    it = GG.item(65, 63, 1024)
    one = 4 * 65 * 63
    assert _query(lib, GG.place([it, it])) == 2 * one
    assert _query(lib, GG.place([it._replace(ckey="g"), it._replace(ckey="g")])) == one
    for name in ("column-slices", "column-slices-thin"):
        w = _walk(lib, GG.BY_NAME[name])
        assert w.flushes == ["overlap"] and [len(t) for t in w.tables] == [1, 1]
        a, b = GG.BY_NAME[name].items
        assert _query(lib, GG.place([a, b])) == 4 * max(GG.expected_split(i.K) * i.M * i.N for i in (a, b))
    # the window is [C, C + 4 ((M - 1) ldc + N)): a C that starts where another one ends shares its table
    p = GG.place([it])[0]
    end = p.c_ptr + 4 * ((p.M - 1) * p.ldc + p.N)
    assert _query(lib, [p, p._replace(c_ptr=end)]) == _query(lib, [p._replace(c_ptr=end), p]) == 2 * one
    assert _query(lib, [p, p._replace(c_ptr=end - 4)]) == _query(lib, [p._replace(c_ptr=end - 4), p]) == one
    w = _walk(lib, GG.BY_NAME["shared-0-2"])
    assert w.flushes == ["overlap"] and [[i for i, _ in t] for t in w.tables] == [[0, 1], [2]]
    # an alone item that adds into a tabled item's C sends the table first (item order); the other way round nothing waits
    assert _walk(lib, GG.BY_NAME["shared-tabled-alone"]).flushes == ["alone-overlap"]
    assert _walk(lib, GG.BY_NAME["shared-alone-tabled"]).flushes == []
    # ... and the table that follows starts with empty slabs: [tabled -> C, alone -> C, tabled] needs the larger table
    a, b = GG.item(65, 63, 2048, ckey="g"), GG.item(65, 63, 190, ckey="g")
    assert lib.hm_gemm_f32_det_workspace_bytes(1, 0, 65, 63, 190, 65, 63) == 0
    assert _query(lib, GG.place([a, b, GG.item(65, 63, 1024)])) == 2 * one
    assert _query(lib, GG.place([a, b._replace(ckey=None), GG.item(65, 63, 1024)])) == 3 * one


def test_zero_sized_items_are_skipped(lib):
    case = GG.BY_NAME["zero-sized"]
    zero = [i for i, it in enumerate(case.items) if 0 in (it.M, it.N, it.K)]
    assert zero[0] == 0 and zero[-1] == len(case.items) - 1 and len(zero) == 3
    assert {("M", "N", "K")[(it.M, it.N, it.K).index(0)] for i, it in enumerate(case.items) if i in zero} == {"M", "N", "K"}
    rest = [it for i, it in enumerate(case.items) if i not in zero]
    assert _query(lib, GG.place(case.items)) == _query(lib, GG.place(rest)) > 0
    assert _query(lib, GG.place([case.items[i] for i in zero])) == 0
    assert _query(lib, []) == 0


def test_query_refuses_a_negative_dimension(lib):
    good = GG.place([GG.item(65, 63, 1024)])[0]
    for f in ("M", "N", "K"):
        assert _query(lib, [good, good._replace(**{f: -1})]) == -1, f
    assert _query(lib, [good]) > 0


def test_cases_reach_every_branch_of_the_walk(lib):
    splits, reasons, flushes, sizes, layouts = set(), set(), set(), set(), set()
    for case in GG.CASES:
        w = _walk(lib, case)
        splits |= {s for t in w.tables for _, s in t}
        reasons |= {frozenset(r) for _, r in w.alone}
        flushes |= set(w.flushes)
        sizes |= {len(t) for t in w.tables}
        layouts |= {(it.la, it.lb) for it in case.items}
        tabled = {i for t in w.tables for i, _ in t}
        assert all(it.K in GG.K_SPLITS or it.K % 128 == 0 for i, it in enumerate(case.items) if i in tabled)
    assert splits == {1, 2, 3, 4}
    assert reasons == {frozenset({"ktail"}), frozenset({"span"})}
    assert flushes == {"count", "overlap", "alone-overlap"}
    assert {1, GG.GROUP_MAX} <= sizes and max(sizes) == GG.GROUP_MAX
    assert ("off3", "pad3") in layouts and {a for a, _ in layouts} == {b for _, b in layouts} == set(LAYOUTS)
    # the list sizes around the table size, and every tile edge and training width as M and as N
    assert {1, 16, 17, 33} <= {len(c.items) for c in GG.CASES}
    for K, dims in ((128, GG.EDGE_DIMS), (256, GG.WIDTHS)):
        mn = {(it.M, it.N) for c in GG.CASES for it in c.items if it.K == K}
        assert {(m, n) for m in dims for n in dims} <= mn, K
    for K in (3328, 4096):
        for name in (f"edge-K{K}",):
            its = GG.BY_NAME[name].items
            assert {it.M for it in its} == {it.N for it in its} == set(GG.EDGE_DIMS) and {it.K for it in its} == {K}
    assert set(GG.K_SPLITS) == {it.K for it in GG.BY_NAME["every-K"].items}
    assert set(GG.ALONE_KS) <= {it.K for it in GG.BY_NAME["tabled-and-alone"].items}
    # the span cases sit on the two sides of the rule
    assert not _walk(lib, GG.BY_NAME["span-tabled"]).alone
    assert _walk(lib, GG.BY_NAME["span-alone"]).alone == [(0, {"span"})]
