"""The case table of the grouped weight-gradient GEMM (hm_gemm_f32_group_tn / _det) and a host model of how
group_tn in csrc/hm_gemm.hip walks a list, shared by tests/test_gemm_group_cpu.py (the model against the library's
workspace query, and that the lists reach every branch of the walk) and tests/test_gemm_group_gpu.py (the same lists
run on the device against float64).

The model, in the words of include/hashmod.h and group_tn's comments:
  * an item with K % 128 != 0, or whose A or B spans 2 GB or more (4 ld K >= 2^31: the grouped kernel forms 32-bit
    operand offsets), goes alone to hm_gemm_f32 / _det;
  * every other item joins the current table; a table is launched when it holds HM_GEMM_GROUP_MAX entries and, in the
    deterministic form, before an item whose C byte window overlaps a tabled one's (tabled or alone: the sums are then
    added in item order);
  * a tabled item's K is cut into expected_split(K) parts, and the deterministic form gives it that many M x N slabs of
    the workspace; the slabs of a table are reused by the next one, so a call needs the largest table's (or the largest
    need of an item that goes alone)."""
from collections import namedtuple

from gemm_cases import LAYOUTS

GROUP_MAX = 16            # HM_GEMM_GROUP_MAX (include/hashmod.h)


def expected_split(K):
    """k parts of >= 1024 that divide K into multiples of 128, at most 4"""
    split = min(max(K // 1024, 1), 4)
    while split > 1 and (K % split != 0 or (K // split) % 128 != 0):
        split -= 1
    return split


def alone_reasons(M, N, K, lda, ldb):
    out = set()
    if K % 128 != 0:
        out.add("ktail")
    if 4 * lda * K >= 2 ** 31 or 4 * ldb * K >= 2 ** 31:
        out.add("span")
    return out


def goes_alone(M, N, K, lda, ldb):
    return bool(alone_reasons(M, N, K, lda, ldb))


# one problem as the library sees it: dimensions, leading dimensions and the ADDRESS of C (any integer: the workspace
# query reads no memory)
Placed = namedtuple("Placed", "M N K lda ldb ldc c_ptr")
Walk = namedtuple("Walk", "need tables alone flushes")


def _window(p):
    return p.c_ptr, p.c_ptr + 4 * ((p.M - 1) * p.ldc + p.N)


def walk(placed, alone_need):
    """the deterministic call's walk over a list: Walk(need in bytes, tables as lists of (item index, split), alone
    items as (item index, reasons), the reason of every table flush before the last).  alone_need(M, N, K, lda, ldb)
    is the workspace of an item that goes alone (hm_gemm_f32_det_workspace_bytes(1, 0, ...))."""
    need, tables, alone, flushes, table = 0, [], [], [], []

    def overlaps(p):
        a0, a1 = _window(p)
        return any(not (a1 <= b0 or b1 <= a0) for b0, b1 in (_window(placed[i]) for i, _ in table))

    def flush(reason):
        nonlocal need, table
        if table:
            need = max(need, 4 * sum(s * placed[i].M * placed[i].N for i, s in table))
            tables.append(table)
            if reason:
                flushes.append(reason)
        table = []

    for i, p in enumerate(placed):
        if p.M == 0 or p.N == 0 or p.K == 0:
            continue
        why = alone_reasons(p.M, p.N, p.K, p.lda, p.ldb)
        if why:
            if overlaps(p):
                flush("alone-overlap")
            need = max(need, alone_need(p.M, p.N, p.K, p.lda, p.ldb))
            alone.append((i, why))
            continue
        if overlaps(p):
            flush("overlap")
        elif len(table) == GROUP_MAX:
            flush("count")
        table.append((i, expected_split(p.K)))
    flush(None)
    return Walk(need, tables, alone, flushes)


def expected_need(placed, alone_need):
    return walk(placed, alone_need).need


# ---- the case table ------------------------------------------------------------------------------------------------
# la / lb: names of gemm_cases.LAYOUTS for the stored A [K, M] and B [K, N]; lda: an explicit row stride of A (the 2 GB
# edge) instead of M + pad.  C is always a window of ld = ctot + 3 in a sentinel-framed buffer: ckey None = a window of
# its own, items with equal ckey share one [M, ctot] window and write its columns [col0, col0 + N).
Item = namedtuple("Item", "M N K la lb ckey col0 ctot lda")
GroupCase = namedtuple("GroupCase", "name items")


def item(M, N, K, la="dense", lb="dense", ckey=None, col0=0, ctot=None, lda=None):
    return Item(M, N, K, la, lb, ckey, col0, N if ctot is None else ctot, lda)


def lda_of(it):
    return it.lda if it.lda is not None else it.M + LAYOUTS[it.la].pad


def ldb_of(it):
    return it.N + LAYOUTS[it.lb].pad


def ldc_of(it):
    return it.ctot + 3


def window_keys(items):
    """the C window of every item: its ckey, or one of its own"""
    return [it.ckey if it.ckey is not None else ("own", i) for i, it in enumerate(items)]


def place(items):
    """the list with placeholder addresses: every C window 4 GB from the next one, on a 16-byte boundary"""
    base = {}
    for k in window_keys(items):
        base.setdefault(k, 0x7e0000000000 + (len(base) << 32))
    return [Placed(it.M, it.N, it.K, lda_of(it), ldb_of(it), ldc_of(it), base[k] + 4 * it.col0)
            for it, k in zip(items, window_keys(items))]


def fake_ab(it):
    """operand addresses with the item's alignments"""
    return 0x7f0000100000 + 4 * LAYOUTS[it.la].off, 0x7f8000100000 + 4 * LAYOUTS[it.lb].off


# K and the number of k parts it must get (test_gemm_group_cpu.py derives the same figures from expected_split and from
# the library's workspace query)
K_SPLITS = {128: 1, 256: 1, 896: 1, 1024: 1, 1152: 1, 2048: 2, 2176: 1, 3072: 3, 3200: 1, 3328: 2, 4096: 4, 5120: 4,
            6144: 4, 6400: 2, 7168: 4}
ALONE_KS = (1000, 445, 257, 190)                 # no multiple of 128: the plain planner's routes
EDGE_DIMS = (1, 63, 64, 65, 127, 129)            # around one and two 64 x 64 tiles
WIDTHS = (512, 445, 281, 257, 67, 3)             # the training networks' layer widths
LNAMES = tuple(LAYOUTS)                          # dense pad3 off1 off2 off3


def lay(i):
    """layouts of A and B for the i-th item of a list: independent walks over the five (i = 4: off3 A with pad3 B)"""
    return LNAMES[i % 5], LNAMES[(i + 2 + i // 5) % 5]


def _with_layouts(shapes):
    return [item(M, N, K, *lay(i)) for i, (M, N, K) in enumerate(shapes)]


_DIAG = sorted({(d, d) for d in EDGE_DIMS} | {(d, e) for d, e in zip(EDGE_DIMS, reversed(EDGE_DIMS))})
EDGE_LDA = 2 ** 22 - 1                           # K = 128: 4 lda K = 2^31 - 512, the largest offsets the kernel forms

CASES = [
    GroupCase("one", [item(65, 63, 1024)]),
    # every (M, N) pair around the tile at one 128-deep group: 36 items, tables of 16 + 16 + 4
    GroupCase("edge-K128", _with_layouts([(M, N, 128) for M in EDGE_DIMS for N in EDGE_DIMS])),
    GroupCase("edge-K3328", [item(M, N, 3328) for M, N in _DIAG]),
    GroupCase("edge-K4096", _with_layouts([(M, N, 4096) for M, N in _DIAG])),
    GroupCase("widths-K256", _with_layouts([(M, N, 256) for M in WIDTHS for N in WIDTHS])),
    GroupCase("every-K", [item(65, 63, K) for K in K_SPLITS]),
    GroupCase("n16", [item(33, 70, 1024) for _ in range(16)]),
    GroupCase("n17", [item(33, 70, 1024) for _ in range(17)]),
    GroupCase("n33", _with_layouts([(1 + 7 * i % 131, 1 + 11 * i % 67, 128 * (1 + i % 3)) for i in range(33)])),
    GroupCase("zero-sized", [item(0, 5, 128), item(65, 63, 2048), item(7, 0, 256), item(64, 64, 128, "off1", "pad3"),
                             item(9, 6, 1000), item(4, 5, 0)]),
    GroupCase("tabled-and-alone", [item(65, 63, 2048), item(130, 67, 1000), item(3, 257, 128), item(281, 64, 445),
                                   item(67, 65, 4096), item(129, 127, 257), item(64, 3, 190), item(63, 129, 1024)]),
    GroupCase("tabled-and-alone-layouts", _with_layouts([(65, 63, 2048), (130, 67, 1000), (3, 257, 128),
                                                          (281, 64, 445), (67, 65, 4096), (129, 127, 257),
                                                          (64, 3, 190), (63, 129, 1024)])),
    # items 0 and 2 add into one C, item 1 is disjoint
    GroupCase("shared-0-2", [item(65, 63, 2048, ckey="g"), item(65, 63, 1024), item(65, 63, 1024, "pad3", "off1", "g")]),
    GroupCase("shared-tabled-tabled", [item(65, 63, 2048, ckey="g"), item(65, 63, 1024, ckey="g")]),
    GroupCase("shared-tabled-alone", [item(65, 63, 2048, ckey="g"), item(65, 63, 1000, ckey="g")]),
    GroupCase("shared-alone-tabled", [item(65, 63, 1000, ckey="g"), item(65, 63, 2048, ckey="g")]),
    # two column slices of one wide buffer (and a column between them that nobody writes): the byte windows overlap,
    # the elements do not
    GroupCase("column-slices", [item(65, 63, 2048, ckey="w", col0=0, ctot=97),
                                item(65, 33, 1024, "off3", "pad3", ckey="w", col0=64, ctot=97)]),
    # ... and thin ones: the second slice starts past the first one's M * N elements, inside its byte window
    GroupCase("column-slices-thin", [item(2, 3, 1024, ckey="w", col0=0, ctot=13),
                                     item(2, 5, 1024, "pad3", "off2", ckey="w", col0=8, ctot=13)]),
    # the 32-bit edge: the largest A the table takes, and the smallest that goes alone
    GroupCase("span-tabled", [item(2, 3, 128, lda=EDGE_LDA), item(65, 63, 128)]),
    GroupCase("span-alone", [item(2, 3, 128, lda=EDGE_LDA + 1), item(65, 63, 128)]),
]
BY_NAME = {c.name: c for c in CASES}
# lists whose items add into one C, in the order the deterministic form must keep
ORDER = [BY_NAME[n] for n in ("shared-tabled-tabled", "shared-tabled-alone", "shared-alone-tabled", "shared-0-2")]


def is_dense(case):
    return all(it.la == "dense" and it.lb == "dense" and it.ckey is None and it.lda is None for it in case.items)


# non-finite values in one column of A and one of B, at shapes with clamped edge lanes; (M, N, row of C, column of C)
ISOLATION_KS = (128, 3328)
ISOLATION_MN = [(65, 65, 64, 33), (65, 129, 33, 128), (129, 65, 128, 64), (129, 129, 65, 70)]
