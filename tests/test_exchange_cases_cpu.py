"""tests/exchange_cases.py on the CPU: the numpy references against independent restatements (a float64 mean, a
slot-by-slot loop), the preconditions the kernels rely on (unique rows inside a list), and the properties the bit-exact
GPU tests of test_exchange_gpu.py rely on: the scale 1/3 separates two roundings from one, the claim-bit words mix listed
and unlisted rows, the copy table reaches all four alignment classes and every tail of the float4 body."""
import numpy as np
import pytest

import exchange_cases as X

I32, U32, F32, F64 = X.I32, X.U32, X.F32, X.F64


def _bit(bits, r):
    return int(bits[r >> 5] >> U32(r & 31)) & 1


# ---- hm_rows_pack ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", X.PACK_F)
def test_pack_inputs_have_the_properties_the_cases_are_named_for(F):
    inp = X.pack_inputs(F)
    rows, bits, extra, dense = inp["rows"], inp["bits"], inp["extra"], inp["dense"]
    assert rows.dtype == I32 and rows.size == X.PACK_CAP + X.PACK_OVER
    assert np.unique(rows).size == rows.size                      # the kernel's precondition
    assert rows[0] == 0 and rows[1] == X.TOTAL_ROWS - 1 and rows.min() >= 0 and rows.max() < X.TOTAL_ROWS
    assert X.TOTAL_ROWS % 32 != 0 and bits.size == X.TOTAL_ROWS // 32 + 1
    assert not set(extra.tolist()) & set(rows.tolist())
    assert all(_bit(bits, r) for r in rows) and all(_bit(bits, r) for r in extra)
    assert int(sum(bin(int(w)).count("1") for w in bits)) == rows.size + extra.size
    # words that hold listed AND claimed-but-unlisted bits: row 0's, the partial last one, and at least 40 more; in the
    # smallest case that packs more than one row (255) several of them have a listed row inside the count
    words = lambda rr: {int(r) >> 5 for r in rr}
    mixed = words(rows) & words(extra)
    assert {0, X.TOTAL_ROWS >> 5} <= mixed and len(mixed) >= 42
    assert len(words(rows[:255]) & words(extra)) >= 10
    assert int(bits[-1]) >> (X.TOTAL_ROWS % 32) == 0              # no bit beyond the table
    # the special values sit in packed slots, every other dense value is a nonzero normal number
    di = dense.view(I32)
    packed = set(di[rows[:8]].reshape(-1).view(U32).tolist())
    assert set(X.SPECIAL_BITS) <= packed
    assert X.SPECIAL_BITS[2] in di[rows[0]].view(U32).tolist()    # the NaN payload is in the count = 1 case
    assert np.count_nonzero(di) == di.size


@pytest.mark.parametrize("F", X.PACK_F)
def test_pack_ref(F):
    inp = X.pack_inputs(F)
    dense, rows, bits = inp["dense"], inp["rows"], inp["bits"]
    cap = X.PACK_CAP
    assert set(X.PACK_COUNTS) == {0, 1, 255, 256, 257, cap} and cap % 256 != 0
    for count in X.PACK_COUNTS + (cap + X.PACK_OVER,):
        payload, d_after, b_after, status = X.pack_ref(dense, rows, count, cap, bits, 0)
        n = min(count, cap)
        assert payload.shape == (cap, 1 + F) and payload.dtype == I32
        assert np.array_equal(payload[:n, 0], rows[:n]) and np.array_equal(payload[:n, 1:], dense.view(I32)[rows[:n]])
        assert bool((payload[n:, 0] == -1).all()) and not payload[n:, 1:].any()
        listed = np.zeros(X.TOTAL_ROWS, dtype=bool)
        listed[rows[:n]] = True
        assert not d_after.view(I32)[listed].any()
        assert np.array_equal(d_after.view(I32)[~listed], dense.view(I32)[~listed])
        for r in range(X.TOTAL_ROWS):
            assert _bit(b_after, r) == (0 if listed[r] else _bit(bits, r)), r
        assert status == max(0, count - cap)
    assert X.pack_ref(dense, rows, cap + X.PACK_OVER, cap, bits, 50)[3] == 50       # a larger earlier overflow stays
    assert X.pack_ref(dense, rows, cap + X.PACK_OVER, cap, bits, 5)[3] == X.PACK_OVER
    assert X.pack_ref(dense, rows, cap, cap, bits, 7)[3] == 7                       # no overflow: unchanged
    assert X.pack_ref(dense, rows, cap + X.PACK_OVER, cap, bits, None)[3] is None   # status == NULL
    assert np.array_equal(dense.view(I32), X.pack_inputs(F)["dense"].view(I32))     # the inputs were not modified


# ---- hm_rows_apply / hm_rows_clear -----------------------------------------------------------------------------------
def test_list_layout_is_the_two_table_layout_of_the_static_exchange():
    (ta, fa, ca), (tb, fb, cb) = X.TABLES["A"], X.TABLES["B"]
    assert (fa, fb) == (2, 8) and X.OFFSETS == {"A": 0, "B": ca * (1 + fa)}
    assert X.STRIDE > ca * (1 + fa) + cb * (1 + fb) and X.SLACK == X.STRIDE - X.OFFSETS["B"] - cb * (1 + fb)
    assert ca % 256 and cb % 256 and ca > 256 and cb > 256 and max(ca, cb) <= 2048
    assert set(X.N_LISTS) == {1, 2, 3, 8} and [F32(s) for s in X.SCALES] == [F32(1), F32(0.5), F32(1 / 3), F32(0.125)]
    buf = X.lists_buffer(3)
    assert buf.shape == (3, X.STRIDE) and buf.dtype == I32
    slack = buf[:, X.STRIDE - X.SLACK:]
    assert bool((slack[:, 0::2] == X.SLACK_ROW).all()) and bool((slack[:, 1::2].view(F32) == 1.0).all())
    for name, (total, F, cap) in X.TABLES.items():
        assert 0 <= X.SLACK_ROW < total
        assert np.array_equal(buf[:, X.OFFSETS[name]:X.OFFSETS[name] + cap * (1 + F)].reshape(3, cap, 1 + F),
                              X.list_segment(name, 3))


@pytest.mark.parametrize("name", sorted(X.TABLES))
@pytest.mark.parametrize("n_lists", X.N_LISTS)
def test_generated_lists_have_unique_rows_and_every_kind_of_entry(name, n_lists):
    total, F, cap = X.TABLES[name]
    seg = X.list_segment(name, n_lists)
    assert seg.shape == (n_lists, cap, 1 + F)
    valid = X.in_range_rows(seg, total)
    for r, rows in enumerate(valid):
        assert np.unique(rows).size == rows.size, "a list names a row twice"       # the kernels' precondition
        assert rows.size == cap - 4 * X.N_SKIP
        for bad in X.skipped_rows(total):
            at = np.nonzero(seg[r, :, 0] == bad)[0]
            assert at.size == X.N_SKIP and bool(seg[r, at, 1:].all())               # skipped entries carry values
            assert at.min() < cap - X.N_SKIP                                        # and are not all at the end
        v = seg[r, :, 1:].view(F32)
        assert float(np.abs(v).min()) >= 2.0 ** -7 and float(np.abs(v).max()) <= 2.0 ** 7
    times = np.zeros(total, dtype=np.int64)
    for rows in valid:
        times[rows] += 1
    assert times[X.SLACK_ROW] == 0 and int((times == 0).sum()) > 100                # rows in no list
    assert int((times == n_lists).sum()) >= X.N_SHARED                              # rows in every list
    if n_lists > 1:
        assert int((times == 1).sum()) > 100                                        # rows in one list only
        shared = np.nonzero(times == n_lists)[0][:X.N_SHARED]
        slots = np.array([[int(np.nonzero(seg[r, :, 0] == row)[0][0]) for r in range(n_lists)] for row in shared])
        assert bool((slots.min(1) != slots.max(1)).any()), "the shared rows sit at the same slot of every list"
    acc = X.accumulator(name)
    assert acc.shape == (total, F) and float(np.abs(acc).min()) >= 2.0 ** -7


@pytest.mark.parametrize("name", sorted(X.TABLES))
@pytest.mark.parametrize("n_lists", X.N_LISTS)
def test_apply_ref_equals_a_slot_loop_and_a_float64_mean(name, n_lists):
    total, F, cap = X.TABLES[name]
    buf, acc = X.lists_buffer(n_lists), X.accumulator(name)
    seg = X.list_segment(name, n_lists)
    for scale in X.SCALES:
        got = X.apply_ref(acc, buf, cap, X.STRIDE, X.OFFSETS[name], n_lists, scale, total)
        s = F32(scale)
        loop = acc.copy()
        sum64, mag64 = acc.astype(F64), np.abs(acc.astype(F64))
        for r in range(n_lists):
            for slot in range(cap):
                row = int(seg[r, slot, 0])
                if 0 <= row < total:
                    for f in range(F):
                        v = seg[r, slot, 1 + f:2 + f].view(F32)[0]
                        loop[row, f] = F32(loop[row, f] + F32(v * s))
                        sum64[row, f] += F64(v) * scale
                        mag64[row, f] += abs(F64(v)) * scale
        assert np.array_equal(got.view(I32), loop.view(I32)), (name, n_lists, scale)
        # n adds of partial sums of magnitude <= mag, n products with the rounded scale: (n + 2) roundings at most
        lim = (n_lists + 2) * X.U * 1.01 * mag64
        assert bool((np.abs(got.astype(F64) - sum64) <= lim).all()), (name, n_lists, scale)
    untouched = np.ones(total, dtype=bool)
    for rows in X.in_range_rows(seg, total):
        untouched[rows] = False
    assert np.array_equal(got[untouched].view(I32), acc[untouched].view(I32))
    assert np.array_equal(acc.view(I32), X.accumulator(name).view(I32))


def test_apply_ref_reads_its_own_segment_only():
    """a reference that mistook the other table's words or the slack for entries would move with them"""
    buf = X.lists_buffer(3)
    for name, other in (("A", "B"), ("B", "A")):
        total, F, cap = X.TABLES[name]
        ref = X.apply_ref(X.accumulator(name), buf, cap, X.STRIDE, X.OFFSETS[name], 3, 0.5, total)
        alt = buf.copy()
        to, fo, co = X.TABLES[other]
        alt[:, X.OFFSETS[other]:X.OFFSETS[other] + co * (1 + fo)] = 1
        alt[:, X.STRIDE - X.SLACK:] = 2
        got = X.apply_ref(X.accumulator(name), alt, cap, X.STRIDE, X.OFFSETS[name], 3, 0.5, total)
        assert np.array_equal(ref.view(I32), got.view(I32))


def test_scale_one_third_separates_two_roundings_from_one():
    """dst = fl(dst + fl(v * s)) against the fused form fl(dst + v * s): the bit-exact GPU comparison at scale 1/3 can
    tell them apart only if they differ on the chosen inputs; at the power-of-two scales they never do"""
    for name, (total, F, cap) in X.TABLES.items():
        buf, acc = X.lists_buffer(1), X.accumulator(name)
        seg = X.list_segment(name, 1)[0]
        ok = (seg[:, 0] >= 0) & (seg[:, 0] < total)
        rows, v = seg[ok, 0], np.ascontiguousarray(seg[ok, 1:]).view(F32)
        for scale in X.SCALES:
            two = X.apply_ref(acc, buf, cap, X.STRIDE, X.OFFSETS[name], 1, scale, total)[rows]
            one = (acc[rows].astype(F64) + v.astype(F64) * F64(F32(scale))).astype(F32)
            differ = int((two.view(I32) != one.view(I32)).sum())
            print(f"    table {name} scale {scale:.4f}: {differ} of {two.size} elements differ from the fused form")
            if F32(scale) == F32(1.0 / 3.0):
                assert differ >= 1
            else:
                assert differ == 0


@pytest.mark.parametrize("name", sorted(X.TABLES))
def test_clear_ref_zeroes_exactly_the_named_rows(name):
    total, F, cap = X.TABLES[name]
    buf, acc = X.lists_buffer(3), X.accumulator(name)
    out, count = X.clear_ref(acc, buf, cap, X.STRIDE, X.OFFSETS[name], 3, total, count=5)
    named = np.zeros(total, dtype=bool)
    for rows in X.in_range_rows(X.list_segment(name, 3), total):
        named[rows] = True
    assert count == 0 and 0 < named.sum() < total
    assert not out[named].view(I32).any() and np.array_equal(out[~named].view(I32), acc[~named].view(I32))
    assert X.clear_ref(acc, buf, cap, X.STRIDE, X.OFFSETS[name], 3, total)[1] is None
    out0, count0 = X.clear_ref(acc, buf, 0, X.STRIDE, X.OFFSETS[name], 3, total, count=5)
    assert count0 == 0 and np.array_equal(out0.view(I32), acc.view(I32))
    # clearing by slot instead of by row would zero other rows
    assert not np.array_equal(np.nonzero(named)[0], np.arange(named.sum()))


# ---- the simulated world ---------------------------------------------------------------------------------------------
def test_world_inputs_sum_exactly_in_any_order():
    g = X.WORLD_GRID
    xs = []
    for rank in range(X.WORLD):
        x, d = X.world_inputs(rank)
        assert x.shape == (X.WORLD_POINTS, 3) and d.shape == (X.WORLD_POINTS, g["n_levels"] * g["n_features"])
        assert x.dtype == F32 and d.dtype == F32
        assert np.array_equal(d * 64, np.round(d * 64)) and float(np.abs(d).max()) <= X.WORLD_MAX_ABS
        assert X.WORLD_POINTS * X.WORLD_MAX_ABS * 64 < 2 ** 24                      # every partial sum is exact in fp32
        assert np.array_equal(x[-X.WORLD_POINTS // 5:][40:], x[:X.WORLD_POINTS // 5][40:])      # repeated points
        xs.append(x)
    assert np.array_equal(xs[0][:40], xs[1][:40]) and np.array_equal(xs[0][:40], xs[2][:40])
    assert not np.array_equal(xs[0][40:], xs[1][40:])


# ---- hm_multi_copy_f32 -----------------------------------------------------------------------------------------------
def test_copy_table_reaches_every_class_tail_and_chunk_edge():
    items = X.COPY_ITEMS
    live = [it for it in items if it[0]]
    classes = {X.copy_class(it) for it in live}
    assert classes == {(True, True), (True, False), (False, True), (False, False)}
    vec = [it for it in live if X.copy_class(it) == (True, True)]
    assert {n % 4 for n, _, _ in vec} == {0, 1, 2, 3}
    assert {1, 3, 4, 8191, 8192, 8193, 8195, 16385} <= {n for n, _, _ in vec}       # around one and two chunks
    assert X.COPY_CHUNK == 8192 and max(n for n, _, _ in live) == 512 * 512 + 3
    zeros = [k for k, it in enumerate(items) if it[0] == 0]
    assert len(zeros) >= 2 and all(0 < k < len(items) - 1 for k in zeros)          # between live items
    assert len(items) <= X.COPY_MAX_ITEMS
    many = X.COPY_MANY
    n_live = sum(1 for it in many if it[0])
    assert n_live == 200 and -(-n_live // X.COPY_MAX_ITEMS) == 3 and len(many) - n_live >= 2
    assert {X.copy_class(it) for it in many if it[0]} == classes
    # a table boundary falls between live items, with empty ones before it
    assert many[5][0] == 0 and all(n <= 13 for n, _, _ in many)


@pytest.mark.parametrize("which", ["COPY_ITEMS", "COPY_MANY"])
def test_copy_layout_and_ref(which):
    items = getattr(X, which)
    starts, size = X.copy_layout(items)
    srcs = X.copy_sources(items)
    flat = X.copy_ref(items, srcs)
    assert flat.size == size and flat.dtype == F32
    covered = np.zeros(size, dtype=bool)
    prev_end = 0
    for (n, so, do), s, src in zip(items, starts, srcs):
        assert src.shape == (n,) and src.dtype == F32 and not bool((src == X.COPY_SENTINEL).any())
        if n == 0:
            assert s is None
            continue
        assert s % 4 == do % 4 and s >= prev_end + 1                               # alignment class, a guard in between
        assert not covered[s:s + n].any()
        covered[s:s + n] = True
        assert np.array_equal(flat[s:s + n], src)
        prev_end = s + n
    assert not covered[0] and size - prev_end >= X.COPY_PAD
    assert bool((flat[~covered] == X.COPY_SENTINEL).all()) and int((~covered).sum()) > sum(1 for it in items if it[0])
