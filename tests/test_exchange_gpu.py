"""The four gradient-exchange kernels of csrc/hm_exchange.hip through the C ABI, and the host protocol of
parallel.StaticGradExchange as a simulated world of three in one process, against the numpy references of
tests/exchange_cases.py (checked on CPU by tests/test_exchange_cases_cpu.py).  Every comparison is bit-exact (int32
views): these kernels exist to keep replicas bitwise identical, so no test takes a tolerance.  The one bounded comparison
(the world's result against a float64 mean) derives its bound from the fp32 operations it covers.

Branch -> case:
  multi_copy_kernel   float4 body, its e4 tail, numel % 4 = 0 .. 3 with both pointers aligned: COPY_ITEMS numel = 1, 3, 4, 6,
                      8191 .. 8195, 16385 at offsets (0, 0); misaligned source into aligned destination, aligned source into
                      misaligned destination, both misaligned: the (1|2|3, 0), (0, 1|2|3) and (k, m) items; chunk edge 8192:
                      8191 .. 8195 and 16385 on every path; many chunks: 512 * 512 + 3 on both paths
                      -> test_multi_copy_alignment_tails_and_chunk_edges (windows, guard floats, sources)
  hm_multi_copy_f32   numel == 0 skip with NULL pointers between live items: the (0, 0, 0) items of both tables; table
                      splitting at HM_COPY_MAX_ITEMS = 96: 200 live items = three launches
                      -> test_multi_copy_200_items_make_three_tables
  rows_pack_kernel    F = 1, 2, 3, 8; cnt == 0, 1, one block 255 / 256, two blocks 257, cnt == cap = 300 (partial block);
                      atomicAnd of single bits in words shared with claimed-but-unlisted rows, the partial last word
                      (total_rows = 4099, rows 0 and 4098 listed); -0.0, inf, NaN payload, subnormal carried as bits
                      -> test_rows_pack_counts_bits_and_special_values
                      cnt > cap (atomicMax into status: 0 -> 37, 50 stays 50), guard words after payload[cap], the rows
                      beyond cap keep bit and value; status == NULL
                      -> test_rows_pack_overflow
  rows_apply_kernel   row < 0 (-1, -5) and row >= total_rows (total_rows, total_rows + 7) skipped, entries with values;
                      scale = 1, 1/2, 1/3, 1/8 (1/3: two roundings differ from a fused multiply-add); n_lists = 1, 2, 3, 8;
                      rows in every list at different slots / in one list / in none; nonzero accumulator; two tables in
                      one buffer with list_stride > cap * (1 + F), table B at offset capA * 3, slack words after it
                      -> test_rows_apply_lists_scales_and_two_table_layout
  rows_clear_kernel   exactly the named in-range rows of a table that is nonzero everywhere, the same skipped rows, counter
                      5 -> 0; touched_count == NULL; cap == 0 with a counter (the early path: reset, nothing touched)
                      -> test_rows_clear_names_rows_and_resets_the_counter
  HM_CHECK_ARG        F = 0, 9; cap < 0; list_stride < cap * (1 + F); NULL table / list with cap > 0; numel < 0; NULL
                      source with numel > 0 -> test_refusals_leave_the_outputs_untouched
  StaticGradExchange  begin_step / attach / add / pack per rank, the three payloads stacked as the all-gather delivers
                      them, apply at scale 1/3 in rank order, finish; a second round; check() on overflow
                      -> test_simulated_world_of_three, test_check_raises_after_an_overflow
"""
import ctypes as C

import numpy as np
import pytest
import torch

import exchange_cases as X

pytestmark = pytest.mark.gpu

DEV = "cuda"
I32, U32, F32, F64 = X.I32, X.U32, X.F32, X.F64
GUARD_ROWS = 8                       # rows of guard words in front of and behind a dense table


def _L():
    from hashmodnffbanks_idr_amd import _lib
    return _lib


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == U32:
        a = a.view(I32)
    return torch.from_numpy(a.copy()).to(DEV)


def _i32(t):
    """a tensor's bits on the host"""
    t = t.detach().contiguous().cpu()
    return t.numpy().view(I32) if t.dtype == torch.float32 else t.numpy()


def _same_bits(t, ref, what):
    ref = np.ascontiguousarray(ref)
    got = _i32(t)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ok = np.array_equal(got, ref.view(I32))
    assert ok, (what, int((got != ref.view(I32)).sum()), "words differ")


def _at(t, words):
    return C.c_void_p(t.data_ptr() + 4 * words)


def _guarded_table(values):
    """(whole buffer, the [rows, F] table inside it): GUARD_ROWS rows of guard words on both sides, so that a write
    through a skipped row id (-1, -5, total_rows, total_rows + 7) would land in memory the test owns and checks"""
    total, F = values.shape
    whole = torch.full((GUARD_ROWS + total + GUARD_ROWS, F), X.GUARD, dtype=torch.int32, device=DEV).view(torch.float32)
    table = whole[GUARD_ROWS:GUARD_ROWS + total]
    table.copy_(_dev(values))
    assert table.is_contiguous()
    return whole, table


def _guards_intact(whole, what):
    w = whole.view(torch.int32)
    assert bool((w[:GUARD_ROWS] == X.GUARD).all()) and bool((w[-GUARD_ROWS:] == X.GUARD).all()), what


# =====================================================================================================================
# hm_rows_pack
# =====================================================================================================================
N_GUARD = 64


def _pack_run(inp, F, count, status0):
    """one hm_rows_pack call on fresh buffers, compared with pack_ref; returns the device buffers"""
    L = _L()
    cap = X.PACK_CAP
    dense, rows, bits = _dev(inp["dense"]), _dev(inp["rows"]), _dev(inp["bits"])
    cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
    payload = torch.full((cap * (1 + F) + N_GUARD,), X.GUARD, dtype=torch.int32, device=DEV)
    status = None if status0 is None else torch.tensor([status0], dtype=torch.int32, device=DEV)
    L.check(L.lib().hm_rows_pack(L.dptr(dense), F, L.dptr(rows), L.dptr(cnt), cap, L.dptr(bits), L.dptr(payload),
                                 L.dptr(status), L.stream_ptr(dense)))
    torch.cuda.synchronize()
    r_payload, r_dense, r_bits, r_status = X.pack_ref(inp["dense"], inp["rows"], count, cap, inp["bits"], status0)
    what = (F, count, status0)
    _same_bits(payload[:cap * (1 + F)].view(cap, 1 + F), r_payload, ("payload",) + what)
    assert bool((payload[cap * (1 + F):] == X.GUARD).all()), ("guard words after payload[cap]",) + what
    _same_bits(dense, r_dense, ("dense",) + what)
    _same_bits(bits, r_bits, ("bits",) + what)
    _same_bits(rows, inp["rows"], ("rows",) + what)
    assert int(cnt.item()) == count
    if status0 is not None:
        assert int(status.item()) == r_status, ("status",) + what
    return dense, bits


@pytest.mark.parametrize("F", X.PACK_F)
def test_rows_pack_counts_bits_and_special_values(F):
    inp = X.pack_inputs(F)
    for count in X.PACK_COUNTS:
        dense, bits = _pack_run(inp, F, count, 0)
        # spelled out once more, without the reference: the claimed-but-unlisted bits survive, unlisted rows keep their bits
        b = _i32(bits).view(U32)
        for r in inp["extra"].tolist() + inp["rows"][count:].tolist():
            assert (int(b[r >> 5]) >> (r & 31)) & 1, (F, count, r)
        for r in inp["rows"][:count].tolist():
            assert not (int(b[r >> 5]) >> (r & 31)) & 1, (F, count, r)
        keep = np.ones(X.TOTAL_ROWS, dtype=bool)
        keep[inp["rows"][:count]] = False
        assert np.array_equal(_i32(dense)[keep], inp["dense"].view(I32)[keep])
        assert not _i32(dense)[~keep].any()


@pytest.mark.parametrize("F", X.PACK_F)
def test_rows_pack_overflow(F):
    """count = cap + 37: status 0 -> 37, 50 stays 50, NULL is accepted; the first cap rows are packed as usual, nothing
    is written behind payload[cap], and - the state include/hashmod.h documents - the 37 rows claimed beyond cap keep
    their claim bit and their dense value"""
    inp = X.pack_inputs(F)
    cap, count = X.PACK_CAP, X.PACK_CAP + X.PACK_OVER
    for status0 in (0, 50, None):
        dense, bits = _pack_run(inp, F, count, status0)
        b = _i32(bits).view(U32)
        left = inp["rows"][cap:]
        assert left.size == X.PACK_OVER
        assert all((int(b[r >> 5]) >> (r & 31)) & 1 for r in left.tolist())
        assert np.array_equal(_i32(dense)[left], inp["dense"].view(I32)[left]) and _i32(dense)[left].all()


# =====================================================================================================================
# hm_rows_apply
# =====================================================================================================================
def _apply(table, name, buf, n_lists, scale):
    L = _L()
    total, F, cap = X.TABLES[name]
    L.check(L.lib().hm_rows_apply(L.dptr(table), total, F, _at(buf, X.OFFSETS[name]), cap, X.STRIDE, n_lists, scale,
                                  L.stream_ptr(table)))


@pytest.mark.parametrize("scale", X.SCALES, ids=["1", "1/2", "1/3", "1/8"])
@pytest.mark.parametrize("n_lists", X.N_LISTS)
def test_rows_apply_lists_scales_and_two_table_layout(n_lists, scale):
    """both tables of one [n_lists, STRIDE] buffer, each through its own call with the shared stride: the result equals
    apply_ref bit for bit (so neither the other table's words nor the slack - whose words name row 3 with the value 1.0 -
    were read as entries), twice; the buffer and the guard rows around the table are untouched"""
    buf_np = X.lists_buffer(n_lists)
    buf = _dev(buf_np)
    for name, (total, F, cap) in X.TABLES.items():
        acc = X.accumulator(name)
        ref = X.apply_ref(acc, buf_np, cap, X.STRIDE, X.OFFSETS[name], n_lists, scale, total)
        outs = []
        for _ in range(2):
            whole, table = _guarded_table(acc)
            _apply(table, name, buf, n_lists, scale)
            torch.cuda.synchronize()
            _same_bits(table, ref, ("apply", name, n_lists, scale))
            _guards_intact(whole, ("apply", name, n_lists, scale))
            outs.append(table.clone())
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
        assert np.array_equal(_i32(table)[X.SLACK_ROW], acc.view(I32)[X.SLACK_ROW])
    _same_bits(buf, buf_np, "the lists are read-only")


# =====================================================================================================================
# hm_rows_clear
# =====================================================================================================================
def _clear(table, name, buf, n_lists, count, cap=None):
    L = _L()
    total, F, cap0 = X.TABLES[name]
    L.check(L.lib().hm_rows_clear(L.dptr(table), total, F, _at(buf, X.OFFSETS[name]), cap0 if cap is None else cap,
                                  X.STRIDE, n_lists, L.dptr(count), L.stream_ptr(table)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("n_lists", X.N_LISTS)
def test_rows_clear_names_rows_and_resets_the_counter(n_lists):
    buf_np = X.lists_buffer(n_lists)
    buf = _dev(buf_np)
    for name, (total, F, cap) in X.TABLES.items():
        acc = X.accumulator(name)
        ref, ref_count = X.clear_ref(acc, buf_np, cap, X.STRIDE, X.OFFSETS[name], n_lists, total, count=5)
        # with a counter
        whole, table = _guarded_table(acc)
        count = torch.tensor([5], dtype=torch.int32, device=DEV)
        _clear(table, name, buf, n_lists, count)
        _same_bits(table, ref, ("clear", name, n_lists))
        _guards_intact(whole, ("clear", name, n_lists))
        assert int(count.item()) == ref_count == 0
        named = np.zeros(total, dtype=bool)
        for rows in X.in_range_rows(X.list_segment(name, n_lists), total):
            named[rows] = True
        got = _i32(table)
        assert not got[named].any() and np.array_equal(got[~named], acc.view(I32)[~named]) and got[~named].all()
        # touched_count == NULL
        whole, table = _guarded_table(acc)
        _clear(table, name, buf, n_lists, None)
        _same_bits(table, ref, ("clear, no counter", name, n_lists))
        _guards_intact(whole, ("clear, no counter", name, n_lists))
        # cap == 0 and a counter: the counter is reset, the table is not touched
        whole, table = _guarded_table(acc)
        count = torch.tensor([5], dtype=torch.int32, device=DEV)
        _clear(table, name, buf, n_lists, count, cap=0)
        _same_bits(table, acc, ("clear, cap 0", name, n_lists))
        _guards_intact(whole, ("clear, cap 0", name, n_lists))
        assert int(count.item()) == 0
    _same_bits(buf, buf_np, "the lists are read-only")


# =====================================================================================================================
# hm_multi_copy_f32
# =====================================================================================================================
def _copy_run(items):
    L = _L()
    srcs = X.copy_sources(items)
    starts, size = X.copy_layout(items)
    flat = torch.full((size,), float(X.COPY_SENTINEL), dtype=torch.float32, device=DEV)
    assert flat.data_ptr() % 16 == 0
    arr = (L.CopyItem * len(items))()
    bufs, befores = [], []
    for k, ((n, so, do), s, src) in enumerate(zip(items, starts, srcs)):
        if n == 0:
            arr[k] = L.CopyItem(None, None, 0)
            continue
        b = torch.full((so + n + X.COPY_PAD,), float(X.COPY_SRC_PAD), dtype=torch.float32, device=DEV)
        b[so:so + n] = _dev(src)
        assert b.data_ptr() % 16 == 0
        arr[k] = L.CopyItem(b.data_ptr() + 4 * so, flat.data_ptr() + 4 * s, n)
        assert ((arr[k].src % 16 == 0), (arr[k].dst % 16 == 0)) == X.copy_class((n, so, do))
        bufs.append(b)
        befores.append(b.clone())
    L.check(L.lib().hm_multi_copy_f32(C.cast(arr, C.c_void_p), len(items), L.stream_ptr(flat)))
    torch.cuda.synchronize()
    ref = X.copy_ref(items, srcs)
    got = _i32(flat)
    for (n, so, do), s in zip(items, starts):                     # window by window first: names the item that failed
        if n:
            assert np.array_equal(got[s:s + n], ref.view(I32)[s:s + n]), ("window", n, so, do)
    _same_bits(flat, ref, "windows and guard floats")
    for b, b0 in zip(bufs, befores):
        assert torch.equal(b.view(torch.int32), b0.view(torch.int32)), "a source changed"


def test_multi_copy_alignment_tails_and_chunk_edges():
    _copy_run(X.COPY_ITEMS)


def test_multi_copy_200_items_make_three_tables():
    _copy_run(X.COPY_MANY)


# =====================================================================================================================
# refusals
# =====================================================================================================================
def test_refusals_leave_the_outputs_untouched():
    L = _L()
    lib = L.lib()
    total, F, cap, n_lists = 64, 2, 8, 2
    stride = cap * (1 + F)
    mk = lambda n, v: torch.full((n,), v, dtype=torch.int32, device=DEV)
    table = torch.full((total, 8), 1.5, dtype=torch.float32, device=DEV)          # wide enough for any F handed over
    rows = torch.arange(cap, dtype=torch.int32, device=DEV)
    count, bits = mk(1, cap), mk((total + 31) // 32, -1)
    payload, status, counter = mk(cap * 10, X.GUARD), mk(1, 0), mk(1, 5)
    lists = torch.zeros((n_lists, cap * 10), dtype=torch.int32, device=DEV)
    lists[:, 0:stride:1 + F] = torch.arange(cap, dtype=torch.int32, device=DEV)   # F = 2: row = slot, values +0.0
    src = torch.full((16,), 2.5, dtype=torch.float32, device=DEV)
    dst = torch.full((16,), float(X.COPY_SENTINEL), dtype=torch.float32, device=DEV)
    outs = [table, bits, payload, status, counter, dst, count, rows, lists, src]
    before = [t.clone() for t in outs]
    st = L.stream_ptr(table)
    p, null = L.dptr, C.c_void_p(0)

    def pack(F=F, cap=cap, table=p(table), rows=p(rows), bits=p(bits), payload=p(payload)):
        return lib.hm_rows_pack(table, F, rows, p(count), cap, bits, payload, p(status), st)

    def apply(F=F, cap=cap, stride=stride, table=p(table), lists=p(lists)):
        return lib.hm_rows_apply(table, total, F, lists, cap, stride, n_lists, 0.5, st)

    def clear(F=F, cap=cap, stride=stride, table=p(table), lists=p(lists)):
        return lib.hm_rows_clear(table, total, F, lists, cap, stride, n_lists, p(counter), st)

    def copy(*items):
        arr = (L.CopyItem * len(items))(*[L.CopyItem(*it) for it in items])
        return lib.hm_multi_copy_f32(C.cast(arr, C.c_void_p), len(items), st)

    good = (src.data_ptr(), dst.data_ptr(), 4)
    cases = {
        "pack F = 0": lambda: pack(F=0), "pack F = 9": lambda: pack(F=9), "pack cap < 0": lambda: pack(cap=-1),
        "pack NULL table": lambda: pack(table=null), "pack NULL list": lambda: pack(rows=null),
        "pack NULL bits": lambda: pack(bits=null), "pack NULL payload": lambda: pack(payload=null),
        "apply F = 0": lambda: apply(F=0), "apply F = 9": lambda: apply(F=9), "apply cap < 0": lambda: apply(cap=-1),
        "apply short stride": lambda: apply(stride=stride - 1), "apply NULL table": lambda: apply(table=null),
        "apply NULL list": lambda: apply(lists=null),
        "clear F = 0": lambda: clear(F=0), "clear F = 9": lambda: clear(F=9), "clear cap < 0": lambda: clear(cap=-1),
        "clear short stride": lambda: clear(stride=stride - 1), "clear NULL table": lambda: clear(table=null),
        "clear NULL list": lambda: clear(lists=null),
        # a good item first: an item is refused before ANY item is copied
        "copy numel < 0": lambda: copy(good, (src.data_ptr() + 16, dst.data_ptr() + 32, -1)),
        "copy NULL source": lambda: copy(good, (None, dst.data_ptr() + 32, 4)),
        "copy NULL destination": lambda: copy(good, (src.data_ptr() + 16, None, 4)),
        "copy NULL items": lambda: lib.hm_multi_copy_f32(null, 2, st),
        "copy n_items < 0": lambda: lib.hm_multi_copy_f32(null, -1, st),
    }
    for name, call in cases.items():
        with pytest.raises(L.HashmodArgumentError):
            L.check(call())
            pytest.fail(f"{name}: accepted")
        torch.cuda.synchronize()
        for t, t0 in zip(outs, before):
            assert torch.equal(t.view(torch.int32), t0.view(torch.int32)), (name, "a buffer changed")
    # the same calls with good arguments are accepted (so each refusal above is about the one argument it names)
    for call in (pack, apply, clear, lambda: copy(good)):
        L.check(call())
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and int(counter.item()) == 0 and bool((dst[:4] == 2.5).all())
    assert bool((dst[4:] == float(X.COPY_SENTINEL)).all())


# =====================================================================================================================
# the host protocol: a simulated world of three in one process
# =====================================================================================================================
def _make_world(n):
    from hashmodnffbanks_idr_amd import parallel
    from hashmodnffbanks_idr_amd.model.embeddings.hashGridEmbedding import MultiResHashGridMLP
    assert not torch.distributed.is_initialized()
    g = X.WORLD_GRID
    embs, exs = [], []
    for _ in range(n):
        torch.manual_seed(0)
        emb = MultiResHashGridMLP(True, 3, g["n_levels"], g["n_features"], g["log2_hashmap_size"], g["base_resolution"],
                                  g["desired_resolution"]).to(DEV)
        assert emb.frac_mode == "reference" and 2000 < emb.desc.total_rows < 8192
        embs.append(emb)
        exs.append(parallel.StaticGradExchange([], tables=[emb]))
    return embs, exs


def _rank_step(ex, rank):
    """what one rank does up to the all-gather; returns its payload"""
    x, d = (torch.from_numpy(a).to(DEV) for a in X.world_inputs(rank))
    ex.begin_step()
    ex.attach()
    ex.tables[0].add(x, d)
    ex.pack()
    return ex.payload.clone()


def _all_zero(t):
    return (int(torch.count_nonzero(t.dense.view(torch.int32))) == 0 and int(torch.count_nonzero(t.bits)) == 0
            and int(t.count.item()) == 0)


def test_simulated_world_of_three():
    from hashmodnffbanks_idr_amd import ops
    embs, exs = _make_world(X.WORLD)
    t0 = exs[0].tables[0]
    total, F = t0.total_rows, t0.F
    # every rank's dense gradient by the plain scatter (the sums are exact: world_inputs), shared by both rounds
    grads = []
    for rank in range(X.WORLD):
        x, d = (torch.from_numpy(a).to(DEV) for a in X.world_inputs(rank))
        grads.append(ops.encode_bwd_table(embs[rank].desc, x, d, 0).cpu().numpy())
    mean64 = sum(g.astype(F64) for g in grads) / X.WORLD
    mag64 = sum(np.abs(g.astype(F64)) for g in grads) / X.WORLD
    results = []
    for rnd in range(2):
        payloads = [_rank_step(ex, rank) for rank, ex in enumerate(exs)]
        cap, stride = t0.cap, exs[0].stride
        assert cap == X.WORLD_POINTS * embs[0].n_levels <= 2048 and stride == cap * (1 + F)
        assert all(ex.stride == stride and ex.offs == [0] for ex in exs)
        for rank, (ex, pl) in enumerate(zip(exs, payloads)):
            t = ex.tables[0]
            ex.check()                                                            # nothing overflowed
            assert int(torch.count_nonzero(t.dense.view(torch.int32))) == 0 and int(torch.count_nonzero(t.bits)) == 0
            e = pl.cpu().numpy().reshape(cap, 1 + F)
            n = int(t.count.item())
            rows = e[:n, 0]
            assert 0 < n <= cap and np.unique(rows).size == n and rows.min() >= 0 and rows.max() < total
            assert bool((e[n:, 0] == -1).all()) and not e[n:, 1:].any()
            assert np.array_equal(e[:n, 1:], grads[rank].view(I32)[rows])         # the rank's own sums, bit for bit
            rest = np.ones(total, dtype=bool)
            rest[rows] = False
            assert not grads[rank][rest].any()                                    # and no touched row is missing
        gathered = torch.stack(payloads)                                          # what the all-gather would deliver
        assert gathered.shape == (X.WORLD, stride)
        exs[0].gathered = gathered
        exs[0].apply()
        torch.cuda.synchronize()
        ref = X.apply_ref(np.zeros((total, F), dtype=F32), gathered.cpu().numpy(), cap, stride, 0, X.WORLD, 1.0 / X.WORLD,
                          total)
        _same_bits(t0.dense, ref, ("apply in rank order at 1/3, round", rnd))
        assert embs[0].table.grad.data_ptr() == t0.dense.data_ptr()
        # against the float64 mean: fl(1/3), one product and at most two effective additions per term (the first lands
        # on +0.0) are four roundings of relative size u; 5 u covers their second-order terms
        got = t0.dense.cpu().numpy()
        err = np.abs(got.astype(F64) - mean64)
        print(f"    round {rnd}: max error against the float64 mean {err.max():.3e}, "
              f"largest error / (u * mean magnitude) {np.max(err / np.maximum(X.U * mag64, 1e-300)):.2f} (limit 5)")
        assert bool((err <= 5 * X.U * mag64).all())
        assert int((mag64 > 0).sum()) > 500
        results.append(got.view(I32).copy())
        for ex in exs:                                                            # (ranks 1, 2: their own list only)
            ex.finish()
        torch.cuda.synchronize()
        assert all(_all_zero(ex.tables[0]) for ex in exs)
    assert np.array_equal(results[0], results[1])
    in_several = sum((g != 0).any(1).astype(int) for g in grads)
    assert int((in_several >= 2).sum()) > 20 and int((in_several == 1).sum()) > 20     # the payloads overlap, partly


def test_check_raises_after_an_overflow():
    """a table whose cap is 37 below its claimed row count: check() raises and says what is left behind, and what is left
    behind is what include/hashmod.h documents - 37 claim bits, and the counter still above the cap"""
    embs, exs = _make_world(1)
    ex, t = exs[0], exs[0].tables[0]
    _rank_step(ex, 0)
    ex.apply()
    ex.finish()
    ex.check()
    assert _all_zero(t)
    ex.begin_step()
    ex.attach()
    x, d = (torch.from_numpy(a).to(DEV) for a in X.world_inputs(0))
    t.add(x, d)
    claimed = int(t.count.item())
    full_cap = t.cap
    assert claimed > 100
    t.cap = claimed - 37                                                          # before pack(): the layout is kept
    ex.pack()
    assert ex.stride == full_cap * (1 + t.F)
    with pytest.raises(RuntimeError, match=r"TouchedRowExchange: 37 touched rows did not fit.*claim bit.*rebuild"):
        ex.check()
    bits = t.bits.cpu().numpy().view(U32)
    assert sum(bin(int(w)).count("1") for w in bits) == 37
    left = np.nonzero((t.dense.cpu().numpy() != 0).any(1))[0]
    assert 0 < left.size <= 37 and all((int(bits[r >> 5]) >> (r & 31)) & 1 for r in left.tolist())
