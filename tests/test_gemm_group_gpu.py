"""hm_gemm_f32_group_tn / _det on the lists of tests/gemm_group_cases.py (their walk through group_tn is pinned on CPU
by tests/test_gemm_group_cpu.py), in the default mode (atomics) and under ops.deterministic() (workspace slabs and one
reduce launch per table).

As in tests/test_gemm_paths_gpu.py: integer operands in [-8, 8] keep every partial sum below 2^24 (64 * 7168 plus the
terms of a shared C), so any correct fp32 summation order - k parts, atomics, slabs - gives C0 + A^T B exactly and the
results are compared bit for bit with float64; float operands are held to (K + 2) 2^-24 (|A|^T |B| + |C0|), which holds
for every fp32 order.  A and B are views framed in NaN, every C is a window of ld = N + 3 framed in sentinels that must
survive the call.  The deterministic contracts (same bits on a repeat, in any company, and item order for terms of one
C) are compared bit for bit on randn data."""
import ctypes
import zlib

import pytest
import torch

import gemm_cases as GC
import gemm_group_cases as GG
from test_gemm_paths_gpu import DEV, SENT, Out, _assert_bound, _assert_exact, _bits, _view

pytestmark = pytest.mark.gpu
MODES = pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])


def _ops():
    from hashmodnffbanks_idr_amd import ops
    return ops


def _draw(shape, gen, kind):
    if kind == "int":
        return torch.randint(-8, 9, shape, generator=gen, device=DEV).float()
    return torch.randn(shape, generator=gen, device=DEV)


def _operand(rows, cols, lname, gen, kind, ld=None):
    """a stored [K, M] / [K, N] operand: a NaN-framed view in the named layout, or (ld given) a view of that row stride
    in an uninitialised buffer of which only the view is written"""
    if rows == 0 or cols == 0:
        return torch.empty((rows, cols), device=DEV)
    if ld is not None:
        store = torch.empty(ld * (rows - 1) + cols + 64, device=DEV)
        v = store.as_strided((rows, cols), (ld, 1))
    else:
        _, v = _view(rows, cols, GC.LAYOUTS[lname], float("nan"))
    v.copy_(_draw((rows, cols), gen, kind))
    return v


class Built:
    """the operands and the initial C windows of a list; fresh() hands out new sentinel-framed windows"""

    def __init__(self, case, kind, salt=""):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(zlib.crc32(f"group/{case.name}/{kind}/{salt}".encode()))
        self.case, self.items, self.keys = case, case.items, GG.window_keys(case.items)
        self.A = [_operand(it.K, it.M, it.la, gen, kind, it.lda) for it in self.items]
        self.B = [_operand(it.K, it.N, it.lb, gen, kind) for it in self.items]
        self.c0 = {}
        for it, k in zip(self.items, self.keys):
            if k not in self.c0:
                self.c0[k] = _draw((it.M, it.ctot), gen, kind)
            assert self.c0[k].shape == (it.M, it.ctot)

    def fresh(self):
        """(problems for ops.gemm_group_tn, {window key: Out or plain empty tensor})"""
        wins = {k: Out(*c.shape, c) if c.numel() else c.clone() for k, c in self.c0.items()}
        probs = []
        for i, (it, k) in enumerate(zip(self.items, self.keys)):
            w = wins[k]
            probs.append((self.A[i], self.B[i], (w.v if isinstance(w, Out) else w)[:, it.col0:it.col0 + it.N]))
        return probs, wins

    def one(self, i, window):
        """item i alone, adding into `window` (an Out)"""
        it = self.items[i]
        return [(self.A[i], self.B[i], window.v[:, it.col0:it.col0 + it.N])]

    def product(self, i):
        """(A^T B, |A|^T |B|) of item i in float64"""
        a, b = self.A[i].double(), self.B[i].double()
        return a.t() @ b, a.abs().t() @ b.abs()

    def refs(self):
        """{window key: (C0 + the sum of its items' products, |C0| + the sum of their magnitudes)} in float64"""
        out = {k: [c.double().clone(), c.double().abs()] for k, c in self.c0.items()}
        for i, (it, k) in enumerate(zip(self.items, self.keys)):
            if 0 in (it.M, it.N):
                continue
            v, mag = self.product(i)
            out[k][0][:, it.col0:it.col0 + it.N] += v
            out[k][1][:, it.col0:it.col0 + it.N] += mag
        return out


def _call(probs, det):
    ops = _ops()
    with ops.deterministic(det):
        ops.gemm_group_tn(probs)
    torch.cuda.synchronize()


def _assert_frames(wins, what):
    for k, w in wins.items():
        if isinstance(w, Out):
            assert w.untouched_outside(), f"{what}: written outside the C window {k}"


def _win(w):
    return w.v if isinstance(w, Out) else w


# ---- a. exact on integers ------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("case", GG.CASES, ids=lambda c: c.name)
def test_list_exact_on_integers(case, det):
    b = Built(case, "int")
    probs, wins = b.fresh()
    _call(probs, det)
    refs = b.refs()
    for k, w in wins.items():
        _assert_exact(_win(w), refs[k][0], f"{case.name}: C window {k}")
    _assert_frames(wins, case.name)


# ---- b. the rounding bound on floats -------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("case", [c for c in GG.CASES if GG.is_dense(c)], ids=lambda c: c.name)
def test_list_rounding_bound_on_floats(case, det):
    b = Built(case, "float")
    probs, wins = b.fresh()
    _call(probs, det)
    refs = b.refs()
    for it, k in zip(b.items, b.keys):          # (dense cases: every item has a window of its own)
        if it.M and it.N:
            _assert_bound(_win(wins[k]), refs[k][0], refs[k][1], it.K, f"{case.name}: C window {k}")
    _assert_frames(wins, case.name)


# ---- c. isolation --------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("K", GG.ISOLATION_KS)
def test_non_finite_stays_in_its_row_and_column(K, det):
    """Inf in one column of A (a row of C), NaN in one column of B: every other element of C is exact.  The shapes have
    partial edge tiles, whose lanes past the edge read a clamped column again and compute values nobody stores; the
    marked row / column is the last one for some items, so those lanes carry the non-finite values too.  (What those
    lanes READ cannot reach a stored element - row m of a tile depends on column m of A alone - so no comparison of
    values notices whether the clamp is there: a build without it passes this file.  The clamp keeps the reads
    inside the operand.)"""
    case = GG.GroupCase(f"isolation-K{K}", [GG.item(M, N, K, *GG.lay(i + 1)) for i, (M, N, _, _) in
                                            enumerate(GG.ISOLATION_MN)])
    b = Built(case, "int")
    refs = b.refs()
    for i, (_, _, r, col) in enumerate(GG.ISOLATION_MN):
        b.A[i][1, r] = float("inf")
        b.B[i][K - 2, col] = float("nan")
    probs, wins = b.fresh()
    _call(probs, det)
    for i, (M, N, r, col) in enumerate(GG.ISOLATION_MN):
        c, ref = _win(wins[b.keys[i]]), refs[b.keys[i]][0].float()
        keep = torch.ones(M, N, dtype=torch.bool, device=DEV)
        keep[r, :] = False
        keep[:, col] = False
        bad = keep & (_bits(c) != _bits(ref))
        assert not bool(bad.any()), (f"{case.name} item {i}: {int(bad.sum())} elements outside row {r} / column {col} "
                                     f"differ, first at {tuple(bad.nonzero()[0].tolist())}")
        assert not bool(torch.isfinite(c[r, :]).any()) and not bool(torch.isfinite(c[:, col]).any()), (case.name, i)
    _assert_frames(wins, case.name)


# ---- d. deterministic contracts, bit for bit on randn data ---------------------------------------------------------
def _assert_same_bits(got, want, what):
    g, w = got.view(torch.int32), want.view(torch.int32)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first at {i}: "
                             f"{got[i].item()!r} vs {want[i].item()!r}")


REPEAT = ["every-K", "tabled-and-alone-layouts", "shared-0-2", "column-slices", "n33"]


@pytest.mark.parametrize("name", REPEAT)
def test_deterministic_repeat_gives_the_same_bits(name):
    b = Built(GG.BY_NAME[name], "float")
    runs = []
    for _ in range(2):
        probs, wins = b.fresh()
        _call(probs, True)
        runs.append(wins)
    for k in runs[0]:
        _assert_same_bits(_win(runs[0][k]), _win(runs[1][k]), f"{name}: C window {k}, second call")


@pytest.mark.parametrize("name", ["every-K", "tabled-and-alone", "tabled-and-alone-layouts", "n17", "edge-K3328"])
def test_deterministic_item_in_a_list_equals_the_item_alone(name):
    """the summation order depends on the item's shape, not on its company or its place in a table"""
    b = Built(GG.BY_NAME[name], "float")
    probs, wins = b.fresh()
    _call(probs, True)
    for i, k in enumerate(b.keys):
        alone = Out(*b.c0[k].shape, b.c0[k])
        _call(b.one(i, alone), True)
        _assert_same_bits(_win(wins[k]), alone.v, f"{name}: item {i} {tuple(b.items[i][:3])} in the list vs alone")


@pytest.mark.parametrize("case", GG.ORDER, ids=lambda c: c.name)
def test_deterministic_terms_of_one_output_are_added_in_item_order(case):
    """items of one call that add into the same C give the bits of consecutive one-item calls in item order, whether
    they run from the table or alone (a K that is no multiple of 128)"""
    b = Built(case, "float")
    probs, wins = b.fresh()
    _call(probs, True)
    _, seq = b.fresh()
    for i, k in enumerate(b.keys):
        _call(b.one(i, seq[k]), True)
    for k in wins:
        _assert_same_bits(_win(wins[k]), _win(seq[k]), f"{case.name}: C window {k}, one call vs one call per item")
    # ... and both are the float64 sum within the bound of all terms
    refs = b.refs()
    for k in wins:
        _assert_bound(_win(wins[k]), refs[k][0], refs[k][1], sum(it.K for it in b.items), case.name)


# ---- e. refusals ---------------------------------------------------------------------------------------------------
def _raw_items(probs):
    from hashmodnffbanks_idr_amd import _lib
    arr = (_lib.GemmGroupItem * len(probs))()
    for i, (a, b, c) in enumerate(probs):
        arr[i] = _lib.GemmGroupItem(a.data_ptr(), b.data_ptr(), c.data_ptr(), a.shape[1], b.shape[1], a.shape[0],
                                    a.stride(0), b.stride(0), c.stride(0))
    return arr


def _unchanged(wins, b):
    torch.cuda.synchronize()
    return all(torch.equal(_win(w).view(torch.int32), b.c0[k].view(torch.int32)) for k, w in wins.items())


def test_deterministic_workspace_of_exactly_the_need_and_four_bytes_less():
    """the deterministic entry point with need - 4 bytes refuses and leaves every C alone; with exactly `need` bytes,
    framed in sentinels, it is exact and stays inside them"""
    from hashmodnffbanks_idr_amd import _lib
    lib = _lib.lib()
    case = GG.BY_NAME["every-K"]                          # one table
    b = Built(case, "int")
    probs, wins = b.fresh()
    arr = _raw_items(probs)
    p = ctypes.cast(arr, ctypes.c_void_p)
    need = lib.hm_gemm_f32_group_tn_det_workspace_bytes(p, len(probs))
    assert need == 4 * sum(GG.K_SPLITS[it.K] * it.M * it.N for it in case.items)
    pad = 4096                                            # (floats: more than a slab row stride of ldc would overrun)
    frame = torch.full((need // 4 + 2 * pad,), SENT, device=DEV)
    ws = frame[pad:pad + need // 4]
    stream = _lib.stream_ptr(ws)
    with pytest.raises(ValueError):
        _lib.check(lib.hm_gemm_f32_group_tn_det(p, len(probs), ws.data_ptr(), need - 4, stream))
    with pytest.raises(ValueError):
        _lib.check(lib.hm_gemm_f32_group_tn_det(p, len(probs), None, need, stream))
    assert _unchanged(wins, b)
    assert bool((frame == SENT).all())
    _lib.check(lib.hm_gemm_f32_group_tn_det(p, len(probs), ws.data_ptr(), need, stream))
    torch.cuda.synchronize()
    refs = b.refs()
    for k, w in wins.items():
        _assert_exact(_win(w), refs[k][0], f"C window {k}")
    _assert_frames(wins, case.name)
    assert bool((frame[:pad] == SENT).all()) and bool((frame[pad + need // 4:] == SENT).all())


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
def test_null_operand_and_short_leading_dimension_raise(det):
    from hashmodnffbanks_idr_amd import _lib
    lib = _lib.lib()
    b = Built(GG.GroupCase("refusals", [GG.item(65, 63, 1024), GG.item(33, 20, 1000)]), "int")
    probs, wins = b.fresh()
    ws = torch.empty(1 << 20, device=DEV)
    stream = _lib.stream_ptr(ws)

    def call(arr):
        p = ctypes.cast(arr, ctypes.c_void_p)
        if det:
            return lib.hm_gemm_f32_group_tn_det(p, len(probs), ws.data_ptr(), 4 * ws.numel(), stream)
        return lib.hm_gemm_f32_group_tn(p, len(probs), stream)
    for field, value in (("A", None), ("B", None), ("C", None), ("lda", 64), ("ldb", 62), ("ldc", 62), ("M", -1)):
        arr = _raw_items(probs)
        setattr(arr[0], field, value)
        with pytest.raises(ValueError):
            _lib.check(call(arr))
        assert _unchanged({k: w for k, w in wins.items() if k == b.keys[0]}, b), field
    _lib.check(call(_raw_items(probs)))
    torch.cuda.synchronize()
    refs = b.refs()
    for k, w in wins.items():
        _assert_exact(_win(w), refs[k][0], f"C window {k}")


def test_ops_refuses_a_c_with_a_column_stride():
    ops = _ops()
    a, b = torch.randn(128, 8, device=DEV), torch.randn(128, 6, device=DEV)
    c = torch.zeros(6, 8, device=DEV).t()
    assert c.shape == (8, 6) and c.stride(1) != 1
    for det in (False, True):
        with ops.deterministic(det), pytest.raises(ValueError):
            ops.gemm_group_tn([(a, b, c)])
    torch.cuda.synchronize()
    assert not bool(c.any())
