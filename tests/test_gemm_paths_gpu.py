"""hm_gemm_f32 / _ep / _det on every kernel it can launch (tests/gemm_cases.py; the routes are pinned on CPU by
tests/test_gemm_plan_cpu.py and asserted again here with the real addresses).

Integer operands in [-8, 8] keep every partial sum below 2^24, so any correct fp32 GEMM - whatever its summation
order, split-K and atomics included - returns the exact product: results are compared bit for bit with float64 (the
sign of a zero aside).  Float operands are held to the elementwise bound (K + 2) 2^-24 (|op(A)| |op(B)| + |bias|
(+ |C0|)), which holds for every summation order in fp32 and fails for any reduced-precision path.  Operand views
are surrounded by NaN, outputs by sentinels that must survive the call."""
import zlib

import pytest
import torch

import gemm_cases as GC

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -1234.5          # output sentinel
BETA, THR = 100.0, 20.0


def _ops():
    from hashmodnffbanks_idr_amd import ops
    return ops


def _gen(case, salt=0):
    g = torch.Generator(device=DEV)
    g.manual_seed(zlib.crc32(f"{case.name}/{salt}".encode()))
    return g


def _draw(shape, gen, kind):
    if kind == "int":
        return torch.randint(-8, 9, shape, generator=gen, device=DEV).float()
    return torch.randn(shape, generator=gen, device=DEV)


def _view(rows, cols, lay, fill):
    """[rows, cols] view with row stride cols + lay.pad, starting lay.off floats past a 16-byte boundary, inside a
    buffer of `fill` with a row before and a row after it; returns (buffer, view)"""
    ld = cols + lay.pad
    lead = ((ld + 3) // 4) * 4 + lay.off
    buf = torch.full((lead + (rows + 1) * ld + 4,), fill, device=DEV)
    v = buf.as_strided((rows, cols), (ld, 1), lead)
    assert v.data_ptr() % 16 == 4 * lay.off
    return buf, v


def _operand(case, which, gen, kind):
    rows, cols = GC.stored_shape(case, which)
    _, v = _view(rows, cols, case.la if which == "A" else case.lb, float("nan"))
    v.copy_(_draw((rows, cols), gen, kind))
    return v


def _op(x, t):
    return x.t() if t else x


class Out:
    """an output window of ld = cols + 3 in a sentinel-filled buffer; `inside` starts as `init`"""

    def __init__(self, rows, cols, init):
        self.buf, self.v = _view(rows, cols, GC.Layout(3, 0), SENT)
        self.v.copy_(init)
        self.inside = torch.zeros_like(self.buf, dtype=torch.bool)
        self.inside.as_strided((rows, cols), self.v.stride(), self.v.storage_offset()).fill_(True)

    def untouched_outside(self):
        out = self.buf[~self.inside]
        return bool((out.view(torch.int32) == torch.tensor([SENT], device=DEV).view(torch.int32)).all())


def _bits(x):
    return (x.float() + 0.0).view(torch.int32)      # (+0.0: -0 -> +0)


def _assert_exact(got, ref, what):
    ref = ref.float()
    if not torch.equal(_bits(got), _bits(ref)):
        bad = (_bits(got) != _bits(ref)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first at {i}: "
                             f"{got[i].item()!r} vs {ref[i].item()!r}")


def _assert_bound(got, ref64, mag64, K, what):
    tol = (K + 2) * 2.0 ** -24 * mag64
    err = (got.double() - ref64).abs()
    assert bool((err <= tol).all()), f"{what}: |C - C64| exceeds the fp32 bound by {(err - tol).max().item():.3e}"


def _run(case, A, B, bias, init, ep_ops=None, scale=1.0):
    """one call on the case's route; returns (C window, out1 window or None)"""
    ops = _ops()
    M, N = case.M, case.N
    if case.ep is None:
        c = Out(M, N, init)
        with ops.deterministic(case.det):
            r = ops.gemm(A, B, bias, bool(case.ta), bool(case.tb), out=c.v, accumulate=case.acc)
        assert r.data_ptr() == c.v.data_ptr()
        return c, None
    z, g, nz = ep_ops
    mode = ops.EPI_RELU if case.ep == "relu" else ops.EPI_RELUMASK
    o1 = Out(M, nz if mode == ops.EPI_RELUMASK else N, float("nan"))
    cv, r1 = ops.gemm_ep(A, B, bias, bool(case.ta), bool(case.tb), mode, BETA, THR, scale=scale, z=z, g=g, nz=nz,
                         out1=o1.v)
    assert r1.data_ptr() == o1.v.data_ptr()
    return cv, o1


def _ep_operands(case, gen, kind):
    if case.ep != "relumask":
        return None, None, None
    nz = max(1, case.N - 5)
    _, z = _view(case.M, case.N + 2, GC.Layout(1, 0), float("nan"))
    z.copy_(_draw(z.shape, gen, "int"))                  # the sign pattern of a ReLU output (zeros included)
    _, g = _view(case.M, nz, GC.Layout(2, 1), float("nan"))
    g.copy_(_draw(g.shape, gen, kind))
    return z, g, nz


def _check_case(case, kind):
    gen = _gen(case, kind)
    A, B = _operand(case, "A", gen, kind), _operand(case, "B", gen, kind)
    GC.check_route(case, GC.plan(case, A.data_ptr(), B.data_ptr()))
    bias = _draw((case.N,), gen, kind) if case.bias else None
    c0 = _draw((case.M, case.N), gen, kind) if case.acc else torch.full((case.M, case.N), float("nan"), device=DEV)
    z, g, nz = _ep_operands(case, gen, kind)
    c, o1 = _run(case, A, B, bias, c0, (z, g, nz))
    torch.cuda.synchronize()
    opA, opB = _op(A, case.ta).double(), _op(B, case.tb).double()
    v = opA @ opB
    mag = opA.abs() @ opB.abs()
    if bias is not None:
        v = v + bias.double()
        mag = mag + bias.double().abs()
    if case.acc:
        v = v + c0.double()
        mag = mag + c0.double().abs()
    cw = c.v if case.ep is None else c
    if kind == "int":
        _assert_exact(cw, v, f"{case.name}: C")
    else:
        _assert_bound(cw, v, mag, case.K, f"{case.name}: C")
    if case.ep is None:
        assert c.untouched_outside(), f"{case.name}: C written outside its window"
        return
    assert o1.untouched_outside(), f"{case.name}: out1 written outside its window"
    ref1 = v.clamp(min=0) if case.ep == "relu" else torch.where(z[:, :nz] > 0, v[:, :nz], 0.0) + g.double()
    if kind == "int":
        _assert_exact(o1.v, ref1, f"{case.name}: out1")
    else:   # the epilogue adds one rounding of its own (+ g)
        m1 = mag if case.ep == "relu" else mag[:, :nz] + g.double().abs()
        _assert_bound(o1.v, ref1, m1, case.K + 1, f"{case.name}: out1")


@pytest.mark.parametrize("case", GC.ROUTES, ids=lambda c: c.name)
def test_route_exact_on_integers(case):
    _check_case(case, "int")


@pytest.mark.parametrize("case", [c for c in GC.ROUTES if c.la == GC.DENSE], ids=lambda c: c.name)
def test_route_rounding_bound_on_floats(case):
    _check_case(case, "float")


@pytest.mark.parametrize("case", GC.EDGE_MN + GC.EDGE_K + GC.EDGE_BIG, ids=lambda c: c.name)
def test_edge_shapes_exact(case):
    _check_case(case, "int")


def run_isolation(case, plan=True):
    """Inf in one row of op(A), NaN in one column of op(B): only that row and column of C may be non-finite, every
    other element is exact.  (The pipelined kernel's K tail used to read the k-contiguous operand's next row or pad
    columns past K and multiply them by 0: a non-finite value there poisoned a whole row of C.)"""
    ops = _ops()
    gen = _gen(case)
    A, B = _operand(case, "A", gen, "int"), _operand(case, "B", gen, "int")
    if plan:
        GC.check_route(case, GC.plan(case, A.data_ptr(), B.data_ptr()))
    ref = (_op(A, case.ta).double() @ _op(B, case.tb).double()).float()
    r, col = case.M // 2 + 1, case.N // 2 + 1
    if case.ta:
        A[1, r] = float("inf")
    else:
        A[r, 1] = float("inf")
    if case.tb:
        B[col, 2] = float("nan")
    else:
        B[2, col] = float("nan")
    c = ops.gemm(A, B, None, bool(case.ta), bool(case.tb))
    keep = torch.ones(case.M, case.N, dtype=torch.bool, device=DEV)
    keep[r, :] = False
    keep[:, col] = False
    bad = keep & (_bits(c) != _bits(ref))
    n = int(bad.sum())
    if n:
        rows = sorted(set(bad.nonzero()[:, 0].tolist()))
        raise AssertionError(f"{case.name}: {n} elements outside row {r} / column {col} differ (rows {rows[:8]}...)")
    assert not bool(torch.isfinite(c[r, col])), case.name


@pytest.mark.parametrize("case", GC.ISOLATION, ids=lambda c: c.name)
def test_non_finite_stays_in_its_row_and_column(case):
    run_isolation(case)


@pytest.mark.parametrize("case", GC.K0, ids=lambda c: c.name)
def test_k0_gives_bias(case):
    """K = 0: C = bias (or zeros), C += bias with accumulate, v = bias * scale in the epilogue - without touching the
    (empty, possibly NULL) operands"""
    ops = _ops()
    M, N = case.M, case.N
    A = torch.empty(GC.stored_shape(case, "A"), device=DEV)
    B = torch.empty(GC.stored_shape(case, "B"), device=DEV)
    GC.check_route(case, GC.plan(case, A.data_ptr(), B.data_ptr()))
    gen = _gen(case)
    bias = _draw((N,), gen, "int")
    ta, tb = bool(case.ta), bool(case.tb)
    _assert_exact(ops.gemm(A, B, bias, ta, tb), bias.expand(M, N), "C = bias")
    _assert_exact(ops.gemm(A, B, None, ta, tb), torch.zeros(M, N, device=DEV), "C = 0")
    c0 = _draw((M, N), gen, "int")
    c = Out(M, N, c0)
    ops.gemm(A, B, bias, ta, tb, out=c.v, accumulate=True)
    _assert_exact(c.v, c0 + bias, "C += bias")
    assert c.untouched_outside()
    with ops.deterministic(True):
        c = Out(M, N, c0)
        ops.gemm(A, B, None, ta, tb, out=c.v, accumulate=True)
        _assert_exact(c.v, c0, "C += 0 (deterministic)")
    sc = 0.7071067811865476
    o1 = Out(M, N, float("nan"))
    cv, _ = ops.gemm_ep(A, B, bias, ta, tb, ops.EPI_RELU, BETA, THR, scale=sc, out1=o1.v)
    v = bias.expand(M, N) * torch.tensor(sc, dtype=torch.float32, device=DEV)
    _assert_exact(cv, v, "epilogue C = bias * scale")
    _assert_exact(o1.v, v.clamp(min=0), "epilogue out1 = relu(bias * scale)")
    assert o1.untouched_outside()


def test_empty_m_or_n_launches_nothing():
    ops = _ops()
    for (M, N, K) in ((0, 5, 7), (5, 0, 7), (0, 0, 0)):
        case = GC._case("e", 0, 0, M, N, K, GC.GENERIC)
        a, b = torch.randn(M, K, device=DEV), torch.randn(K, N, device=DEV)
        info = GC.plan(case, a.data_ptr(), b.data_ptr())
        assert info.kernel == 0
        assert ops.gemm(a, b, torch.randn(N, device=DEV)).shape == (M, N)
        out = torch.empty(M, N, device=DEV)
        assert ops.gemm(a, b, None, out=out, accumulate=True) is out


@pytest.mark.parametrize("case", GC.SUBNORMAL, ids=lambda c: c.name)
def test_subnormal_operands_exact(case):
    """A = integers x 2^-140 (subnormal in fp32), B = integers x 2^100: products are normal and exact, so a
    flush-to-zero build would show"""
    ops = _ops()
    gen = _gen(case)
    A, B = _operand(case, "A", gen, "int"), _operand(case, "B", gen, "int")
    A.mul_(2.0 ** -140)
    B.mul_(2.0 ** 100)
    assert bool(((A != 0) & (A.abs() < 2.0 ** -126)).any())
    GC.check_route(case, GC.plan(case, A.data_ptr(), B.data_ptr()))
    c = ops.gemm(A, B, None, bool(case.ta), bool(case.tb))
    ref = _op(A, case.ta).double() @ _op(B, case.tb).double()
    assert bool((ref != 0).any())
    _assert_exact(c, ref, case.name)


@pytest.mark.parametrize("case", GC.EPILOGUE, ids=lambda c: c.name)
def test_epilogue_raw_outputs_exact(case):
    """every epilogue's raw output v = (sum + bias) * scale is the exact sum rounded once by the fp32 scale; the
    ReLU / ReLU-mask outputs are exact (nz < N, the g addend, want_c=False)"""
    ops = _ops()
    gen = _gen(case)
    A, B = _operand(case, "A", gen, "int"), _operand(case, "B", gen, "int")
    GC.check_route(case, GC.plan(case, A.data_ptr(), B.data_ptr()))
    bias = _draw((case.N,), gen, "int")
    ta, tb = bool(case.ta), bool(case.tb)
    sc = 0.7071067811865476
    exact = _op(A, ta).double() @ _op(B, tb).double() + bias.double()
    v = exact.float() * torch.tensor(sc, dtype=torch.float32, device=DEV)
    z = _draw((case.M, case.N), gen, "int")
    g = _draw((case.M, case.N), gen, "int")
    for mode in (ops.EPI_SOFTPLUS, ops.EPI_S1MUL, ops.EPI_RELU, ops.EPI_RELUMASK):
        kw = dict(z=z, g=g) if mode in (ops.EPI_S1MUL, ops.EPI_RELUMASK) else {}
        c, _ = ops.gemm_ep(A, B, bias, ta, tb, mode, BETA, THR, scale=sc, **kw)
        _assert_exact(c, v, f"{case.name}: raw output of mode {mode}")
    nz = case.N - 7
    c, o = ops.gemm_ep(A, B, bias, ta, tb, ops.EPI_RELUMASK, BETA, THR, scale=sc, z=z, g=g, nz=nz, want_c=False)
    assert c is None and o.shape == (case.M, nz)
    _assert_exact(o, torch.where(z[:, :nz] > 0, v[:, :nz], 0.0) + g[:, :nz], "relumask with nz < N and g")
    c, o = ops.gemm_ep(A, B, bias, ta, tb, ops.EPI_RELU, BETA, THR, scale=sc, want_c=False)
    _assert_exact(o, v.clamp(min=0), "relu without C")


@pytest.mark.parametrize("case", GC.EPILOGUE, ids=lambda c: c.name)
def test_adjoint_windows(case):
    """out1 / out3 of ADJOINT as row-strided windows: values against float64, sentinels around them untouched"""
    ops = _ops()
    gen = _gen(case)
    A, B = _operand(case, "A", gen, "float"), _operand(case, "B", gen, "float")
    ta, tb = bool(case.ta), bool(case.tb)
    z = _draw((case.M, case.N), gen, "float") * 0.05
    g = _draw((case.M, case.N), gen, "float")
    o1, o3 = Out(case.M, case.N, float("nan")), Out(case.M, case.N, float("nan"))
    r1, r2, r3 = ops.gemm_ep(A, B, None, ta, tb, ops.EPI_ADJOINT, BETA, THR, z=z, g=g, out1=o1.v, out3=o3.v)
    assert r1.data_ptr() == o1.v.data_ptr() and r3.data_ptr() == o3.v.data_ptr()
    assert o1.untouched_outside() and o3.untouched_outside()
    opA, opB = _op(A, ta).double(), _op(B, tb).double()
    v, mag = opA @ opB, opA.abs() @ opB.abs()
    bz = z.double() * BETA
    e = torch.exp(torch.clamp(bz, max=80.0))
    s1 = torch.where(bz > THR, torch.ones_like(bz), e / (e + 1))
    # (the fp32 s1 = e / (e + 1) carries a few ulps of its own: 2^-16 relative is a loose allowance for it)
    err1 = (o1.v.double() - v * s1).abs()
    assert bool((err1 <= (case.K + 2) * 2.0 ** -24 * mag * s1 + 2.0 ** -16 * (v * s1).abs()).all()), "adjoint out1"
    assert bool(((o3.v.double() - g.double() * s1).abs() <= 2.0 ** -16 * (g.double() * s1).abs()).all()), "adjoint out3"
    assert bool(torch.isfinite(r2).all())


def test_m1_epilogue_operand_with_unit_row_stride():
    """an M = 1 epilogue operand whose row stride torch reports as 1 (x[:, None].t()) is a valid [1, N] row"""
    ops = _ops()
    g0 = torch.Generator(device=DEV)
    g0.manual_seed(3)
    N, K = 200, 96
    a = _draw((1, K), g0, "int")
    w = _draw((N, K), g0, "int")
    z = _draw((N,), g0, "int")[:, None].t()
    g = _draw((N,), g0, "int")[:, None].t()
    assert z.shape == (1, N) and z.stride(0) == 1
    o1 = _draw((N,), g0, "int")[:, None].t()
    c, o = ops.gemm_ep(a, w, None, False, True, ops.EPI_RELUMASK, BETA, THR, z=z, g=g, out1=o1)
    v = a.double() @ w.double().t()
    _assert_exact(c, v, "M = 1: C")
    _assert_exact(o, torch.where(z > 0, v, 0.0) + g.double(), "M = 1: out1")


def test_bad_arguments_raise_before_launch():
    ops = _ops()
    a, b = torch.randn(70, 40, device=DEV), torch.randn(40, 30, device=DEV)
    good = torch.full((70, 30), 7.0, device=DEV)
    bads = [torch.empty(69, 30, device=DEV), torch.empty(70, 31, device=DEV),
            torch.empty(70, 30, device=DEV, dtype=torch.float64), torch.empty(30, 70, device=DEV).t()]
    torch.cuda.synchronize()
    for out in bads:
        keep = out.clone()
        with pytest.raises(ValueError):
            ops.gemm(a, b, None, out=out)
        with pytest.raises(ValueError):
            ops.gemm(a, b, None, out=out, accumulate=True)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32) if out.dtype == torch.float32 else out.view(torch.int64),
                           keep.view(torch.int32) if out.dtype == torch.float32 else keep.view(torch.int64))
    with pytest.raises(ValueError):
        ops.gemm(a, b, torch.randn(29, device=DEV), out=good)                # short bias
    with pytest.raises(ValueError):
        ops.gemm(a, b, torch.randn(30, device=DEV, dtype=torch.float64), out=good)
    with pytest.raises(ValueError):
        ops.gemm(a, b, None, accumulate=True)                                  # accumulate into nothing
    with pytest.raises(ValueError):
        ops.gemm_ep(a, b.t().contiguous(), torch.randn(29, device=DEV), False, True, ops.EPI_RELU, BETA, THR)
    with pytest.raises(ValueError):
        ops.gemm_ep(a, b.t().contiguous(), None, False, True, ops.EPI_RELU, BETA, THR, out1=bads[3])
    torch.cuda.synchronize()
    assert bool((good == 7.0).all())
