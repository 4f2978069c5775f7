"""The tail of the pipelined GEMM kernels (csrc/hm_gemm.hip, gemm_pipe2_body): the two wave groups exchange halves of
their partial tiles and BOTH run the epilogue, and outputs / epilogue operands go as 16-byte accesses when every base
and row stride allows it, as dwords otherwise.

Integer operands in [-8, 8] keep every partial sum below 2^24, so the fp32 result is exact in any summation order and
is compared bit for bit with float64 (the sign of a zero aside).  The Softplus epilogues are made exact the same way:
beta = 100, threshold = 20 and z in {0, 1, 2} give s1 in {1/2, 1} and s2 in {25, 0} without rounding (exp2(0) = 1,
rcp(2) = 1/2), and softplus(v) of an integer v is v (v >= 1) or 0 (v <= -1, the logarithm term underflows); only
softplus(0) = ln 2 / beta goes through the hardware logarithm, and is held to the 2e-9 that csrc/hm_common.h documents
for that term, with one bit pattern for all of them."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BETA, THR = 100.0, 20.0
GUARD = 64              # floats of guard band before and after every destination
PIPE64, PIPE96 = 3, 4   # hm_gemm_plan_info.kernel (include/hashmod.h)
SOFTPLUS, S1MUL, ADJOINT, RELU, RELUMASK = 1, 2, 3, 4, 5


def _lib():
    from hashmodnffbanks_idr_amd import _lib as L
    return L


def _ops():
    from hashmodnffbanks_idr_amd import ops
    return ops


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _ints(shape, gen, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=gen, device=DEV).float()


def _bits(x):
    return (x.float() + 0.0).view(torch.int32)      # (+0.0: -0 -> +0)


def _assert_exact(got, ref, what):
    ref = ref.float()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if not torch.equal(_bits(got), _bits(ref)):
        bad = (_bits(got) != _bits(ref)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first at {i}: "
                             f"{got[i].item()!r} vs {ref[i].item()!r}")


class Window:
    """[rows, cols] view with row stride ld whose first element is `off` floats past a 16-byte boundary, in a buffer of
    NaN with a guard band before and after it.  untouched(): every float outside the window - guard bands and the
    rows' pad columns - is still that NaN."""

    def __init__(self, rows, cols, ld=None, off=0, init=None):
        ld = cols if ld is None else ld
        assert ld >= cols
        self.buf = torch.full((GUARD + off + rows * ld + GUARD,), float("nan"), device=DEV)
        self.v = self.buf.as_strided((rows, cols), (ld, 1), GUARD + off)
        assert self.v.data_ptr() % 16 == 4 * off
        if init is not None:
            self.v.copy_(init)
        self.inside = torch.zeros_like(self.buf, dtype=torch.bool)
        self.inside.as_strided((rows, cols), (ld, 1), GUARD + off).fill_(True)
        self.ld = ld

    def untouched(self):
        return bool(torch.isnan(self.buf[~self.inside]).all())


def _plan(ta, tb, M, N, K, a, b, has_ep=False, det=False):
    L = _lib()
    info = L.GemmPlanInfo()
    L.check(L.lib().hm_diag_gemm_plan(int(ta), int(tb), M, N, K, L.dptr(a), a.stride(0), L.dptr(b), b.stride(0),
                                      int(has_ep), int(det), ctypes.byref(info)))
    return info


def _gemm_ep(a, b, bias, tb, mode, M, N, K, c=None, scale=1.0, z=None, g=None, nz=0, out1=None, out2=None, out3=None):
    """hm_gemm_f32_ep on caller-owned views (ops.gemm_ep allocates C and out2 itself, always aligned)"""
    L = _lib()
    ep = L.GemmEpilogue()
    ep.mode, ep.nz, ep.scale, ep.beta, ep.threshold = mode, nz, scale, BETA, THR
    for name, ldn, t in (("z", "ldz", z), ("g", "ldg", g), ("out1", "ld1", out1), ("out2", "ld2", out2),
                         ("out3", "ld3", out3)):
        if t is not None:
            setattr(ep, name, t.data_ptr())
            setattr(ep, ldn, t.stride(0))
    L.check(L.lib().hm_gemm_f32_ep(0, int(tb), M, N, K, L.dptr(a), a.stride(0), L.dptr(b), b.stride(0), L.dptr(bias),
                                   L.dptr(c), c.stride(0) if c is not None else N, ctypes.byref(ep), L.stream_ptr(a)))


def _s1s2(z64):
    """exact for z in {0, 1, 2, ...} at beta = 100, threshold = 20"""
    pos = z64 >= 1
    return torch.where(pos, 1.0, 0.5), torch.where(pos, 0.0, BETA / 4)


def _check_softplus(got, v64, what):
    ref = torch.where(v64 >= 1, v64, torch.zeros_like(v64))
    at0 = v64 == 0
    _assert_exact(torch.where(at0, torch.zeros_like(got), got), ref, what)
    if bool(at0.any()):
        zs = got[at0]
        assert bool((zs.view(torch.int32) == zs.view(torch.int32)[0]).all()), f"{what}: softplus(0) has several values"
        assert abs(zs[0].item() - 0.6931471805599453 / BETA) <= 2e-9, f"{what}: softplus(0) = {zs[0].item()!r}"


def _run_mode(mode, A, B, tb, v64, gen, lay, flags):
    """one epilogue call with every destination and epilogue operand in a Window of layout lay = (pad, off): row stride
    cols + pad, base off floats past a 16-byte boundary; compared with float64.  flags: (g given, C wanted, out3 wanted)."""
    pad, off = lay
    with_g, want_c, want_o3 = flags
    M, N = v64.shape
    K = A.shape[1]
    what = f"mode {mode} M={M} N={N} K={K} {'NT' if tb else 'NN'} pad={pad} off={off} flags={flags}"
    masked = mode in (S1MUL, RELUMASK)
    nz = max(1, (N // 2) & ~3) if masked else N          # nz < N, a multiple of 4 where N allows it
    bias = _ints((N,), gen) if mode in (SOFTPLUS, RELU) else None
    scale = 0.5 if mode in (S1MUL, ADJOINT, RELUMASK) else 1.0
    v64 = (v64 + (bias.double() if bias is not None else 0.0)) * scale
    W = lambda cols, init=None: Window(M, cols, cols + pad, off, init)   # noqa: E731
    c = W(N) if (want_c or mode == SOFTPLUS) else None
    zw = gw = o2 = o3 = None
    if mode in (S1MUL, ADJOINT):
        zw = W(nz, _ints((M, nz), gen, 0, 2))
    elif mode == RELUMASK:
        zw = W(nz, _ints((M, nz), gen, -2, 2))
    if zw is not None and (with_g or mode == ADJOINT):
        gw = W(nz, _ints((M, nz), gen))
    o1 = W(nz)
    if mode == ADJOINT:
        o2 = W(N)
        o3 = W(N) if want_o3 else None
    _gemm_ep(A, B, bias, tb, mode, M, N, K, c=c.v if c else None, scale=scale, z=zw.v if zw else None,
             g=gw.v if gw else None, nz=nz if masked else 0, out1=o1.v, out2=o2.v if o2 else None,
             out3=o3.v if o3 else None)
    z64 = zw.v.double() if zw else None
    g64 = gw.v.double() if gw else (torch.zeros_like(z64) if zw else None)
    if c is not None:
        _assert_exact(c.v, v64, what + ": C")
    if mode == SOFTPLUS:
        _check_softplus(o1.v, v64, what + ": out1")
    elif mode == RELU:
        _assert_exact(o1.v, v64.clamp(min=0), what + ": out1")
    elif mode == RELUMASK:
        _assert_exact(o1.v, torch.where(z64 > 0, v64[:, :nz], 0.0) + g64, what + ": out1")
    elif mode == S1MUL:
        _assert_exact(o1.v, v64[:, :nz] * _s1s2(z64)[0] + g64, what + ": out1")
    else:
        s1, s2 = _s1s2(z64)
        _assert_exact(o1.v, v64 * s1, what + ": out1")
        _assert_exact(o2.v, v64 * g64 * s2, what + ": out2")
        if o3 is not None:
            _assert_exact(o3.v, g64 * s1, what + ": out3")
    for name, w in (("C", c), ("z", zw), ("g", gw), ("out1", o1), ("out2", o2), ("out3", o3)):
        assert w is None or w.untouched(), f"{what}: write outside the window of {name}"


MS, NS, KS = (1, 63, 64, 65, 95, 96, 97, 192), (4, 60, 64, 68, 257), (128, 445)


@pytest.fixture(scope="module")
def products():
    """integer operands of the largest shape and their float64 products, shared by the tests (slices of them are the
    smaller cases): {K: (A [192, K], B [K, 257], B^T [257, K], A B in float64)}"""
    gen = _gen(20)
    out = {}
    for K in KS:
        A, B = _ints((MS[-1], K), gen), _ints((K, NS[-1]), gen)
        out[K] = (A, B, B.t().contiguous(), A.double() @ B.double())
    return out


def _operands(products, M, N, K, tb):
    A, B, Bt, P = products[K]
    return A[:M], (Bt[:N] if tb else B[:, :N]), P[:M, :N]


def test_plain_tile_edges(products):
    """plain stores on both tile heights' edges, whole K and K tail, NN and NT; N = 4, 60, 64, 68 take the 16-byte
    path, 257 and the padded destinations the dword path"""
    ops = _ops()
    gen = _gen(21)
    routes = set()
    for K in KS:
        for tb in (False, True):
            for M in MS:
                for N in NS:
                    A, B, ref = _operands(products, M, N, K, tb)
                    info = _plan(0, tb, M, N, K, A, B)
                    routes.add((info.kernel, info.k_tail))
                    bias = _ints((N,), gen)
                    for pad, off in ((0, 0), (3, 1)):
                        c = Window(M, N, N + pad, off)
                        ops.gemm(A, B, bias, False, tb, out=c.v)
                        _assert_exact(c.v, ref + bias.double(), f"plain M={M} N={N} K={K} tb={tb} pad={pad} off={off}")
                        assert c.untouched(), f"plain M={M} N={N} K={K} tb={tb} pad={pad} off={off}: write outside C"
    assert (PIPE64, 0) in routes, routes       # (K = 445 without an epilogue stays on the generic kernel at these sizes)


@pytest.mark.parametrize("mode", [SOFTPLUS, S1MUL, ADJOINT, RELU, RELUMASK])
def test_epilogue_tile_edges(products, mode):
    """every epilogue mode on the same edges: whole K and the K-tail instantiation (K = 445 in the NN form), nz < N, with
    and without the g addend, C and out3 wanted or not, aligned (16-byte path where N and nz allow it) and padded"""
    gen = _gen(22 + mode)
    routes = set()
    i = 0
    for K in KS:
        for tb in (False, True):
            for M in MS:
                for N in NS:
                    A, B, ref = _operands(products, M, N, K, tb)
                    info = _plan(0, tb, M, N, K, A, B, has_ep=True)
                    routes.add((info.kernel, info.k_tail))
                    i += 1
                    flags = (bool(i & 1), bool(i & 2), bool(i & 4))
                    _run_mode(mode, A, B, tb, ref, gen, (0, 0), flags)
                    _run_mode(mode, A, B, tb, ref, gen, (1, 3), (not flags[0], not flags[1], not flags[2]))
    assert {(PIPE64, 0), (PIPE64, 1)} <= routes, routes


def _smallest_m96(N, K, has_ep):
    """the smallest M whose plan is the 96-row kernel: one row past the last M whose 64-row grid fits one round of the
    256 CUs"""
    M = 64 * (256 // ((N + 63) // 64)) + 1
    a, b = torch.empty(M - 1, K, device=DEV), torch.empty(K, N, device=DEV)
    assert _plan(0, 0, M - 1, N, K, a, b, has_ep).kernel == PIPE64
    return M


@pytest.mark.parametrize("N", [68, 257])
def test_m96_route(N):
    """the 96-row kernel (twelve waves, two groups of six) at the smallest M that takes it: N = 68 on the 16-byte path
    (with a partial column tile), N = 257 on the dword path; plain and two epilogues"""
    ops = _ops()
    K = 128
    M = _smallest_m96(N, K, False)
    gen = _gen(30 + N)
    A, B = _ints((M, K), gen), _ints((K, N), gen)
    ref = A.double() @ B.double()
    for has_ep in (False, True):
        info = _plan(0, 0, M, N, K, A, B, has_ep)
        assert info.kernel == PIPE96 and info.split == 1, (M, N, info.kernel, info.split)
    c = Window(M, N)
    ops.gemm(A, B, None, False, False, out=c.v)
    _assert_exact(c.v, ref, f"m96 plain M={M} N={N}")
    assert c.untouched()
    _run_mode(ADJOINT, A, B, False, ref, gen, (0, 0), (True, True, True))
    _run_mode(S1MUL, A, B, False, ref, gen, (0, 0), (True, False, False))
    Bt = B.t().contiguous()
    _run_mode(SOFTPLUS, A, Bt, True, ref, gen, (0, 0), (False, True, False))


@pytest.mark.parametrize("ld", [67, 445, 513, 516])
def test_alignment_fallback(products, ld):
    """destinations and epilogue operands as row slices 0, 4, 8 and 12 bytes off a 16-byte boundary with row strides that
    are no multiple of 4 floats (and 516, which is: there only the base decides): the result is the same, the rows'
    pad columns and the guard bands keep their NaN"""
    ops = _ops()
    gen = _gen(40 + ld)
    M, K = 97, 128
    for N in (64, 60):
        for tb in (False, True):
            A, B, ref = _operands(products, M, N, K, tb)
            assert _plan(0, tb, M, N, K, A, B).kernel == PIPE64
            for off in (0, 1, 2, 3):
                c = Window(M, N, ld, off)
                ops.gemm(A, B, None, False, tb, out=c.v)
                _assert_exact(c.v, ref, f"plain ld={ld} off={off} N={N} tb={tb}")
                assert c.untouched(), f"plain ld={ld} off={off} N={N} tb={tb}: write outside C"
                for mode in (ADJOINT, S1MUL, RELU):
                    _run_mode(mode, A, B, tb, ref, gen, (ld - N, off), (True, True, True))


def test_one_misaligned_operand_falls_back(products):
    """every array of the ADJOINT epilogue in turn is the only one off the 16-byte grid"""
    gen = _gen(50)
    M, N, K = 97, 64, 128
    A, B, ref = _operands(products, M, N, K, False)
    v64 = ref * 0.5
    for odd in ("c", "z", "g", "out1", "out2", "out3"):
        w = {}
        for name in ("c", "z", "g", "out1", "out2", "out3"):
            init = _ints((M, N), gen, 0, 2) if name == "z" else _ints((M, N), gen) if name == "g" else None
            w[name] = Window(M, N, N + 4, 1, init) if name == odd else Window(M, N, N, 0, init)
        _gemm_ep(A, B, None, False, ADJOINT, M, N, K, c=w["c"].v, scale=0.5, z=w["z"].v, g=w["g"].v, out1=w["out1"].v,
                 out2=w["out2"].v, out3=w["out3"].v)
        s1, s2 = _s1s2(w["z"].v.double())
        g64 = w["g"].v.double()
        for name, r in (("c", v64), ("out1", v64 * s1), ("out2", v64 * g64 * s2), ("out3", g64 * s1)):
            _assert_exact(w[name].v, r, f"only {odd} misaligned: {name}")
        assert all(x.untouched() for x in w.values()), f"only {odd} misaligned: write outside a window"


@pytest.mark.parametrize("M,N", [(192, 68), (192, 257), (97, 64), (65, 4)])
def test_every_element_of_both_halves(M, N):
    """C[m, n] = 16 (512 m + n): every element has its own value, so a wrong row split between the wave groups or a
    transposed quad cannot pass by symmetry, and every k-octet of both groups carries 1/16 of it, so a dropped partial
    cannot either (the partial sums j (512 m + n), j <= 16, stay below 2^24)"""
    ops = _ops()
    K = 128
    k = torch.arange(K, device=DEV)
    m = torch.arange(M, device=DEV, dtype=torch.float32)[:, None]
    n = torch.arange(N, device=DEV, dtype=torch.float32)[None, :]
    A = torch.where(k % 8 == 0, m, torch.where(k % 8 == 1, 1.0, 0.0)).contiguous()                # [M, K]
    B = torch.where((k % 8 == 0)[:, None], 512.0, torch.where((k % 8 == 1)[:, None], n, 0.0)).contiguous()   # [K, N]
    ref = (16.0 * (512.0 * m + n)).double()
    assert _plan(0, 0, M, N, K, A, B).kernel == PIPE64
    for tb, Bop in ((False, B), (True, B.t().contiguous())):
        for pad, off in ((0, 0), (1, 0)):
            c = Window(M, N, N + pad, off)
            ops.gemm(A, Bop, None, False, tb, out=c.v)
            _assert_exact(c.v, ref, f"unique values M={M} N={N} tb={tb} pad={pad}")
            assert c.untouched()
            o1 = Window(M, N, N + pad, off)
            _gemm_ep(A, Bop, None, tb, RELU, M, N, K, out1=o1.v)
            _assert_exact(o1.v, ref, f"unique values, RELU without C, M={M} N={N} tb={tb} pad={pad}")
            assert o1.untouched()


# (M, N): tile edges of the 64-row part kernel, and the smallest M of the 96-row part kernel at N = 68
@pytest.mark.parametrize("M,N", [(1, 4), (65, 64), (97, 68), (192, 257), (8193, 68)])
def test_deterministic_mode(M, N):
    """split K (K = 512 on few tiles): the deterministic mode's part kernels write their slabs through the same tail;
    on integers it equals the default mode (atomics) and float64 bit for bit, on random fp32 data two runs are equal"""
    ops = _ops()
    K = 512
    gen = _gen(60 + M)
    for ta, tb in ((0, 0), (0, 1), (1, 0)):
        A = _ints((K, M) if ta else (M, K), gen)
        B = _ints((N, K) if tb else (K, N), gen)
        info = _plan(ta, tb, M, N, K, A, B, det=True)
        assert info.part == 1 and info.split > 1 and info.kernel == (PIPE96 if M > 4096 else PIPE64), \
            (ta, tb, info.kernel, info.split, info.part)
        ref = (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())
        for pad, off in ((0, 0), (3, 1)):
            outs = []
            for det in (False, True):
                c = Window(M, N, N + pad, off)
                with ops.deterministic(det):
                    ops.gemm(A, B, None, bool(ta), bool(tb), out=c.v)
                _assert_exact(c.v, ref, f"det={det} ta={ta} tb={tb} M={M} N={N} pad={pad}")
                assert c.untouched(), f"det={det} ta={ta} tb={tb} M={M} N={N} pad={pad}: write outside C"
                outs.append(c.v)
            assert torch.equal(_bits(outs[0]), _bits(outs[1]))
        Af, Bf = torch.randn(A.shape, generator=gen, device=DEV), torch.randn(B.shape, generator=gen, device=DEV)
        with ops.deterministic(True):
            r1 = ops.gemm(Af, Bf, None, bool(ta), bool(tb))
            r2 = ops.gemm(Af, Bf, None, bool(ta), bool(tb))
        assert torch.equal(r1, r2), f"deterministic runs differ: ta={ta} tb={tb} M={M} N={N}"
        assert bool(((r1.double() - ((Af.double().t() if ta else Af.double()) @ (Bf.double().t() if tb else Bf.double())))
                     .abs() <= (K + 2) * 2.0 ** -24 *
                     ((Af.abs().double().t() if ta else Af.abs().double()) @
                      (Bf.abs().double().t() if tb else Bf.abs().double()))).all())
