"""Case lists, inputs and float64 references of the elementwise / reduction / copy kernel tests (csrc/hm_elem.hip,
hm_loss.hip, hm_optim.hip), shared by tests/test_elem_cases_cpu.py (the inputs and references checked on CPU) and
tests/test_elem_gpu.py (the kernels against them).  Import-only: no test lives here.

Every reference is a closed-form expression of ONE order of one op (order 0 = value, 1 = backward, 2 = backward of the
backward), written for any dtype: `xxx_ref(order, inputs, ..., dt)` evaluates it with torch on the CPU in `dt`.  The
inputs are fp32 tensors; dt = float64 gives the reference, dt = float32 gives "torch's fp32 evaluation of the same
expression", whose error against the reference sets the tolerance of the kernel (limit()).  The CPU test checks every
closed form against float64 autograd of the forward expression, so a reference cannot share a mistake with the kernel it
was read from.

Tolerance (no fixed numbers; see limit()):  a kernel output may differ from the float64 reference by at most
    4 * e32 + 2^-22 * scale,   but never more than 2e-5 * scale
e32   = max |fp32 torch evaluation - reference| on the same inputs,
scale = max |reference| (per row for rownorm),
factor 4: the kernels use the hardware rcp / exp2 / log2 and another summation order, each about an ulp over torch's;
the floor of two ulps keeps a case where torch happens to be exact from demanding exactness; 2e-5 * scale is the bound
of the existing _second_order_check (tests/test_nffb_gpu.py), so a badly conditioned input cannot widen the limit -
the CPU test asserts e32 <= 2e-5 * scale / 4 for every case, i.e. the cap is never what decides.
"""
import itertools

import numpy as np
import torch

CAP = 2e-5
FLOOR = 2.0 ** -22
F32, F64 = torch.float32, torch.float64


def _gen(*key):
    return torch.Generator(device="cpu").manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key))) % (2 ** 31))


def randn(shape, *key):
    return torch.randn(shape, generator=_gen(*key), dtype=F32)


def f32(v):
    """the double value of the fp32 rounding of a python float (what a kernel receives for a float argument)"""
    return float(np.float32(v))


# ---- tolerance -------------------------------------------------------------------------------------------------------
def errors(ref64, ref32, rowwise=False):
    """(e32, scale) of one output: numbers, or per-row vectors"""
    d = (ref32.to(F64) - ref64).abs()
    if rowwise:
        return d.amax(1), ref64.abs().amax(1)
    return (float(d.max()) if d.numel() else 0.0), (float(ref64.abs().max()) if d.numel() else 0.0)


def limit(e32, scale):
    lim = 4.0 * e32 + FLOOR * scale
    cap = CAP * scale
    return torch.minimum(lim, cap) if torch.is_tensor(lim) else min(lim, cap)


def compare(name, got, ref64, ref32, rowwise=False):
    """print and assert |got - ref64| <= limit(e32, scale); got: the kernel's output (any device)"""
    got = got.detach().to("cpu", F64)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), name
    e32, scale = errors(ref64, ref32, rowwise)
    lim = limit(e32, scale)
    d = (got - ref64).abs()
    if rowwise:
        err = d.amax(1)
        k = int((err - lim).argmax())
        print(f"    {name}: worst row {k}: err {float(err[k]):.3e} limit {float(lim[k]):.3e} "
              f"(e32 {float(e32[k]):.3e}, scale {float(scale[k]):.3e}); max err {float(err.max()):.3e}")
        assert bool((err <= lim).all()), f"{name}: row {k} err {float(err[k]):.3e} > limit {float(lim[k]):.3e}"
        return
    err = float(d.max()) if d.numel() else 0.0
    print(f"    {name}: err {err:.3e} limit {lim:.3e} (e32 {e32:.3e}, scale {scale:.3e})")
    assert err <= lim, f"{name}: err {err:.3e} > limit {lim:.3e}"


# ---- column sums (exact) ---------------------------------------------------------------------------------------------
COLSUM_SMALL = [(1, 1), (7, 3), (8, 256), (9, 257), (31, 1), (32, 5), (33, 257), (65, 300), (0, 4)]
COLSUM_ATOMIC_BIG = (2097121, 2)         # the first M whose 32-row slabs exceed 65535: the slab height is re-sized
COLSUM_DET_EDGE = [(16384, 3), (16385, 3)]   # exactly 512 slabs of 32 rows / the first M with 33-row slabs
COLSUM_MAX_ABS = 4


def colsum_ints(M, N, *key):
    """[M, N] integers of [-4, 4] as fp32"""
    return torch.randint(-COLSUM_MAX_ABS, COLSUM_MAX_ABS + 1, (M, N), generator=_gen(M, N, 17, *key)).to(F32)


def colsum_as_view(x):
    """the same values as a view with ld = N + 3 that starts at column 1 of a wider buffer (pads hold 7: a read of
    them changes the sum)"""
    M, N = x.shape
    buf = torch.full((M, N + 3), 7.0, dtype=F32, device=x.device)
    buf[:, 1:1 + N] = x
    return buf[:, 1:1 + N]


def colsum_ref(x, out0=None):
    """int64 column sums (+ the initial out)"""
    s = x.to("cpu").to(torch.int64).sum(0)
    return s if out0 is None else s + out0.to("cpu").to(torch.int64)


def colsum_multi_shapes():
    """the 17 (M, N) of the one colsum_into_multi call that spans two tables of 16: the atomic slab re-sizing next to small
    items, M = 0, N = 0; the last two items write the two halves of ONE output"""
    return [(2097121, 1), (33, 257), (0, 4), (5, 0), (1, 1), (7, 3), (8, 256), (9, 257), (31, 1), (32, 5), (65, 300),
            (100, 2), (64, 64), (3, 511), (1000, 9), (40, 130), (24, 130)]


# ---- copies (exact) --------------------------------------------------------------------------------------------------
COPY_ROWS = [1, 3, 65]
COPY_COLS = [1, 3, 4, 5, 256, 1028]
COPY_PADS = [0, 1, 4]
COPY_OFFS = [0, 1, 4]
SENTINEL = -12345.0


def copy_cases(rows):
    """(cols, src offset, src pad, dst offset, dst pad): ld = offset + cols + pad.  hm_copy2d_f32 takes the float4 path iff
    cols % 4 == 0, both ld % 4 == 0 and both pointers are 16-byte aligned (offset % 4 == 0)"""
    return list(itertools.product(COPY_COLS, COPY_OFFS, COPY_PADS, COPY_OFFS, COPY_PADS))


def copy_is_vec4(cols, so, sp, do, dp):
    return cols % 4 == 0 and (so + cols + sp) % 4 == 0 and (do + cols + dp) % 4 == 0 and so % 4 == 0 and do % 4 == 0


# ---- softplus --------------------------------------------------------------------------------------------------------
SOFTPLUS_N = [1, 3, 4, 5, 1023, 1024, 1025, 4099]
SP_BETA, SP_THR = 100.0, 20.0


def threshold_neighbours():
    """fp32 neighbours of z = 0.2 (beta z = threshold): two below, fl(0.2), two above"""
    z = np.float32(0.2)
    lo1 = np.nextafter(z, np.float32(-1)); lo2 = np.nextafter(lo1, np.float32(-1))
    hi1 = np.nextafter(z, np.float32(1)); hi2 = np.nextafter(hi1, np.float32(1))
    return [float(v) for v in (lo2, lo1, z, hi1, hi2)]


def softplus_inputs(n):
    """z: +-0, the threshold neighbours, +-1e-3, -0.17, -5, -1e3, 5, a denormal, then random values of width 0.2;
    gy, gg: unit normals"""
    special = threshold_neighbours() + [0.0, -0.0, 1e-3, -1e-3, -0.17, -5.0, -1e3, 5.0, 1e-40]
    z = randn((n,), n, 1) * 0.2
    k = min(n, len(special))
    z[:k] = torch.tensor(special[:k], dtype=F32)
    return dict(z=z, gy=randn((n,), n, 2), gg=randn((n,), n, 3))


def softplus_exact_mask(z, beta=SP_BETA, thr=SP_THR):
    """the kernel's predicate: the fp32 product z * beta > threshold"""
    return (z.to(F32) * torch.tensor(beta, dtype=F32)) > torch.tensor(thr, dtype=F32)


def softplus_terms(z, beta=SP_BETA, thr=SP_THR):
    """float64 (y, s1, s2, dl, ds1, ds2) on the fp32 z: value, first and second derivative, and the derivatives of the
    logarithm term, s1 and s2 along bz = beta z (what a rounding of the exponent's argument is multiplied by)"""
    m = softplus_exact_mask(z, beta, thr)
    z = z.to(F64)
    bz = z * beta
    t = torch.exp(-bz.abs())
    y = torch.clamp(z, min=0.0) + torch.log1p(t) / beta
    s1 = torch.sigmoid(bz)
    s2 = beta * s1 * torch.sigmoid(-bz)
    dl = t / (1.0 + t) / beta
    ds1 = s2 / beta
    ds2 = s2 * (1.0 - 2.0 * s1)
    one, zero = torch.ones_like(z), torch.zeros_like(z)
    return (torch.where(m, z, y), torch.where(m, one, s1), torch.where(m, zero, s2), torch.where(m, zero, dl),
            torch.where(m, zero, ds1), torch.where(m, zero, ds2))


def softplus_ref(order, inp, beta=SP_BETA, thr=SP_THR):
    """float64 outputs of hm_softplus and their limits.  hm_common.h documents < 2e-9 absolute for the logarithm term at
    beta = 100 and ~3e-7 relative for s1, s2.  On top of those the number format gives: the two fp32 roundings of the
    exponent's argument (z * beta, then * log2 e) move bz by up to 2^-23 |bz|, i.e. the output by that times its
    derivative along bz; every fp32 product / sum that follows rounds by 2^-24 of its result; the exp2 unit flushes
    results below the smallest normal 2^-126 to zero."""
    y, s1, s2, dl, ds1, ds2 = softplus_terms(inp["z"], beta, thr)
    bz = (inp["z"].to(F64) * beta).abs()
    u, tiny = 2.0 ** -24, 2.0 ** -126
    arg = 2.0 * u * bz
    l_y = 2e-9 * (100.0 / beta) + arg * dl + u * y.abs()
    l_s1 = 3e-7 * s1 + arg * ds1.abs() + tiny
    l_s2 = 3e-7 * s2 + arg * ds2.abs() + tiny * beta
    exact = softplus_exact_mask(inp["z"], beta, thr)
    l_y, l_s1, l_s2 = (torch.where(exact, torch.zeros_like(v), v) for v in (l_y, l_s1, l_s2))
    z0 = lambda v: torch.where(exact, torch.zeros_like(v), v)      # exact region: z, gy * 1, gg * 1, gg * gy * 0
    if order == 0:
        return [(y, l_y)]
    gy = inp["gy"].to(F64)
    if order == 1:
        r = gy * s1
        return [(r, z0(gy.abs() * l_s1 + u * r.abs()))]
    gg = inp["gg"].to(F64)
    r0, r1 = gg * s1, gg * gy * s2
    return [(r0, z0(gg.abs() * l_s1 + u * r0.abs())), (r1, z0((gg * gy).abs() * l_s2 + 3.0 * u * r1.abs()))]


# ---- sine ------------------------------------------------------------------------------------------------------------
SINE_N = [1, 255, 256, 257]
SINE_W0 = [30.0, 56.0]           # L^F - L of the two filter-bank embedders


def sine_inputs(n, w0):
    return dict(x=torch.rand((n,), generator=_gen(n, w0, 1), dtype=F32) * 2 - 1, gy=randn((n,), n, w0, 2),
                gg=randn((n,), n, w0, 3))


def sine_ref(order, inp, w0, dt):
    """u = x * w0 is formed in fp32, as the kernel (and torch.sin(x * w0)) forms it; sin / cos of THAT u in dt"""
    u = (inp["x"] * torch.tensor(w0, dtype=F32)).to(dt)
    gy, gg = inp["gy"].to(dt), inp["gg"].to(dt)
    if order == 0:
        return [torch.sin(u)]
    if order == 1:
        return [gy * torch.cos(u) * w0]
    return [gg * w0 * torch.cos(u), -(gg * w0 * gy) * (torch.sin(u) * w0)]


# ---- positional encoding ---------------------------------------------------------------------------------------------
POSENC_SHAPES = [(1, 1), (3, 6), (4, 8), (4, 16), (64, 2)]     # (dim, n_freq)
POSENC_N = [1, 65]


def posenc_freqs(n_freq):
    return tuple(float(2 ** k) for k in range(n_freq))      # powers of two: the fp32 arguments f * c are exact


def posenc_inputs(n, dim, n_freq):
    W = 2 * dim + 2 * n_freq * dim
    return dict(c=torch.rand((n, dim), generator=_gen(n, dim, n_freq, 1), dtype=F32) * 2 - 1,
                g=randn((n, W), n, dim, n_freq, 2), gg=randn((n, dim), n, dim, n_freq, 3))


def posenc_fwd(c, freqs):
    parts = [c, c]
    for f in freqs:
        parts += [torch.sin(c * f), torch.cos(c * f)]
    return torch.cat(parts, 1)


def posenc_ref(order, inp, freqs, dt):
    c, g, gg = inp["c"].to(dt), inp["g"].to(dt), inp["gg"].to(dt)
    D = c.shape[1]
    if order == 0:
        return [posenc_fwd(c, freqs)]
    if order == 1:
        acc = g[:, :D] + g[:, D:2 * D]
        for k, f in enumerate(freqs):
            gs, gc = g[:, 2 * D + 2 * k * D:][:, :D], g[:, 2 * D + (2 * k + 1) * D:][:, :D]
            acc = acc + f * (torch.cos(c * f) * gs - torch.sin(c * f) * gc)
        return [acc]
    parts, acc = [gg, gg], torch.zeros_like(c)
    for k, f in enumerate(freqs):
        gs, gc = g[:, 2 * D + 2 * k * D:][:, :D], g[:, 2 * D + (2 * k + 1) * D:][:, :D]
        sn, cs = torch.sin(c * f), torch.cos(c * f)
        parts += [gg * f * cs, -(gg * f * sn)]
        acc = acc + f * f * (sn * gs + cs * gc)
    return [torch.cat(parts, 1), -(gg * acc)]


# ---- row normalisation -----------------------------------------------------------------------------------------------
ROWNORM_W = [1, 2, 7, 8, 9, 56, 127, 128]
ROWNORM_ROWS = [1, 31, 32, 33, 100]
ROWNORM_EPS = 1e-5


def rownorm_constant(W):
    """the value of the constant row: one whose row mean is exact in fp32 however it is formed (sum * fl(1 / W) or
    sum / W; the sums of W copies are exact).  A constant row whose mean is off by one ulp has yh = ulp / sqrt(eps)
    instead of 0 and, through the 1 / (W eps) of the second order, an O(1) output where the reference is exactly 0:
    that would measure the conditioning of the input, not the kernel."""
    for v in (0.5, 1.0, 0.75, 3.0, 0.25):
        s = np.float32(W) * np.float32(v)
        if s * (np.float32(1.0) / np.float32(W)) == np.float32(v) and s / np.float32(W) == np.float32(v):
            return v
    raise AssertionError(f"no exact constant for W = {W}")


def rownorm_const_row(rows):
    return rows // 2 if rows >= 3 else None


def rownorm_inputs(W, rows):
    """rows in turn: unit normal | mean 8 with unit spread; row rows // 2 is constant (sigma = sqrt(eps)).
    W = 2 is the exception: there yh = +-(1 - eps / (2 d^2) ...) for a half-difference d >> sqrt(eps), every gradient is the
    small remainder h eps / (d^2 sigma) of two cancelling terms, and a row's own maximum (the scale here) is that
    remainder - fp32 torch itself is off by 1e-4 .. 1 of it on unit-normal rows.  So the W = 2 rows have spread 4e-3,
    about sqrt(eps), where the terms do not cancel; the lanes W = 2 leaves empty do not depend on the values.
    The comparison is row by row, and a random row now and then has an output whose own maximum is small against its
    terms (2 % of the mean-8 rows at the second order).  Such a row measures its conditioning, not the kernel: a row on
    which torch's fp32 evaluation of any output is off by more than 2e-5 / 8 of that output's row maximum is drawn
    again (from the reference alone; tests/test_elem_cases_cpu.py then holds every row to 2e-5 / 4)."""
    def draw(salt):
        y = randn((rows, W), W, rows, 1, salt)
        if W == 2:
            y *= 4e-3
        else:
            y[1::2] += 8.0
        return dict(y=y, g=randn((rows, W), W, rows, 2, salt), gg=randn((rows, W), W, rows, 3, salt))
    inp = draw(0)
    k = rownorm_const_row(rows)
    if k is not None:
        inp["y"][k] = rownorm_constant(W)
    for salt in range(1, 40 if W > 1 else 1):
        bad = torch.zeros(rows, dtype=torch.bool)
        for order in (0, 1, 2):
            for r64, r32 in zip(rownorm_ref(order, inp, ROWNORM_EPS, F64), rownorm_ref(order, inp, ROWNORM_EPS, F32)):
                e32, scale = errors(r64, r32, rowwise=True)
                bad |= e32 > CAP / 8 * scale
        if k is not None:
            bad[k] = False
        if not bool(bad.any()):
            break
        new = draw(salt)
        for name in inp:
            inp[name][bad] = new[name][bad]
    return inp


def rownorm_fwd(y, eps):
    d = y - y.mean(1, keepdim=True)
    return d / torch.sqrt((d * d).mean(1, keepdim=True) + eps)


def rownorm_ref(order, inp, eps, dt):
    y, g, gg = inp["y"].to(dt), inp["g"].to(dt), inp["gg"].to(dt)
    n, eps = y.shape[1], f32(eps)
    d = y - y.mean(1, keepdim=True)
    sigma = torch.sqrt((d * d).mean(1, keepdim=True) + eps)
    yh = d / sigma
    if order == 0:
        return [yh]

    def F(u):
        return (u - u.mean(1, keepdim=True) - yh * (u * yh).mean(1, keepdim=True)) / sigma
    if order == 1:
        return [F(g)]
    s = lambda t: t.sum(1, keepdim=True)
    a = s(gg * g) - s(gg) * s(g) / n
    b, c = s(gg * yh), s(g * yh)
    fq = gg - s(gg) / n - yh * b / n
    fg = g - s(g) / n - yh * c / n
    return [F(gg), -(yh * (a - b * c / n) + c * fq + b * fg) / (n * sigma * sigma)]


# ---- sdf head --------------------------------------------------------------------------------------------------------
HEAD_N = [1, 255, 257]
HEAD_COLS = [1, 2, 257]
HEAD_BETA = [0.01, 0.1, 1.0]
HEAD_SPECIAL = [0.0, 1e-8, -1e-8, 1e-3, -1e-3, 0.5, -0.5, 3.0, -3.0, 50.0, -50.0, 1e4, -1e4]


def head_inputs(n, cols):
    zl = randn((n, cols), n, cols, 1)
    s = randn((n,), n, cols, 2) * 0.3
    s[n // 2:] = randn((n - n // 2,), n, cols, 3) * 0.01
    k = min(n, len(HEAD_SPECIAL))
    s[:k] = torch.tensor(HEAD_SPECIAL[:k], dtype=F32)
    zl[:, 0] = s
    return dict(zl=zl, d_out=randn((n, cols), n, cols, 4), cb=randn((n,), n, cols, 5))


def head_fwd_ref(s, beta, dt):
    """(sdf, c, denom): tests/helpers.py mlp_fp64's clamp, c = d sdf / d s with rho held constant"""
    s, beta = s.to(dt), f32(beta)
    rho = (1.0 / beta) * (0.5 + 0.5 * torch.sign(s) * torch.expm1(-s.abs() / beta))
    denom = 2.0 + rho
    sdf = torch.tanh(s / denom)
    return [sdf, (1.0 - sdf * sdf) / denom, denom]


def head_bwd_ref(d0, sdf, c, denom, cb, dt):
    """column 0 of z-bar from the fp32 (sdf, c, denom) the backward kernel is handed"""
    d0, sdf, c, denom = d0.to(dt), sdf.to(dt), c.to(dt), denom.to(dt)
    r = d0 * c
    return [r if cb is None else r + cb.to(dt) * (-2.0 * sdf * c / denom)]


# ---- weight norm -----------------------------------------------------------------------------------------------------
WN_COLS = [1, 255, 256, 257, 1000]
WN_LAYERS = 32                   # HM_MAX_LAYERS * 2: the by-value table's limit


def wn_inputs(n_layers=WN_LAYERS):
    """per layer (v [rows, cols], g [rows, 1], gw [rows, cols]); cols cycle through WN_COLS, rows 1 .. 5.  At cols = 1
    grad_v is a difference of two equal terms (exactly 0); |v| stays in [0.5, 1.5] there so that the rounding of those
    terms stays at the scale of the other layers' gradients"""
    out = []
    for i in range(n_layers):
        rows, cols = 1 + i % 5, WN_COLS[i % len(WN_COLS)]
        v = randn((rows, cols), i, 1)
        if cols == 1:
            v = torch.sign(v) * (0.5 + torch.rand((rows, 1), generator=_gen(i, 9), dtype=F32))
        out.append((v, randn((rows, 1), i, 2), randn((rows, cols), i, 3)))
    return out


def wn_ref(layers, with_grad, dt):
    """(w, grad_v, grad_g), each the concatenation over layers (over the layers of `with_grad` for the gradients)"""
    ws, gvs, ggs = [], [], []
    for i, (v, g, gw) in enumerate(layers):
        v, g, gw = v.to(dt), g.to(dt), gw.to(dt)
        norm = torch.sqrt((v * v).sum(1, keepdim=True))
        ws.append((g * v / norm).reshape(-1))
        if i in with_grad:
            dot = (gw * v).sum(1, keepdim=True)
            gvs.append((g * (gw / norm - v * dot / norm ** 3)).reshape(-1))
            ggs.append((dot / norm).reshape(-1))
    return [torch.cat(ws), torch.cat(gvs), torch.cat(ggs)]


# ---- ClipAdam --------------------------------------------------------------------------------------------------------
ADAM_NUMEL = [1, 3, 8191, 8192, 8193, 8195, 16385]      # around the 8192-element chunk of one workgroup
ADAM_STEPS = 3
ADAM_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def adam_inputs(gscale):
    """(params, [grads of step 0, 1, 2]) as fp32 CPU tensors"""
    ps = [randn((n,), n, 1) for n in ADAM_NUMEL]
    gs = [[randn((n,), n, 2, it) * gscale for n in ADAM_NUMEL] for it in range(ADAM_STEPS)]
    return ps, gs


def adam_ref(ps, gs, max_norm):
    """clip_grad_norm_(max_norm) + torch.optim.Adam written out in float64, with the hyper-parameters as the kernel
    receives them (fp32).  Returns per step (params, clipped grads, total norm)."""
    lr, b1, b2, eps = (f32(ADAM_HYPER[k]) for k in ("lr", "b1", "b2", "eps"))
    p = [t.to(F64).clone() for t in ps]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    out = []
    for it, grads in enumerate(gs):
        g = [t.to(F64) for t in grads]
        total = float(torch.sqrt(sum((t * t).sum() for t in g)))
        coef = min(f32(max_norm) / (total + f32(1e-6)), 1.0) if max_norm else 1.0
        g = [t * coef for t in g]
        t_ = it + 1
        bc1, bc2 = 1.0 - b1 ** t_, 1.0 - b2 ** t_
        for k in range(len(p)):
            m[k] = m[k] + (g[k] - m[k]) * (1.0 - b1)
            v[k] = v[k] * b2 + (1.0 - b2) * g[k] * g[k]
            p[k] = p[k] - (lr / bc1) * (m[k] / (torch.sqrt(v[k]) / np.sqrt(bc2) + eps))
        out.append(([t.clone() for t in p], g, total))
    return out


# ---- IDR loss --------------------------------------------------------------------------------------------------------
LOSS_N = [1023, 1024, 1025]      # around the 1024 lanes of the one workgroup
LOSS_M = [0, 1, 1025]
LOSS_ALPHA = [50.0, 1600.0]      # 1600: the start value after five doublings of the schedule
LOSS_W_EIK, LOSS_W_MASK = 0.1, 100.0


def loss_inputs(n, m):
    g = _gen(n, m, 1)
    sdf = torch.randn((n, 1), generator=g) * 0.05
    sdf[0], sdf[1], sdf[2] = 1.0, -1.0, 0.0
    hit = torch.rand(n, generator=g) > 0.4
    inside = torch.rand(n, generator=g) > 0.3
    hit[:3], inside[:3] = False, torch.tensor([True, False, True])[:n]
    grad = torch.randn((m, 3), generator=g)
    if m > 2:
        grad[1] = 0.0
    return dict(rgb=torch.rand((n, 3), generator=g), gt=torch.rand((1, n, 3), generator=g), sdf=sdf, hit=hit, inside=inside,
                grad=grad)


def loss_ref(inp, alpha):
    """float64 terms and gradients of d (1.7 loss): loss.py's torch formulation with autograd, all in double"""
    from hashmodnffbanks_idr_amd.model import loss as L
    rgb, sdf, grad = (inp[k].to(F64).clone().requires_grad_(True) for k in ("rgb", "sdf", "grad"))
    out = {"rgb_values": rgb, "sdf_output": sdf, "grad_theta": grad, "network_object_mask": inp["hit"],
           "object_mask": inp["inside"]}
    terms = L.idr_loss_terms_torch(out, inp["gt"].to(F64), LOSS_W_EIK, LOSS_W_MASK, alpha)
    (terms["loss"] * 1.7).backward()
    grads = [t.grad if t.grad is not None else torch.zeros_like(t) for t in (rgb, sdf, grad)]
    return {k: float(v.detach()) for k, v in terms.items()}, grads
