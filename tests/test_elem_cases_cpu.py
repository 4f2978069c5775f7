"""tests/elem_cases.py on the CPU: every closed-form reference against float64 autograd of the forward expression (so a
reference cannot share a mistake with the kernel whose comment it was read from), the conditioning of every case (torch's
fp32 evaluation stays within a quarter of the 2e-5 cap, so the cap never decides a limit), and the properties the exact
tests rely on (the threshold neighbours straddle in fp32, the integer column sums stay below 2^24, the copy cases reach
both sides of every float4 condition)."""
import numpy as np
import pytest
import torch

import elem_cases as E

F32, F64 = torch.float32, torch.float64


def _conditioned(name, refs64, refs32, rowwise=False):
    for k, (r64, r32) in enumerate(zip(refs64, refs32)):
        e32, scale = E.errors(r64, r32, rowwise)
        worst = float((e32 / scale.clamp_min(1e-300)).max()) if rowwise else e32 / max(scale, 1e-300)
        print(f"    {name} out{k}: fp32 torch error / scale {worst:.3e}")
        if rowwise:
            assert bool((e32 <= 0.25 * E.CAP * scale).all()), (name, k, worst)
        else:
            assert e32 <= 0.25 * E.CAP * scale, (name, k, worst)


def _second_order(fwd, x64, m64, r64):
    """(y, gx, d/dm of <gx, r>, d/dx of <gx, r>) by float64 autograd: gx = J^T m"""
    x, m = x64.clone().requires_grad_(True), m64.clone().requires_grad_(True)
    y = fwd(x)
    (gx,) = torch.autograd.grad((y * m).sum(), x, create_graph=True)
    d_m, d_x = torch.autograd.grad((gx * r64).sum(), (m, x))
    return y.detach(), gx.detach(), d_m, d_x


def _close(a, b, what):
    assert a.shape == b.shape, what
    scale = max(float(b.abs().max()), 1e-300) if b.numel() else 1.0
    assert float((a - b).abs().max()) <= 1e-10 * scale, (what, float((a - b).abs().max()), scale)


# ---- limit() ---------------------------------------------------------------------------------------------------------
def test_limit_is_set_by_the_reference_and_capped():
    assert E.limit(0.0, 1.0) == 2.0 ** -22
    assert E.limit(1e-7, 2.0) == 4e-7 + 2.0 ** -21
    assert E.limit(1.0, 1.0) == 2e-5
    assert E.limit(1e-7, 0.0) == 0.0
    lim = E.limit(torch.tensor([0.0, 1.0], dtype=F64), torch.tensor([1.0, 1.0], dtype=F64))
    assert lim.tolist() == [2.0 ** -22, 2e-5]


# ---- exact cases -----------------------------------------------------------------------------------------------------
def test_colsum_cases_stay_exact_in_fp32():
    shapes = E.COLSUM_SMALL + [E.COLSUM_ATOMIC_BIG] + E.COLSUM_DET_EDGE + E.colsum_multi_shapes()
    for M, N in shapes:
        assert (M + 1) * E.COLSUM_MAX_ABS < 2 ** 24, (M, N)        # every partial sum (+ the initial out) is an integer < 2^24
    x = E.colsum_ints(33, 257)
    assert x.dtype == F32 and float(x.abs().max()) == E.COLSUM_MAX_ABS and torch.equal(x, x.round())
    v = E.colsum_as_view(x)
    assert v.stride() == (260, 1) and v.storage_offset() == 1 and torch.equal(v, x)
    assert torch.equal(E.colsum_ref(v), x.double().sum(0).long())
    # the branch edges the cases are named for
    M = E.COLSUM_ATOMIC_BIG[0]
    assert (M - 1 + 31) // 32 == 65535 and (M + 31) // 32 == 65536
    assert [(m + 31) // 32 for m, _ in E.COLSUM_DET_EDGE] == [512, 513]
    ms = {m for m, _ in E.COLSUM_SMALL}
    assert {0, 1, 7, 8, 9, 32, 33} <= ms
    multi = E.colsum_multi_shapes()
    assert len(multi) == 17 and multi[0] == (M, 1) and (33, 257) in multi and (0, 4) in multi
    assert any(n == 0 and m > 0 for m, n in multi) and multi[-1][1] == multi[-2][1]


def test_copy_cases_reach_both_sides_of_every_vec4_condition():
    cases = E.copy_cases(1)
    assert len(cases) == len(E.COPY_COLS) * 81
    vec = [c for c in cases if E.copy_is_vec4(*c)]
    assert vec and len(vec) < len(cases)
    # each condition alone decides at least once: a float4 case with exactly that one condition flipped is in the list
    flips = dict(cols=lambda c: (5,) + c[1:], src_ptr=lambda c: (c[0], 1, c[2], c[3], c[4]),
                 src_ld=lambda c: (c[0], c[1], 1, c[3], c[4]), dst_ptr=lambda c: (c[0], c[1], c[2], 1, c[4]),
                 dst_ld=lambda c: (c[0], c[1], c[2], c[3], 1))
    base = (256, 0, 0, 0, 0)
    assert base in vec
    for name, flip in flips.items():
        assert flip(base) in cases and not E.copy_is_vec4(*flip(base)), name
    # misaligned pointers with ld % 4 == 0: offset 1 + pad 3 is not in the list, offset 4 / pad 4 and offset 1 / pad 0 are
    assert (4, 4, 4, 4, 4) in vec and (1028, 4, 0, 0, 4) in vec


def test_softplus_grid_straddles_the_threshold_in_fp32():
    nb = torch.tensor(E.threshold_neighbours(), dtype=F32)
    assert torch.equal(nb, nb.sort().values) and len(set(nb.tolist())) == 5
    m = E.softplus_exact_mask(nb)
    print("    neighbours", [f"{v:.9g}" for v in nb.tolist()], "exact region", m.tolist())
    assert bool(m.any()) and not bool(m.all())
    k = int(m.int().argmax())
    assert bool(m[k:].all()) and not bool(m[:k].any())            # one switch, between two ADJACENT fp32 values
    for n in E.SOFTPLUS_N:
        inp = E.softplus_inputs(n)
        assert inp["z"].shape == (n,) and inp["z"].dtype == F32
    z = E.softplus_inputs(1025)["z"]
    ex = E.softplus_exact_mask(z)
    assert bool(ex.any()) and bool((~ex).any())
    assert bool((z == 0).sum() >= 2) and bool(((z != 0) & (z.abs() < 2.0 ** -126)).any())      # +-0, a denormal
    # in the exact region the reference is z, 1, 0 with a zero limit
    inp = E.softplus_inputs(1025)
    (y, ly), = E.softplus_ref(0, inp)
    assert torch.equal(y[ex], z[ex].double()) and float(ly[ex].abs().max()) == 0.0
    (r0, l0), (r1, l1) = E.softplus_ref(2, inp)
    assert torch.equal(r0[ex], inp["gg"][ex].double()) and float(r1[ex].abs().max()) == 0.0
    assert float(l0[ex].abs().max()) == 0.0 and float(l1[ex].abs().max()) == 0.0


def test_softplus_reference_matches_float64_autograd_and_its_limits_sit_inside_the_existing_bound():
    inp = E.softplus_inputs(4099)
    z, gy, gg = (inp[k].double() for k in ("z", "gy", "gg"))
    ex = E.softplus_exact_mask(inp["z"])
    fwd = lambda t: torch.nn.functional.softplus(t, beta=E.SP_BETA, threshold=E.SP_THR)
    y, gx, d_m, d_x = _second_order(fwd, z, gy, gg)
    got = [E.softplus_ref(0, inp)[0], E.softplus_ref(1, inp)[0]] + E.softplus_ref(2, inp)
    # (torch's float64 predicate z * beta > threshold differs from the fp32 one only AT the straddling neighbours)
    near = (inp["z"] - 0.2).abs() < 1e-6
    for (ref, lim), t, what in zip(got, (y, gx, d_m, d_x), ("y", "gz", "d_gy", "d_z")):
        keep = ~near
        assert float((ref - t)[keep].abs().max()) <= 1e-12 * max(1.0, float(t.abs().max())), what
        # the derived limit never exceeds what the existing test allows (rtol 5e-6, atol 2e-6 against float64)
        assert bool((lim <= 5e-6 * ref.abs() + 2e-6).all()), what
        assert bool((lim[~ex] > 0).all()), what


# ---- closed forms against float64 autograd, and conditioning ---------------------------------------------------------
@pytest.mark.parametrize("w0", E.SINE_W0)
def test_sine_reference(w0):
    for n in E.SINE_N:
        inp = E.sine_inputs(n, w0)
        assert float(inp["x"].abs().max()) <= 1.0
        for order in (0, 1, 2):
            _conditioned(f"sine n={n} w0={w0} order {order}", E.sine_ref(order, inp, w0, F64), E.sine_ref(order, inp, w0, F32))
    inp = E.sine_inputs(257, w0)
    u = (inp["x"] * torch.tensor(w0, dtype=F32)).double()          # the fp32 product is the point of differentiation
    y, gx, d_m, d_x = _second_order(torch.sin, u, inp["gy"].double(), inp["gg"].double() * w0)
    _close(E.sine_ref(0, inp, w0, F64)[0], y, "order 0")
    _close(E.sine_ref(1, inp, w0, F64)[0], gx * w0, "order 1")
    r0, r1 = E.sine_ref(2, inp, w0, F64)
    _close(r0, d_m, "order 2 d/d gy")
    _close(r1, d_x * w0, "order 2 d/d x")


@pytest.mark.parametrize("dim,n_freq", E.POSENC_SHAPES)
def test_posenc_reference(dim, n_freq):
    freqs = E.posenc_freqs(n_freq)
    assert all(np.float32(f) == f and np.log2(f) == int(np.log2(f)) for f in freqs)
    for n in E.POSENC_N:
        inp = E.posenc_inputs(n, dim, n_freq)
        for f in freqs:       # exact fp32 arguments
            assert torch.equal((inp["c"] * torch.tensor(f, dtype=F32)).double(), inp["c"].double() * f)
        for order in (0, 1, 2):
            _conditioned(f"posenc n={n} D={dim} L={n_freq} order {order}", E.posenc_ref(order, inp, freqs, F64),
                         E.posenc_ref(order, inp, freqs, F32))
        y, gx, d_m, d_x = _second_order(lambda c: E.posenc_fwd(c, freqs), inp["c"].double(), inp["g"].double(),
                                        inp["gg"].double())
        _close(E.posenc_ref(0, inp, freqs, F64)[0], y, "order 0")
        _close(E.posenc_ref(1, inp, freqs, F64)[0], gx, "order 1")
        r0, r1 = E.posenc_ref(2, inp, freqs, F64)
        _close(r0, d_m, "order 2 d/d g")
        _close(r1, d_x, "order 2 d/d c")
    if n_freq == 16:
        assert max(freqs) == 2.0 ** 15


@pytest.mark.parametrize("W", E.ROWNORM_W)
def test_rownorm_reference(W):
    eps = E.f32(E.ROWNORM_EPS)
    for rows in E.ROWNORM_ROWS:
        inp = E.rownorm_inputs(W, rows)
        k = E.rownorm_const_row(rows)
        if k is not None:
            assert float(inp["y"][k].std(unbiased=False)) == 0.0 and float(inp["y"][k, 0]) != 0.0
        refs = [E.rownorm_ref(o, inp, E.ROWNORM_EPS, F64) for o in (0, 1, 2)]
        if W == 1:
            for r in refs:
                for t in r:
                    assert float(t.abs().max()) == 0.0
            continue
        for order in (0, 1, 2):
            _conditioned(f"rownorm W={W} rows={rows} order {order}", refs[order], E.rownorm_ref(order, inp, E.ROWNORM_EPS, F32),
                         rowwise=True)
        y, gx, d_m, d_x = _second_order(lambda t: E.rownorm_fwd(t, eps), inp["y"].double(), inp["g"].double(),
                                        inp["gg"].double())
        for a, b, what in zip((refs[0][0], refs[1][0], refs[2][0], refs[2][1]), (y, gx, d_m, d_x),
                              ("order 0", "order 1", "order 2 d/d g", "order 2 d/d y")):
            for r in range(rows):       # row by row: the constant row's 1 / sqrt(eps) must not set the scale
                _close(a[r], b[r], (what, r)) if float(b[r].abs().max()) > 0 else _close(a[r] + 1.0, b[r] + 1.0, (what, r))


@pytest.mark.parametrize("beta", E.HEAD_BETA)
def test_sdf_head_reference(beta):
    for n in E.HEAD_N:
        for cols in E.HEAD_COLS:
            inp = E.head_inputs(n, cols)
            s = inp["zl"][:, 0]
            if n >= len(E.HEAD_SPECIAL):
                assert s[:len(E.HEAD_SPECIAL)].tolist() == [float(np.float32(v)) for v in E.HEAD_SPECIAL]
            r64, r32 = E.head_fwd_ref(s, beta, F64), E.head_fwd_ref(s, beta, F32)
            _conditioned(f"sdf_head n={n} cols={cols} beta={beta} fwd", r64, r32)
            sdf, c, denom = (t.float() for t in r64)
            for cb in (None, inp["cb"]):
                _conditioned(f"sdf_head n={n} cols={cols} beta={beta} bwd cb={'yes' if cb is not None else 'no'}",
                             E.head_bwd_ref(inp["d_out"][:, 0], sdf, c, denom, cb, F64),
                             E.head_bwd_ref(inp["d_out"][:, 0], sdf, c, denom, cb, F32))
    # c = d sdf / d s with rho held constant (density under no_grad), as tests/helpers.py mlp_fp64 composes it
    s = E.head_inputs(257, 2)["zl"][:, 0].double().requires_grad_(True)
    b = E.f32(beta)
    rho = ((1.0 / b) * (0.5 + 0.5 * torch.sign(s) * torch.expm1(-s.abs() / b))).detach()
    sdf = torch.tanh(s / (2.0 + rho))
    (ds,) = torch.autograd.grad(sdf.sum(), s, create_graph=True)
    r = E.head_fwd_ref(s.detach().float(), beta, F64)
    _close(r[0], sdf.detach(), "sdf")
    _close(r[1], ds.detach(), "c")
    # the c-bar term: d c / d s = -2 sdf c / denom
    (dc,) = torch.autograd.grad(ds.sum(), s)
    _close(-2.0 * r[0] * r[1] / r[2], dc, "d c / d s")


def test_weight_norm_reference():
    layers = E.wn_inputs()
    assert len(layers) == E.WN_LAYERS and {v.shape[1] for v, _, _ in layers} == set(E.WN_COLS)
    sel = [i for i in range(E.WN_LAYERS) if i % 3 != 1]
    assert {layers[i][0].shape[1] for i in sel} == set(E.WN_COLS)
    _conditioned("weight_norm", E.wn_ref(layers, sel, F64), E.wn_ref(layers, sel, F32))
    vs = [v.double().requires_grad_(True) for v, _, _ in layers]
    gs = [g.double().requires_grad_(True) for _, g, _ in layers]
    ws = [torch._weight_norm(v, g, 0) for v, g in zip(vs, gs)]
    loss = sum((ws[i] * layers[i][2].double()).sum() for i in sel)
    gv = torch.autograd.grad(loss, [vs[i] for i in sel], retain_graph=True)
    gg = torch.autograd.grad(loss, [gs[i] for i in sel])
    w, rv, rg = E.wn_ref(layers, sel, F64)
    _close(w, torch.cat([t.detach().reshape(-1) for t in ws]), "w")
    _close(rg, torch.cat([t.reshape(-1) for t in gg]), "grad_g")
    a, b = rv, torch.cat([t.reshape(-1) for t in gv])
    assert float((a - b).abs().max()) <= 1e-10 * float(b.abs().max())


@pytest.mark.parametrize("max_norm,gscale", [(None, 1.0), (1.0, 3.0), (1.0, 1e-3)])
def test_adam_reference_matches_torch_in_float64(max_norm, gscale):
    ps, gs = E.adam_inputs(gscale)
    assert [p.numel() for p in ps] == E.ADAM_NUMEL
    ref = E.adam_ref(ps, gs, max_norm)
    h = {k: E.f32(v) for k, v in E.ADAM_HYPER.items()}
    qs = [torch.nn.Parameter(p.double().clone()) for p in ps]
    opt = torch.optim.Adam(qs, lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"])
    for it in range(E.ADAM_STEPS):
        for q, g in zip(qs, gs[it]):
            q.grad = g.double().clone()
        if max_norm:
            total = torch.nn.utils.clip_grad_norm_(qs, max_norm=max_norm)
            assert abs(float(total) - ref[it][2]) <= 1e-12 * ref[it][2]
            assert (ref[it][2] > max_norm) == (gscale > 1)       # clipping active / inactive as the case says
        opt.step()
        for q, p, g in zip(qs, ref[it][0], ref[it][1]):
            assert float((q.detach() - p).abs().max()) <= 1e-12
            assert float((q.grad - g).abs().max()) <= 1e-9 * max(1.0, float(g.abs().max()))


def test_loss_cases():
    for n in E.LOSS_N:
        for m in E.LOSS_M:
            inp = E.loss_inputs(n, m)
            assert float(inp["sdf"].max()) == 1.0 and float(inp["sdf"].min()) == -1.0
            surface = inp["hit"] & inp["inside"]
            assert bool(surface.any()) and not bool(surface[:3].any())     # the sdf = +-1 rays feed the mask term
            for alpha in E.LOSS_ALPHA:
                terms, grads = E.loss_ref(inp, alpha)
                assert all(np.isfinite(v) for v in terms.values()) and all(bool(torch.isfinite(g).all()) for g in grads)
                assert grads[2].shape == (m, 3)
