"""The elementwise, reduction and copy kernels of csrc/hm_elem.hip, hm_loss.hip and hm_optim.hip at their branch edges,
order by order through the per-order helpers of ops.py, against the float64 closed forms of tests/elem_cases.py (checked on
CPU by tests/test_elem_cases_cpu.py).  Exact tests compare bits; the others hold each output to the limit its own
reference sets (elem_cases.limit) or to the bound the project documents.  Every comparison prints its error and limit.

Branch -> case:
  hm_softplus      float4 body / scalar tail / n < 4 / block edge: n = 1, 3, 4, 5, 1023, 1024, 1025, 4099; the scalar
                   launch for misaligned pointers: views buf[k:], k = 1, 2, 3; bz > threshold: fp32 neighbours of 0.2
  hm_colsum*       remainder loop only: M = 1, 7; 8-row body + remainder: M = 9, 33, 65; one slab / two: M = 32, 33;
                   ld > N: every case again as a view; M = 0, N = 0; slabs > 65535: M = 2 097 121; 17 items: two tables;
                   items of very different M in one table: the 17-item call
  hm_colsum*_det   512 slabs of 32 rows / 33-row slabs: M = 16384, 16385; two tables sharing one workspace: 17 items
  hm_rownorm       lanes without element: W = 1, 2, 7; all 16 slots: W = 127, 128; fewer rows than a block's 32, block edge:
                   rows = 1, 31, 32, 33; constant row; refusals W = 129, 1-D input
  hm_posenc        dim = 1, 3, 4, 64, n_freq = 1, 6, 8, 16; strided c and g; refusals dim = 65, n_freq = 17
  hm_sdf_head      s = 0, saturated tanh (|s| = 50, 1e4), cols = 1, cb given / NULL, block edge n cols = 255, 257
  hm_copy2d_f32    every combination of cols % 4, ld % 4 and pointer alignment on both sides (dcopy_), take_block, cat_rows_
  hm_weight_norm   cols = 1, 255, 256, 257, 1000 (one pass of 256 threads, its edge, four passes), 32 layers, 33 refused
  hm_adam_step*    scalar path of grad_sqnorm_kernel / adam_update_kernel: views at element offset 1; numel = 8191 .. 8195,
                   16385 around the 8192-element chunk
  hm_idr_loss*     n = 1023, 1024, 1025 around the 1024 lanes, m = 0, 1, 1025, alpha = 50, 1600, sdf = +-1
"""
import numpy as np
import pytest
import torch

import elem_cases as E

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"


def _ops():
    from hashmodnffbanks_idr_amd import ops
    return ops


def _cuda(inp):
    return {k: v.to(DEV) for k, v in inp.items()}


def _offset_view(t, k):
    """the values of t as a contiguous view that starts k floats into its storage (k = 0: an aligned clone)"""
    t = t.to(DEV)
    if k == 0:
        v = t.clone()
    else:
        buf = torch.zeros(t.numel() + k, dtype=F32, device=DEV)
        v = buf[k:].view(t.shape)
        v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * k) % 16
    return v


# =====================================================================================================================
# exact: column sums
# =====================================================================================================================
COLSUM_KINDS = ["colsum", "colsum_into", "colsum_into_multi"]


def _colsum_run(ops, kind, x, out0):
    if kind == "colsum":
        return ops.colsum(x)
    out = out0.clone()
    if kind == "colsum_into":
        ops.colsum_into(x, out)
    else:
        ops.colsum_into_multi([(x, out)])
    return out


def _colsum_check(ops, kind, det, M, N, view):
    x = E.colsum_ints(M, N).to(DEV)
    if view:
        x = E.colsum_as_view(x)
        assert x.stride(-1) == 1 and (M == 0 or x.storage_offset() == 1)
    out0 = E.colsum_ints(1, N, 5)[0].to(DEV)
    ref = E.colsum_ref(x, None if kind == "colsum" else out0).to(F32)
    with ops.deterministic(det):
        got = _colsum_run(ops, kind, x, out0)
        again = _colsum_run(ops, kind, x, out0) if det else got
    assert torch.equal(got.cpu(), ref), (kind, det, M, N, view, (got.cpu() - ref).abs().max().item())
    assert torch.equal(got, again), (kind, M, N, view)


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("kind", COLSUM_KINDS)
def test_colsum_small_shapes_exact(kind, det):
    """integers of [-4, 4]: every summation order gives the exact int64 sum.  M = 1, 7: the remainder loop alone;
    M = 8, 9, 31, 33, 65: the 8-row body with and without remainder, one and several 32-row slabs; N = 256 / 257: one
    block of columns / two; (0, 4): no rows.  Each contiguous and as a view with ld = N + 3 at column 1 (pads = 7)."""
    ops = _ops()
    for M, N in E.COLSUM_SMALL:
        for view in (False, True):
            _colsum_check(ops, kind, det, M, N, view)


@pytest.mark.parametrize("kind", COLSUM_KINDS)
def test_colsum_atomic_slab_resize_exact(kind):
    """M = 2 097 121: 65536 slabs of 32 rows do not fit gridDim.y, the slab height becomes 33"""
    M, N = E.COLSUM_ATOMIC_BIG
    _colsum_check(_ops(), kind, False, M, N, False)


@pytest.mark.parametrize("kind", COLSUM_KINDS)
@pytest.mark.parametrize("M,N", E.COLSUM_DET_EDGE)
def test_colsum_deterministic_slab_edge_exact(kind, M, N):
    """M = 16384: exactly 512 slabs of 32 rows; M = 16385: the first M with 33-row slabs (497 of them)"""
    for view in (False, True):
        _colsum_check(_ops(), kind, True, M, N, view)


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
def test_colsum_into_multi_17_items_exact(det):
    """one call of 17 items = two tables of 16 (the deterministic ones share one workspace): M = 2 097 121 (slab re-sizing
    from the table's largest M) next to M = 1 .. 1000, an M = 0 and an N = 0 item, every other x a strided view, and
    the last two items writing the two halves of ONE output"""
    ops = _ops()
    shapes = E.colsum_multi_shapes()
    xs = []
    for i, (M, N) in enumerate(shapes):
        x = E.colsum_ints(M, N, i).to(DEV)
        xs.append(E.colsum_as_view(x) if (i % 2 and N) else x)
    half = shapes[-1][1]
    init = [E.colsum_ints(1, N, 100 + i)[0].to(DEV) for i, (_, N) in enumerate(shapes[:-2])]
    init.append(E.colsum_ints(1, 2 * half, 200)[0].to(DEV))
    refs = [E.colsum_ref(x, o).to(F32) for x, o in zip(xs[:-2], init[:-1])]
    refs.append(torch.cat([E.colsum_ref(xs[-2]), E.colsum_ref(xs[-1])]).to(F32) + init[-1].cpu())

    def run():
        outs = [o.clone() for o in init]
        pairs = list(zip(xs[:-2], outs[:-1])) + [(xs[-2], outs[-1][:half]), (xs[-1], outs[-1][half:])]
        ops.colsum_into_multi(pairs)
        return outs
    with ops.deterministic(det):
        got = run()
        again = run() if det else got
    for i, (g, a, r) in enumerate(zip(got, again, refs)):
        assert torch.equal(g.cpu(), r), (i, shapes[i], (g.cpu() - r).abs().max().item())
        assert torch.equal(g, a), i


# =====================================================================================================================
# exact: copies
# =====================================================================================================================
@pytest.mark.parametrize("rows", E.COPY_ROWS)
def test_dcopy_every_vec4_combination_leaves_the_padding_alone(rows):
    """hm_copy2d_f32 moves float4s iff cols % 4 == 0, both row strides % 4 == 0 and both pointers are 16-byte aligned;
    the cases flip each of the five conditions on its own.  The destination is a sentinel-filled buffer compared WHOLE."""
    ops = _ops()
    n_vec = 0
    for cols, so, sp, do, dp in E.copy_cases(rows):
        sbuf = torch.arange(1, rows * (so + cols + sp) + 1, dtype=F32, device=DEV).reshape(rows, -1)
        src = sbuf[:, so:so + cols]
        dbuf = torch.full((rows, do + cols + dp), E.SENTINEL, dtype=F32, device=DEV)
        exp = dbuf.clone()
        exp[:, do:do + cols] = src
        dst = dbuf[:, do:do + cols]
        vec = E.copy_is_vec4(cols, so, sp, do, dp)
        assert vec == (cols % 4 == 0 and ops._ld(dst) % 4 == 0 and ops._ld(src) % 4 == 0
                       and dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0)
        n_vec += vec
        assert ops.dcopy_(dst, src) is dst
        assert torch.equal(dbuf, exp), (rows, cols, so, sp, do, dp)
    assert 0 < n_vec < len(E.copy_cases(rows))


def test_dcopy_1d_and_refusals():
    ops = _ops()
    for n in (5, 1028):
        for k in (0, 1):
            src = _offset_view(torch.arange(n, dtype=F32), k)
            dbuf = torch.full((n + 2,), E.SENTINEL, dtype=F32, device=DEV)
            ops.dcopy_(dbuf[1:1 + n], src)
            exp = torch.full((n + 2,), E.SENTINEL, dtype=F32, device=DEV)
            exp[1:1 + n] = src
            assert torch.equal(dbuf, exp)
    a, b = torch.zeros(4, 6, device=DEV), torch.zeros(4, 5, device=DEV)
    with pytest.raises(ValueError):
        ops.dcopy_(a, b)                                       # shape mismatch
    with pytest.raises(ValueError):
        ops.dcopy_(a[:, ::2], torch.zeros(4, 3, device=DEV))   # column-strided destination
    with pytest.raises(ValueError):
        ops.dcopy_(torch.zeros(4, 3, device=DEV), a[:, ::2])   # column-strided source
    with pytest.raises(ValueError):
        ops.dcopy_(a, a.double())                              # dtype


@pytest.mark.parametrize("box", [(2, 3, 1, 5), (0, 7, 4, 8), (6, 1, 12, 1), (1, 65, 0, None)])
def test_take_block_forward_backward_double_backward_match_slicing(box):
    ops = _ops()
    r0, nr, c0, nc = box
    rows = 70
    x0 = E.randn((rows, 16), 1, *box[:3]).to(DEV)
    sl = (slice(r0, r0 + nr), slice(c0, None if nc is None else c0 + nc))
    outs = []
    for fn in (lambda t: ops.take_block(t, r0, nr, c0, nc), lambda t: t[sl]):
        x = x0.clone().requires_grad_(True)
        y = fn(x)
        w = E.randn(tuple(y.shape), 2, *box[:3]).to(DEV).requires_grad_(True)
        (gx,) = torch.autograd.grad(y, x, grad_outputs=w, create_graph=True)
        r = E.randn((rows, 16), 3, *box[:3]).to(DEV)
        (gw,) = torch.autograd.grad(gx, w, grad_outputs=r)
        outs.append((y.detach(), gx.detach(), gw))
    assert outs[0][0].is_contiguous()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dim", [0, 1])
def test_cat_rows_matches_torch_cat(dim):
    ops = _ops()
    other = 6 if dim == 1 else 7
    parts = [E.randn((other, w) if dim == 1 else (w, other), w, dim).to(DEV) for w in (3, 4, 5)]
    ref = torch.cat(parts, dim)
    buf = torch.full((ref.shape[0] + 2, ref.shape[1] + 2), E.SENTINEL, dtype=F32, device=DEV)
    exp = buf.clone()
    exp[1:-1, 1:-1] = ref
    dst = buf[1:-1, 1:-1]
    assert ops.cat_rows_(dst, parts, dim) is dst
    assert torch.equal(buf, exp)
    out = torch.empty_like(ref)
    ops.cat_rows_(out, [parts[0], parts[1].t().contiguous().t(), parts[2]], dim)     # a column-major part is made row-major
    assert torch.equal(out, ref)


# =====================================================================================================================
# softplus
# =====================================================================================================================
@pytest.mark.parametrize("n", E.SOFTPLUS_N)
def test_softplus_orders_against_float64(n):
    """n = 1, 3: the scalar tail alone; 4, 5: one float4 with / without tail; 1023 / 1024 / 1025: one block's 1024
    elements; 4099: five blocks and a tail of 3.  Limits: elem_cases.softplus_ref (hm_common.h's 2e-9 for the logarithm
    term and 3e-7 relative for s1, s2, plus the roundings the number format adds), inside the existing test's
    rtol 5e-6 / atol 2e-6.  Where the fp32 product z * beta > threshold the outputs are z, gy, gg and 0 bit for bit."""
    ops = _ops()
    inp = E.softplus_inputs(n)
    d = _cuda(inp)
    ex = E.softplus_exact_mask(inp["z"])
    for order in (0, 1, 2):
        outs = ops._softplus_call(order, d["z"], d["gy"] if order else None, d["gg"] if order == 2 else None,
                                  E.SP_BETA, E.SP_THR)
        for k, (ref, lim) in enumerate(E.softplus_ref(order, inp)):
            got = outs[k].cpu()
            err = (got.double() - ref).abs()
            over = err - lim
            j = int(over.argmax())
            print(f"    softplus n={n} order {order} out{k}: max err {float(err.max()):.3e}; worst against its limit at "
                  f"z={float(inp['z'][j]):.9g}: err {float(err[j]):.3e} limit {float(lim[j]):.3e}")
            assert bool((err <= lim).all()), (order, k, float(inp["z"][j]), float(err[j]), float(lim[j]))
            assert bool((err <= 5e-6 * ref.abs() + 2e-6).all())
            exact = {(0, 0): inp["z"], (1, 0): inp["gy"], (2, 0): inp["gg"]}.get((order, k))
            if exact is not None:
                assert torch.equal(got[ex], exact[ex])
            else:
                assert bool((got[ex] == 0).all())
    if n >= 16:
        assert bool(ex.any())


@pytest.mark.parametrize("k", [1, 2, 3])
def test_softplus_on_a_misaligned_view_is_bit_identical_through_second_order(k):
    """ops.softplus on a contiguous view that starts 4, 8 or 12 bytes into its storage, with misaligned upstream
    gradients: the scalar launch of hm_softplus gives the bits of the float4 launch on an aligned clone (value, first
    order, both second-order outputs).  n = 5: inside one thread's four; 1025, 4099: whole blocks and a tail."""
    ops = _ops()
    for n in (5, 1025, 4099):
        inp = E.softplus_inputs(n)

        def run(off):
            z = _offset_view(inp["z"], off).requires_grad_(True)
            w = _offset_view(inp["gy"], off).requires_grad_(True)
            r = _offset_view(inp["gg"], off)
            y = ops.softplus(z, E.SP_BETA, E.SP_THR)
            (g,) = torch.autograd.grad(y, z, grad_outputs=w, create_graph=True)
            d_z, d_w = torch.autograd.grad(g, (z, w), grad_outputs=r)
            return y.detach(), g.detach(), d_z, d_w
        for a, b, what in zip(run(k), run(0), ("y", "gz", "d_z", "d_gy")):
            assert torch.equal(a, b), (n, k, what)
        # and the per-order entry with only ONE pointer off: the output, the input or a gradient
        d = _cuda(inp)
        want = ops._softplus_call(2, d["z"], d["gy"], d["gg"], E.SP_BETA, E.SP_THR)
        for name in ("z", "gy", "gg"):
            args = dict(d)
            args[name] = _offset_view(inp[name], k)
            got = ops._softplus_call(2, args["z"], args["gy"], args["gg"], E.SP_BETA, E.SP_THR)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (n, k, name)


# =====================================================================================================================
# sine, positional encoding, row normalisation, sdf head, weight norm: limits from the reference (elem_cases.limit)
# =====================================================================================================================
@pytest.mark.parametrize("w0", E.SINE_W0)
def test_sine_orders_against_float64(w0):
    """n = 1, 255, 256, 257: one lane, one block less one, one block, two blocks.  u = x * w0 is the fp32 product in the
    reference too, so what is measured is the device sinf / cosf."""
    ops = _ops()
    for n in E.SINE_N:
        inp = E.sine_inputs(n, w0)
        d = _cuda(inp)
        for order in (0, 1, 2):
            outs = ops._sine_call(order, d["x"], d["gy"] if order else None, d["gg"] if order == 2 else None, w0)
            r64, r32 = E.sine_ref(order, inp, w0, F64), E.sine_ref(order, inp, w0, F32)
            for k in range(len(r64)):
                E.compare(f"sine n={n} w0={w0:g} order {order} out{k}", outs[k], r64[k], r32[k])


@pytest.mark.parametrize("dim,n_freq", E.POSENC_SHAPES)
def test_posenc_orders_against_float64(dim, n_freq):
    """(1, 1): one thread per row, one band; (3, 6) / (4, 8): the embedders' shapes; (4, 16): all 16 bands, arguments up to
    2^15 rad; (64, 2): the widest dim.  c is a column slice at an odd column of a wider row, g a strided view."""
    ops = _ops()
    freqs = E.posenc_freqs(n_freq)
    for n in E.POSENC_N:
        inp = E.posenc_inputs(n, dim, n_freq)
        W = inp["g"].shape[1]
        wide = torch.full((n, dim + 5), 9.0, dtype=F32, device=DEV)
        wide[:, 3:3 + dim] = inp["c"].to(DEV)
        c = wide[:, 3:3 + dim]
        gbuf = torch.full((n, W + 2), 9.0, dtype=F32, device=DEV)
        gbuf[:, 1:1 + W] = inp["g"].to(DEV)
        g = gbuf[:, 1:1 + W]
        gg = inp["gg"].to(DEV)
        for order in (0, 1, 2):
            outs = ops._posenc_call(order, c, g if order else None, gg if order == 2 else None, freqs)
            r64, r32 = E.posenc_ref(order, inp, freqs, F64), E.posenc_ref(order, inp, freqs, F32)
            for k in range(len(r64)):
                E.compare(f"posenc n={n} D={dim} L={n_freq} order {order} out{k}", outs[k], r64[k], r32[k])
        out0 = ops._posenc_call(0, c, None, None, freqs)[0]
        assert torch.equal(out0[:, :dim], c) and torch.equal(out0[:, dim:2 * dim], c)


def test_posenc_refusals():
    ops = _ops()
    with pytest.raises(ValueError):
        ops._posenc_call(0, torch.zeros(2, 65, device=DEV), None, None, (1.0,))
    with pytest.raises(ValueError):
        ops._posenc_call(0, torch.zeros(2, 3, device=DEV), None, None, E.posenc_freqs(17))
    assert ops._posenc_call(0, torch.zeros(2, 64, device=DEV), None, None, E.posenc_freqs(16))[0].shape == (2, 2176)


@pytest.mark.parametrize("W", E.ROWNORM_W)
def test_rownorm_orders_against_float64_row_by_row(W):
    """W = 1, 2, 7: lanes of the row's eight without an element; 8, 9: one element per lane, a second on lane 0; 56: the
    embedders' width; 127, 128: all 16 register slots (the last one empty on lane 7 at 127).  rows = 1, 31: less than one
    block's 32 rows (the idle lanes stay in the shuffles); 32, 33, 100: a full block, the next one, four.  Unit-normal
    rows, mean-8 rows and one constant row (sigma = sqrt(eps)), each compared over ITS OWN reference maximum, so the
    constant row's 1 / sqrt(eps) gradients do not set the scale for the others.  W = 1: exact zeros everywhere."""
    ops = _ops()
    for rows in E.ROWNORM_ROWS:
        inp = E.rownorm_inputs(W, rows)
        d = _cuda(inp)
        for order in (0, 1, 2):
            outs = ops._rownorm_call(order, d["y"], d["g"] if order else None, d["gg"] if order == 2 else None,
                                     E.ROWNORM_EPS)
            r64 = E.rownorm_ref(order, inp, E.ROWNORM_EPS, F64)
            r32 = E.rownorm_ref(order, inp, E.ROWNORM_EPS, F32)
            for k in range(len(r64)):
                if W == 1:
                    assert bool((outs[k] == 0).all()) and float(r64[k].abs().max()) == 0.0
                else:
                    E.compare(f"rownorm W={W} rows={rows} order {order} out{k}", outs[k], r64[k], r32[k], rowwise=True)


def test_rownorm_refusals():
    ops = _ops()
    with pytest.raises(ValueError):
        ops._rownorm_call(0, torch.zeros(4, 129, device=DEV), None, None, E.ROWNORM_EPS)
    with pytest.raises(ValueError):
        ops.rownorm(torch.zeros(8, device=DEV))
    with pytest.raises(ValueError):
        ops.rownorm(torch.zeros(2, 2, 2, device=DEV))


@pytest.mark.parametrize("beta", E.HEAD_BETA)
def test_sdf_head_against_float64(beta):
    """column 0: s = 0, +-1e-8 ... +-1e4 (tanh saturated: sdf = +-1, c = 0), then values of width 0.3 and 0.01;
    cols = 1: every element is column 0; n cols = 255 / 257 / ...: block edges.  Forward: sdf, c, denom against
    helpers.mlp_fp64's expression; backward with cb = None and a random cb; columns >= 1 are bit-equal copies."""
    ops = _ops()
    for n in E.HEAD_N:
        for cols in E.HEAD_COLS:
            inp = E.head_inputs(n, cols)
            d = _cuda(inp)
            tag = f"sdf_head n={n} cols={cols} beta={beta}"
            out, sdf, c, denom = ops.sdf_head_fwd(d["zl"], beta)
            s = inp["zl"][:, 0]
            r64, r32 = E.head_fwd_ref(s, beta, F64), E.head_fwd_ref(s, beta, F32)
            for got, a, b, what in zip((sdf, c, denom), r64, r32, ("sdf", "c", "denom")):
                E.compare(f"{tag} {what}", got, a, b)
            assert torch.equal(out[:, 0], sdf) and torch.equal(out[:, 1:], d["zl"][:, 1:])
            assert bool((sdf.abs() <= 1).all()) and bool((c >= 0).all())
            if n >= len(E.HEAD_SPECIAL):       # s = 0 and s = +-1e4 (tanh of +-5000)
                assert float(sdf[0]) == 0.0 and sdf[11:13].tolist() == [1.0, -1.0] and c[11:13].tolist() == [0.0, 0.0]
            # the backward kernel reads fp32 (sdf, c, denom): hand it the rounded reference, refer to those same values
            sdf32, c32, den32 = (t.float() for t in r64)
            for cb in (None, inp["cb"]):
                zb = ops.sdf_head_bwd(d["d_out"], sdf32.to(DEV), c32.to(DEV), den32.to(DEV),
                                      None if cb is None else cb.to(DEV))
                b64 = E.head_bwd_ref(inp["d_out"][:, 0], sdf32, c32, den32, cb, F64)[0]
                b32 = E.head_bwd_ref(inp["d_out"][:, 0], sdf32, c32, den32, cb, F32)[0]
                E.compare(f"{tag} bwd cb={'given' if cb is not None else 'NULL'}", zb[:, 0], b64, b32)
                assert torch.equal(zb[:, 1:], d["d_out"][:, 1:])


def test_weight_norm_fold_32_layers_against_float64():
    """32 layers in one call (the by-value table's limit; 33 are refused) with cols = 1, 255, 256, 257, 1000: fewer columns
    than the block's 256 threads, the edge, four strided passes.  Backward with a gradient into two layers of three
    only.  Each of w, grad_v, grad_g is compared as ONE output over all layers: grad_v of a cols = 1 layer is a
    difference of two equal terms, whose own maximum is no scale."""
    ops = _ops()
    layers = E.wn_inputs()
    sel = [i for i in range(E.WN_LAYERS) if i % 3 != 1]
    vs = [v.to(DEV).requires_grad_(True) for v, _, _ in layers]
    gs = [g.to(DEV).requires_grad_(True) for _, g, _ in layers]
    ws = ops.weight_norm_fold(vs, gs)
    assert [tuple(w.shape) for w in ws] == [tuple(v.shape) for v in vs]
    loss = sum((ws[i] * layers[i][2].to(DEV)).sum() for i in sel)
    grads = torch.autograd.grad(loss, vs + gs, allow_unused=True)
    gv, gg = grads[:E.WN_LAYERS], grads[E.WN_LAYERS:]
    for i in range(E.WN_LAYERS):
        if i not in sel:       # no gradient arrived: None, or exact zeros
            assert gv[i] is None or not bool(gv[i].any())
            assert gg[i] is None or not bool(gg[i].any())
    got = [torch.cat([w.detach().reshape(-1) for w in ws]), torch.cat([gv[i].reshape(-1) for i in sel]),
           torch.cat([gg[i].reshape(-1) for i in sel])]
    r64, r32 = E.wn_ref(layers, sel, F64), E.wn_ref(layers, sel, F32)
    for g, a, b, what in zip(got, r64, r32, ("w", "grad_v", "grad_g")):
        E.compare(f"weight_norm_fold {what}", g, a, b)
    more = E.wn_inputs(E.WN_LAYERS + 1)
    with pytest.raises(ValueError):
        ops.weight_norm_fold([v.to(DEV) for v, _, _ in more], [g.to(DEV) for _, g, _ in more])


# =====================================================================================================================
# ClipAdam, IDR loss: the existing tests' limits against float64
# =====================================================================================================================
@pytest.mark.parametrize("max_norm,gscale", [(None, 1.0), (1.0, 3.0), (1.0, 1e-3)],
                         ids=["no_clip", "clip_active", "clip_inactive"])
def test_clip_adam_misaligned_views_against_float64(max_norm, gscale):
    """Parameters and gradients as views at element offset 1 of flat buffers (the scalar paths of grad_sqnorm_kernel and
    adam_update_kernel) next to the same set aligned (float4 paths), numel around the 8192-element chunk, 3 steps,
    against clip_grad_norm_ + Adam written out in float64 at the existing test's limits (rtol 2e-6, atol 2e-7).
    Both paths update an element with the same arithmetic, so without clipping, and with clipping that does not bite
    (coefficient exactly 1), the two runs agree bit for bit.  The norm does NOT have one summation order: the float4 path
    gives a lane four adjacent elements per pass, the scalar path one element per pass, so the per-chunk partial sums
    differ in their last bits and with them the clip coefficient; with clipping active each run is therefore held to the
    float64 bound (norm: rtol 2e-6) and the two are not compared with each other."""
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    ps, gs = E.adam_inputs(gscale)
    ref = E.adam_ref(ps, gs, max_norm)

    def run(off):
        params = [torch.nn.Parameter(_offset_view(p, off)) for p in ps]
        for p in params:
            assert p.data_ptr() % 16 == 4 * off and p.is_contiguous()
        opt = ClipAdam(params, lr=E.ADAM_HYPER["lr"], betas=(E.ADAM_HYPER["b1"], E.ADAM_HYPER["b2"]),
                       eps=E.ADAM_HYPER["eps"], max_norm=max_norm)
        hist = []
        for it in range(E.ADAM_STEPS):
            for p, g in zip(params, gs[it]):
                p.grad = _offset_view(g, off)
            opt.step()
            for p in params:
                assert p.grad.data_ptr() % 16 == 4 * off
            hist.append(([p.detach().clone() for p in params], [p.grad.clone() for p in params],
                         float(opt.last_grad_norm)))
        return hist
    runs = {"misaligned": run(1), "aligned": run(0)}
    for name, hist in runs.items():
        for it, ((p_got, g_got, norm), (p_ref, g_ref, total)) in enumerate(zip(hist, ref)):
            ep = max(float((a.cpu().double() - b).abs().max()) for a, b in zip(p_got, p_ref))
            eg = max(float((a.cpu().double() - b).abs().max()) for a, b in zip(g_got, g_ref))
            print(f"    ClipAdam {name} step {it + 1}: max |d param| {ep:.3e}, max |d grad| {eg:.3e}"
                  + (f", norm {norm:.9g} vs {total:.9g} (rel {abs(norm - total) / total:.2e})" if max_norm else ""))
            if max_norm:
                np.testing.assert_allclose(norm, total, rtol=2e-6)
            for a, b in zip(p_got, p_ref):
                np.testing.assert_allclose(a.cpu().double().numpy(), b.numpy(), rtol=2e-6, atol=2e-7)
            for a, b in zip(g_got, g_ref):
                np.testing.assert_allclose(a.cpu().double().numpy(), b.numpy(), rtol=2e-6, atol=1e-9)
    if gscale <= 1.0:
        for (pa, ga, _), (pb, gb, _) in zip(runs["misaligned"], runs["aligned"]):
            for a, b in zip(pa + ga, pb + gb):
                assert torch.equal(a, b)


@pytest.mark.parametrize("alpha", E.LOSS_ALPHA)
@pytest.mark.parametrize("m", E.LOSS_M)
@pytest.mark.parametrize("n", E.LOSS_N)
def test_idr_loss_around_the_lane_count_against_float64(n, m, alpha):
    """n, m = 1023 / 1024 / 1025: every lane of the one workgroup holds one element, or lane 0 a second one; m = 0, 1;
    sdf = +-1 with alpha = 1600: logits of +-1600, exp overflows to inf on one side and the sigmoid is exactly 0 / 1.
    Limits of tests/test_loss_gpu.py, against float64.  The device-hyper entry gives the same bits."""
    from hashmodnffbanks_idr_amd.model import loss as L
    inp = E.loss_inputs(n, m)
    terms_ref, grads_ref = E.loss_ref(inp, alpha)
    leaves = [inp[k].to(DEV).requires_grad_(True) for k in ("rgb", "sdf", "grad")]
    out = {"rgb_values": leaves[0], "sdf_output": leaves[1], "grad_theta": leaves[2],
           "network_object_mask": inp["hit"].to(DEV), "object_mask": inp["inside"].to(DEV)}
    gt = inp["gt"].to(DEV)
    ours = L.idr_loss_terms(out, gt, E.LOSS_W_EIK, E.LOSS_W_MASK, alpha)
    (ours["loss"] * 1.7).backward()
    got = [t.grad.clone() if t.grad is not None else torch.zeros_like(t) for t in leaves]
    for k in ("loss", "rgb_loss", "eikonal_loss", "mask_loss"):
        v = float(ours[k].detach())
        print(f"    idr_loss n={n} m={m} alpha={alpha:g} {k}: {v:.9g} vs {terms_ref[k]:.9g} "
              f"(rel {abs(v - terms_ref[k]) / max(abs(terms_ref[k]), 1e-30):.2e})")
        np.testing.assert_allclose(v, terms_ref[k], rtol=3e-6, atol=1e-7, err_msg=k)
    for a, b, name in zip(got, grads_ref, ("d_rgb", "d_sdf", "d_grad")):
        assert bool(torch.isfinite(a).all()), name
        err = float((a.cpu().double() - b).abs().max()) if b.numel() else 0.0
        print(f"    idr_loss n={n} m={m} alpha={alpha:g} {name}: max |d| {err:.3e} (scale {float(b.abs().max()) if b.numel() else 0:.3e})")
        np.testing.assert_allclose(a.cpu().double().numpy(), b.numpy(), rtol=2e-5, atol=1e-9, err_msg=name)
    hyper = torch.tensor(L.loss_hyper_values(E.LOSS_W_EIK, E.LOSS_W_MASK, alpha), dtype=F32, device=DEV)
    for t in leaves:
        t.grad = None
    dev = L.idr_loss_terms(out, gt, hyper=hyper)
    (dev["loss"] * 1.7).backward()
    for k in ("loss", "rgb_loss", "eikonal_loss", "mask_loss"):
        assert torch.equal(dev[k].detach(), ours[k].detach()), k
    for t, a in zip(leaves, got):
        assert torch.equal(t.grad if t.grad is not None else torch.zeros_like(t), a)
