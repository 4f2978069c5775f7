"""The fused SDF kernels over the shape table of tests/sdf_shapes.py: widths, depths, skip layouts, output widths and
embedding widths the model can send them, each against a float64 evaluation of the same network (helpers.mlp_fp64) or,
where the kernels promise it, bit for bit against each other.

Entry points: hm_sdf_fwd (tile_points 4, 8, 16, 64 and 0 = auto), hm_sdf_fwd_emb, hm_sdf_fwd_bf16 / _emb_bf16,
hm_sdf_fwd_split / _emb_split (bf16x2, f16x2), the grad-path node mlp_grad.sdf_mlp and the device ray tracer."""
import ctypes as C

import numpy as np
import pytest
import torch

import params as P
import sdf_shapes as S
from helpers import make_implicit, mlp_fp64, pin

pytestmark = pytest.mark.gpu

FUSED = [c for c in S.CASES if c.fp32]
TILES = [4, 8, 16, 64, 0]
# batch sizes per tile size: ragged last tiles of each body; auto mode on both sides of kSdfMini, kSdfTiny, kSdfSmall;
# the 64-point body with two full rounds of 256 workgroups and a half-tile remainder
SIZES = {4: (1, 5, 1023), 8: (3, 13, 2047), 16: (7, 31, 4097), 64: (37, 64 * 256 * 2 + 5000),
         0: (1000, 1025, 2047, 2049, 8192, 8193)}
RTOL, ATOL = 1e-5, 2e-6          # what the fused-forward tests hold against the C oracle

_NETS = {}


def _net(case):
    if case.name not in _NETS:
        _NETS[case.name] = make_implicit(S.grid_config(case), case.hidden, case.fvs, 11, 0.3, 0.3, skip_in=case.skip)
        _NETS[case.name].eval()
    return _NETS[case.name]


def _points(n, seed):
    return torch.from_numpy(P.make_points(1000 + seed, n, -1.05, 1.05)).cuda()


def _grid(net):
    from hashmodnffbanks_idr_amd import ops
    emb = net._hash_embedder()
    return emb.desc, emb.table.detach(), emb.freq_encoding.B, ops.FRAC_MODES[emb.frac_mode]


def _embedding(net, x):
    from hashmodnffbanks_idr_amd import ops
    desc, table, B, frac = _grid(net)
    return ops.encode_fwd(desc, x, table, B, frac)


def _strided(e, pad=5):
    """e in a wider buffer (row stride E + pad), the gap filled with NaN"""
    buf = torch.full((e.shape[0], e.shape[1] + pad), float("nan"), device=e.device)
    buf[:, :e.shape[1]] = e
    return buf[:, :e.shape[1]]


def _fwd(net, x, tile, sdf_only=False):
    from hashmodnffbanks_idr_amd import ops
    desc, table, B, frac = _grid(net)
    return ops.sdf_fwd(desc, net.packed_weights(), x, table, B, frac, sdf_only=sdf_only, tile_points=tile)


def _rel_err(got, ref):
    """max |got - ref| / (atol / rtol + |ref|): <= rtol exactly when assert_allclose(rtol, atol) holds"""
    return float(((got.double() - ref).abs() / (ATOL / RTOL + ref.abs())).max())


def _close(got, ref, what):
    np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg=what)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", FUSED, ids=lambda c: c.name)
def test_fp32_forward_against_fp64(case, tile):
    """hm_sdf_fwd (full and sdf-only output) against float64; hm_sdf_fwd_emb on the same embedding rows (row stride
    E + 5, NaN in the gap) bit for bit: both run the same tile bodies on the same embedding values (the encode stage and
    hm_encode_fwd share one device implementation); with a forced tile size, every point's value is independent of its
    position in the batch and of its neighbours (bit for bit)"""
    from hashmodnffbanks_idr_amd import ops
    net = _net(case)
    assert net._fusable()
    pk = net.packed_weights()
    want = S.layers(case)
    assert pk.desc.n_layers == len(want)
    for l, ly in enumerate(want):
        d = pk.desc.layer[l]
        assert (d.out_dim, d.n_tiles, d.post_div_sqrt2) == (ly["out"], ly["n_tiles"], ly["post_div_sqrt2"])
        assert [d.seg_octets[s] for s in range(len(ly["segs"]))] == [(w + 7) // 8 for _, w in ly["segs"]]
    worst = 0.0
    for i, n in enumerate(SIZES[tile]):
        x = _points(n, i)
        with torch.no_grad():
            full = _fwd(net, x, tile)
            sdf = _fwd(net, x, tile, sdf_only=True)
            e = _embedding(net, x)
            ref, _ = mlp_fp64(net, e)
            emb_full = ops.sdf_fwd_emb(pk, _strided(e), tile_points=tile)
            emb_sdf = ops.sdf_fwd_emb(pk, _strided(e), sdf_only=True, tile_points=tile)
        assert full.shape == ref.shape
        err = max(_rel_err(full, ref), _rel_err(sdf, ref[:, 0]))
        print(f"{case.name} tile {tile} n {n}: max |d| / (|ref| + 0.2) = {err:.3e}")
        worst = max(worst, err)
        _close(full, ref, f"{case.name} tile {tile} n {n}: full output")
        _close(sdf, ref[:, 0], f"{case.name} tile {tile} n {n}: sdf-only output")
        assert torch.equal(emb_full, full), f"{case.name} tile {tile} n {n}: hm_sdf_fwd_emb differs from hm_sdf_fwd"
        assert torch.equal(emb_sdf, sdf), f"{case.name} tile {tile} n {n}: hm_sdf_fwd_emb (sdf-only) differs"
    pin(f"sdf_shapes:{case.name}:t{tile}", worst)
    if tile == 0:
        return
    n = 3001 if tile != 64 else 5000
    x = _points(n, 7)
    with torch.no_grad():
        full = _fwd(net, x, tile)
        for k in (1, 31, 63):
            assert torch.equal(_fwd(net, x[k:].contiguous(), tile), full[k:]), f"rows of x[{k}:] changed"
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).cuda()
        assert torch.equal(_fwd(net, x[perm].contiguous(), tile), full[perm]), "a permutation changed values"


@pytest.mark.parametrize("case", FUSED, ids=lambda c: c.name)
def test_fp32_output_window(case):
    """hm_sdf_fwd writes exactly the [n, out_cols] window of a strided output (out_stride = out_cols + 3, a spare row
    before and after); with a device-side count k < n it writes rows < k only, with the values of a call on k points"""
    from hashmodnffbanks_idr_amd import _lib
    net = _net(case)
    pk = net.packed_weights()
    desc, table, B, frac = _grid(net)
    L = _lib.lib()
    sentinel = -7.25e30
    for tile, n, k in ((64, 3000, 1234), (16, 3000, 1234), (8, 700, 333), (4, 300, 77), (0, 9000, 5000)):
        x = _points(n, tile + 1)
        for cols in (1, pk.out_dim):
            stride = cols + 3
            for n_dev in (None, k):
                buf = torch.full((n + 2, stride), sentinel, device="cuda")
                out = buf[1:]
                nd = torch.tensor([n_dev], dtype=torch.int32, device="cuda") if n_dev is not None else None
                _lib.check(L.hm_sdf_fwd(desc.handle, C.byref(pk.desc), _lib.dptr(x), n, _lib.dptr(table),
                                        _lib.dptr(B.contiguous()), _lib.dptr(out), stride, cols, frac, tile,
                                        _lib.dptr(nd), 0, _lib.stream_ptr(x)))
                torch.cuda.synchronize()
                m = n if n_dev is None else k
                with torch.no_grad():
                    want = _fwd(net, x[:m].contiguous(), tile, sdf_only=cols == 1)
                want = want.reshape(m, cols)
                what = f"{case.name} tile {tile} cols {cols} n_dev {n_dev}"
                assert torch.equal(buf[1:1 + m, :cols], want), what + ": window values"
                untouched = torch.ones_like(buf, dtype=torch.bool)
                untouched[1:1 + m, :cols] = False
                assert bool((buf[untouched] == sentinel).all()), what + ": wrote outside the window"


EMB_ONLY = [  # (E, hidden, skip_in, fvs): embedding widths no hash grid gives (E = 3 + 4L is always 3 mod 4)
    (5, (64,) * 4, (2,), 3),
    (17, (96,) * 6, (3,), 20),
    (130, (256,) * 8, (4,), 64),
]


def _plain_net(E, hidden, skip, fvs, seed=5, perturb=0.3):
    """ImplicitNetwork on raw inputs of width E (no embedder): the MLP alone, for hm_sdf_fwd_emb and the grad node"""
    from hashmodnffbanks_idr_amd.model.implicit_differentiable_renderer import ImplicitNetwork
    net = ImplicitNetwork(fvs, E, 1, list(hidden), True, 0.6, list(skip), True)
    sd = net.state_dict()
    for k, v in P.make_sdf_params(seed, E, hidden, 1 + fvs, tuple(skip), 0.6, perturb, 0.1).items():
        assert sd[k].shape == v.shape, (k, sd[k].shape, v.shape)
        sd[k] = torch.from_numpy(v)
    net.load_state_dict(sd)
    return net.cuda()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("width", EMB_ONLY, ids=lambda w: f"E{w[0]}")
def test_fp32_emb_widths_against_fp64(width, tile):
    from hashmodnffbanks_idr_amd import ops
    E, hidden, skip, fvs = width
    net = _plain_net(E, hidden, skip, fvs)
    pk = net.packed_weights()
    worst = 0.0
    for i, n in enumerate(SIZES[tile]):
        e = (torch.rand((n, E), generator=torch.Generator().manual_seed(i)) * 2 - 1).cuda() * 0.5
        with torch.no_grad():
            got = ops.sdf_fwd_emb(pk, _strided(e), tile_points=tile)
            ref, _ = mlp_fp64(net, e)
        worst = max(worst, _rel_err(got, ref))
        _close(got, ref, f"E {E} tile {tile} n {n}")
    print(f"E {E} tile {tile}: max |d| / (|ref| + 0.2) = {worst:.3e}")
    pin(f"sdf_shapes:emb{E}:t{tile}", worst)


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_16bit_kernels(case):
    """hm_sdf_fwd_bf16 / hm_sdf_fwd_split (bf16x2, f16x2) and their _emb forms on every case they accept, at the bounds of
    tests/test_bf16_gpu.py and tests/test_split_gpu.py; every case they refuse raises ValueError from the host-side check,
    and the model then runs its coarse scans in exact fp32 (coarse_mode 0)"""
    from hashmodnffbanks_idr_amd import ops
    net = _net(case)
    desc, table, B, frac = _grid(net)
    x = _points(64 * 300 + 41, 5)
    with torch.no_grad():
        ref32 = net.sdf(x)
        e = _embedding(net, x)
        ref64 = mlp_fp64(net, e)[0][:, 0]
    e32 = (ref32.double() - ref64).abs()
    # bf16 bounds of tests/test_bf16_gpu.py, calibrated on 512-wide layers.  Plain bf16 operands (8 significant bits) lose
    # more on networks with a hidden layer narrower than 256 or more than 8 of them: fewer terms per product average the
    # rounding out less and more layers compound it.  Measured there (w32, odd_tiles, ragged, depth15, no_skip): up to
    # 8.9e-3 max and 1.4e-3 mean, while the split kernels, on the same tile bodies, stay within 6e-6 of float64 - the
    # format's error, not a kernel defect.
    narrow = min(ly["out"] for ly in S.layers(case)[:-1] if not ly["post_div_sqrt2"]) < 256 \
        if len(S.layers(case)) > 1 else False
    bmax, bmean = (2e-2, 2e-3) if (narrow or len(case.hidden) > 8) else (5e-3, 5e-4)
    try:
        net.bf16_coarse_search = True
        pk = net.packed_weights()
        assert pk.has_bf16 and net.coarse_mode() == (1 if case.bf16 else 0)
        with torch.no_grad():
            if not case.bf16:
                with pytest.raises(ValueError):
                    ops.sdf_fwd_bf16(desc, pk, x, table, B, frac)
                with pytest.raises(ValueError):
                    ops.sdf_fwd_emb_bf16(pk, _strided(e))
            else:
                for form, got in (("bf16", ops.sdf_fwd_bf16(desc, pk, x, table, B, frac)),
                                  ("bf16 emb", ops.sdf_fwd_emb_bf16(pk, _strided(e)))):
                    d = (got - ref32).abs()
                    print(f"{case.name} {form}: vs fp32 max {d.max().item():.3e} mean {d.mean().item():.3e}")
                    assert torch.isfinite(got).all()
                    assert d.max().item() <= bmax and d.mean().item() <= bmean, form
        net.bf16_coarse_search = False
        for kind in ("bf16x2", "f16x2"):
            net.coarse_split = kind
            pk = net.packed_weights()
            assert pk.split == kind and net.coarse_mode() == (2 if case.split else 0)
            with torch.no_grad():
                if not case.split:
                    with pytest.raises(ValueError):
                        ops.sdf_fwd_split(desc, pk, x, table, B, frac)
                    with pytest.raises(ValueError):
                        ops.sdf_fwd_emb_split(pk, _strided(e))
                    continue
                for form, got in ((kind, ops.sdf_fwd_split(desc, pk, x, table, B, frac)),
                                  (kind + " emb", ops.sdf_fwd_emb_split(pk, _strided(e)))):
                    assert torch.isfinite(got).all()
                    esp = (got.double() - ref64).abs()
                    d = (got - ref32).abs()
                    print(f"{case.name} {form}: vs fp64 max {esp.max().item():.3e} mean {esp.mean().item():.3e}; "
                          f"fp32 kernel vs fp64 max {e32.max().item():.3e}; vs fp32 kernel max {d.max().item():.3e}")
                    if kind == "f16x2":
                        assert esp.max().item() <= max(8 * e32.max().item(), 2e-6), form
                        assert esp.mean().item() <= max(4 * e32.mean().item(), 2e-7), form
                        assert d.max().item() <= 1e-5, form
                    else:
                        assert esp.max().item() <= 2e-4 and esp.mean().item() <= 2e-5, form
    finally:
        net.bf16_coarse_search = False
        net.coarse_split = None


def _restated_fp64(net, x, prm):
    """ImplicitNetwork.forward + d sdf / d x on raw inputs in float64 autograd, from the parameters prm (weight_v,
    weight_g, bias per layer) - the reference's formulation, differentiable twice"""
    import torch.nn.functional as F
    h = x
    n_lin = net.num_layers - 1
    for l in range(n_lin):
        v, g, b = prm[f"lin{l}.weight_v"], prm[f"lin{l}.weight_g"], prm[f"lin{l}.bias"]
        W = g * v / v.norm(dim=1, keepdim=True)
        if l in net.skip_in:
            h = torch.cat([h, x], 1) / np.sqrt(2.0)
        h = h @ W.t() + b
        if l < n_lin - 1:
            h = F.softplus(h, beta=100, threshold=20)
    s = h[:, 0]
    with torch.no_grad():
        beta = net.dencity_net.beta.detach().abs().double() + 1e-4
        rho = (1.0 / beta) * (0.5 + 0.5 * torch.sign(s) * torch.expm1(-s.abs() / beta))
    sdf = torch.tanh(s / (2.0 + rho))
    (gr,) = torch.autograd.grad(sdf.sum(), x, create_graph=True)
    return torch.cat([sdf.unsqueeze(1), h[:, 1:]], 1), gr


def _loss(out, gr, x, R):
    return ((gr.norm(2, dim=1) - 1) ** 2).mean() + 0.01 * (out * R).sum() + (gr * x).sum()


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_grad_path_against_fp64_autograd(case):
    """forward_with_gradient (mlp_grad.sdf_mlp for at most one skip, the generic route for two) against float64
    autograd: the output, d sdf / d x, and the gradients of the eikonal-style loss of
    test_fused_mlp_grad_node_matches_generic_autograd with respect to x and every parameter (2e-5 of each's scale)"""
    E = S.emb_width(case)
    net = _plain_net(E, case.hidden, case.skip, case.fvs, seed=17, perturb=0.5)
    net.train()
    n = 300
    x0 = (torch.rand((n, E), generator=torch.Generator().manual_seed(1)) * 2 - 1) * 0.5
    R = torch.randn((n, 1 + case.fvs), generator=torch.Generator().manual_seed(2)).cuda()
    assert net.use_fused_mlp_grad
    x = x0.clone().cuda()
    out, gr = net.forward_with_gradient(x)
    _loss(out, gr[:, 0, :], x, R).backward()
    got = (out.detach(), gr[:, 0, :].detach(), x.grad, {k: p.grad for k, p in net.named_parameters() if p.grad is not None})

    prm = {k: p.detach().double().requires_grad_(True) for k, p in net.named_parameters() if k.startswith("lin")}
    x64 = x0.double().cuda().requires_grad_(True)
    out64, gr64 = _restated_fp64(net, x64, prm)
    _loss(out64, gr64, x64, R.double()).backward()

    def close(a, b, what):
        scale = b.abs().max().item() + 1e-12
        err = (a.double() - b).abs().max().item()
        assert err <= 2e-5 * scale, (case.name, what, err, scale)
        return err / scale

    worst = max(close(got[0], out64.detach(), "out"), close(got[1], gr64.detach(), "gradient"),
                close(got[2], x64.grad, "x.grad"))
    assert set(got[3]) == set(prm), set(got[3]) ^ set(prm)
    for k in prm:
        worst = max(worst, close(got[3][k], prm[k].grad, k))
    print(f"{case.name} ({'fused node' if len(case.skip) <= 1 else 'generic route'}): worst error / scale {worst:.3e}")


def test_lds_boundary_falls_back_to_the_generic_route():
    """L = 27 fuses at 512-wide layers (test_fp32_forward_against_fp64); L = 28 is over the 160 KB tile: the module's
    no-grad forward takes the layer-by-layer route instead of raising, on batches on both sides of kSdfSmall"""
    c = S.BY_NAME["L28"]
    net = _net(c)
    assert not net._fusable()
    with pytest.raises(ValueError, match="160 KB"):
        _fwd(net, _points(9000, 1), 0)
    for n in (100, 9000):
        x = _points(n, 2)
        with torch.no_grad():
            sdf = net.sdf(x)
            full = net(x)
            ref, _ = mlp_fp64(net, _embedding(net, x))
        _close(full, ref, f"L28 n {n}: full output")
        _close(sdf, ref[:, 0], f"L28 n {n}: sdf-only output")


def _trace(net, tile, dev_tracer, mode="train", n_rays=512, seed=4):
    from hashmodnffbanks_idr_amd.model.ray_tracing import RayTracing
    cam, dirs = P.make_rays(seed, n_rays)
    om = np.random.RandomState(seed).uniform(0, 1, n_rays) < 0.7
    net.sdf_tile_points = tile
    rt = RayTracing(1.0, 5.0e-5, 0.5, 3, 10, 100, 8).cuda()
    rt.train(mode == "train")
    rt.use_device_tracer = dev_tracer
    rt.steps_override = torch.from_numpy(np.random.RandomState(seed + 1).uniform(0, 1, 100).astype(np.float32))
    try:
        with torch.no_grad():
            res = rt(sdf=net.sdf, cam_loc=torch.from_numpy(cam).cuda(), object_mask=torch.from_numpy(om).cuda(),
                     ray_directions=torch.from_numpy(dirs).cuda())
    finally:
        net.sdf_tile_points = 0
    return res


@pytest.mark.parametrize("tile", [16, 64, 0])
@pytest.mark.parametrize("name", ["w32", "ragged", "skip_2_5"])
def test_device_tracer_on_odd_shapes(name, tile):
    """RayTracing's device tracer (persistent march, secant, scan-secant kernels on the same tile bodies) against the
    generic tracer over the same network: bit for bit with a fixed tile size; with the tile size left to the library the
    bodies may differ per call (see tests/test_raytrace_gpu.py), so the masks and distances agree to a tolerance"""
    net = _net(S.BY_NAME[name])
    (p1, m1, d1), (p2, m2, d2) = _trace(net, tile, True), _trace(net, tile, False)
    print(f"{name} tile {tile}: {int(m1.sum())} hits of {m1.numel()} rays")
    if tile == 0:
        flips = int((m1 != m2).sum())
        close = (d1 - d2).abs() <= 1e-4 * (1.0 + d2.abs())
        assert flips <= max(1, m1.numel() // 200)
        assert 1.0 - float(close.float().mean()) <= 0.01
        return
    assert torch.equal(m1, m2)
    assert torch.equal(d1, d2), (d1 - d2).abs().max()
    assert torch.equal(p1, p2), (p1 - p2).abs().max()


@pytest.mark.parametrize("name", ["skip_last", "depth0"])
def test_tracer_with_refused_bf16_coarse_scans(name):
    """a network the bf16 kernel refuses still traces with bf16_coarse_search on: its coarse scans stay exact fp32, so
    the result is the fp32 tracer's, bit for bit"""
    net = _net(S.BY_NAME[name])
    ref = _trace(net, 64, True)
    try:
        net.bf16_coarse_search = True
        assert net.coarse_mode() == 0
        got = _trace(net, 64, True)
    finally:
        net.bf16_coarse_search = False
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
