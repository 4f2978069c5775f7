"""The hash-grid encoder kernels (csrc/hm_encode.hip, csrc/hm_encode_dx.hip) over the case table of
tests/encode_cases.py: level counts 1 ... 32, feature counts 1 ... 8, hand-made level tables, strided and misaligned
buffers, voxel-face points, ragged last waves.

Every comparison is array_equal (on the exact inputs of encode_cases.py, or where the project already asks for bits) or
a tolerance an existing test uses for the same quantity:
  reference-mode hash columns bit for bit, trilinear ones rtol 1e-5 / atol 1e-6, Fourier columns atol 1e-5,
  out[:, :3] == x, every forward kernel identical rows ......... test_encode_gpu.py::test_zordered_forward_vs_oracle
  scatter on real inputs 3e-5 * max|ref| (+ the sum check) ..... test_encode_gpu.py::test_zordered_table_backward_vs_oracle
  adjoint identity 1e-6 of the summed magnitudes ............... test_encode_gpu.py::test_encode_bwd_table_small_table_path
  input gradients 2e-4 * scale, scale > 0 ...................... test_encode_gpu.py::test_trilinear_input_gradient_first_and_second_order
  Fourier input gradients 2e-5 * scale, scale > 0 .............. test_encode_gpu.py::test_embedding_row_input_gradient_matches_torch_autograd
The case table's own claims (sizes, exactness of the integer inputs) are checked in test_encode_cases_cpu.py."""
import functools

import numpy as np
import pytest
import torch

import encode_cases as EC

pytestmark = pytest.mark.gpu

MODES = tuple(EC.MODES)
KINDS = ("lattice", "real")
NAN = float("nan")


def _api():
    from hashmodnffbanks_idr_amd import _lib, ops
    return _lib, ops


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


@functools.lru_cache(maxsize=None)
def _desc(name):
    _, ops = _api()
    g = EC.grid(name)
    return ops.GridDesc(g.res.tolist(), g.rows.tolist(), g.F)


def _inputs(name, kind, n):
    """(x, table, B) on the device: lattice points go with the integer table"""
    g = EC.grid(name)
    return _dev(EC.points(name, kind, n)), _dev(EC.table(name, kind == "lattice")), _dev(EC.fourier_B(g.L))


def _fwd(name, x, table, B, fm, ws=None, ws_bytes=0, out=None, stride=None):
    """hm_encode_fwd (ws is None) / hm_encode_fwd_ws into `out` (or a fresh contiguous tensor); B None: hash columns"""
    _lib, _ = _api()
    g, desc, n = EC.grid(name), _desc(name), x.shape[0]
    width = g.E if B is not None else g.L * g.F
    if out is None:
        out, stride = torch.empty((n, width), dtype=torch.float32, device=x.device), width
    if ws is None:
        _lib.check(_lib.lib().hm_encode_fwd(desc.handle, _lib.dptr(x), n, _lib.dptr(table), _lib.dptr(B), _lib.dptr(out),
                                            stride, fm, _lib.stream_ptr(x)))
    else:
        _lib.check(_lib.lib().hm_encode_fwd_ws(desc.handle, _lib.dptr(x), n, _lib.dptr(table), _lib.dptr(B),
                                               _lib.dptr(out), stride, fm, _lib.dptr(ws), ws_bytes, _lib.stream_ptr(x)))
    return out


def _workspace(name, n):
    """(buffer, full size, offset of the slab ids) of the z-ordered forward's workspace"""
    _lib, _ = _api()
    need = _lib.check(_lib.lib().hm_encode_workspace_bytes(_desc(name).handle, n))
    assert need > 0
    return torch.empty(need, dtype=torch.uint8, device="cuda"), need, need - 2 * ((n + 1) & ~1)


def _check_rows(out, ref, x, g, mode, kind, hash_only, what):
    """the criteria of test_zordered_forward_vs_oracle; on exact (lattice) inputs the hash columns are compared bit for
    bit in both modes"""
    nf = 3 + 2 * g.L
    feats, rfeats = (out if hash_only else out[:, nf:]), ref[:, nf:]
    assert feats.shape == rfeats.shape, what
    if mode == "reference" or kind == "lattice":
        assert torch.equal(feats, rfeats), f"{what}: hash columns differ from the oracle"
    else:
        bad = (feats - rfeats).abs() > 1e-6 + 1e-5 * rfeats.abs()
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} hash features beyond rtol 1e-5 / atol 1e-6"
    if not hash_only:
        assert torch.equal(out[:, :3], x), what
        assert (out[:, 3:nf] - ref[:, 3:nf]).abs().max().item() <= 1e-5, what


# ---- 1. forward, the four F = 2 kernels -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", EC.Z_CASES + ("T_F2",))
def test_forward_f2_routes(name, mode, kind):
    """z cases at n = 131109: ops.encode_fwd (z-ordered kernel), hm_encode_fwd (sweep kernel), hm_encode_fwd_ws with
    exactly the slab offset as workspace size (z-ordered, slabs recomputed from x) and with one byte less (falls back
    to the sweep kernel), and the first 131071 points through the tile kernel; T_F2: the tile kernel.  Every route
    against the oracle, full rows and hash_only, and the routes against each other bit for bit."""
    _, ops = _api()
    g, fm = EC.grid(name), EC.MODES[mode]
    n = EC.default_n(name)
    x, table, B = _inputs(name, kind, n)
    ref = _dev(EC.oracle_fwd(name, kind, n, mode))
    for hash_only in (False, True):
        Bh = None if hash_only else B
        routes = {"ops.encode_fwd": ops.encode_fwd(_desc(name), x, table, B, fm, hash_only=hash_only)}
        if name in EC.Z_CASES:
            ws, need, slab_off = _workspace(name, n)
            routes["hm_encode_fwd (sweep)"] = _fwd(name, x, table, Bh, fm)
            routes["hm_encode_fwd_ws, workspace == slab offset"] = _fwd(name, x, table, Bh, fm, ws, slab_off)
            routes["hm_encode_fwd_ws, one byte less"] = _fwd(name, x, table, Bh, fm, ws, slab_off - 1)
            routes["hm_encode_fwd_ws, full workspace"] = _fwd(name, x, table, Bh, fm, ws, need)
            below = _fwd(name, x[:EC.N_BELOW], table, Bh, fm)
            _check_rows(below, ref[:EC.N_BELOW], x[:EC.N_BELOW], g, mode, kind, hash_only, f"{name} tile kernel")
            routes["hm_encode_fwd, n = 131071 (tile)"] = torch.cat([below, routes["ops.encode_fwd"][EC.N_BELOW:]])
        first = None
        for what, out in routes.items():
            _check_rows(out, ref, x, g, mode, kind, hash_only, f"{name}/{mode}/{kind} {what}")
            first = out if first is None else first
            assert torch.equal(out, first), f"{what} and ops.encode_fwd must produce identical rows"


# ---- 2. forward window and strides ----------------------------------------------------------------------------
@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("hash_only", (False, True))
@pytest.mark.parametrize("name,route", [("Z3", "zorder"), ("Z3", "sweep"), ("T_F2", "tile")])
def test_forward_writes_only_its_window(name, route, hash_only, off):
    """rows of a NaN-filled [n + 2, stride] buffer, 16-byte aligned (off 0) or one float off: the [n, E] window equals
    the contiguous result bit for bit and nothing else is written - except, as include/hashmod.h documents, the pad
    floats up to ceil(E/4)*4 of the n rows, which the z-ordered kernel's vector path writes as zeros"""
    g, fm = EC.grid(name), EC.MODES["trilinear"]
    n = EC.default_n(name)
    x, table, B = _inputs(name, "real", n)
    Bh = None if hash_only else B
    E = g.L * g.F if hash_only else g.E
    ES = (E + 3) & ~3
    ws, need = (None, 0) if route != "zorder" else _workspace(name, n)[:2]
    want = _fwd(name, x, table, Bh, fm, ws, need)
    for stride in sorted({E, E + 1, ES, ES + 4}):
        flat = torch.full(((n + 2) * stride + 2,), NAN, dtype=torch.float32, device="cuda")
        assert flat.data_ptr() % 16 == 0
        buf = flat[off:off + (n + 2) * stride].view(n + 2, stride)
        _fwd(name, x, table, Bh, fm, ws, need, out=buf, stride=stride)
        what = f"{name} {route} stride {stride} (E {E}) offset {off}"
        assert torch.equal(buf[:n, :E], want), what
        zero_pad = ES - E if (route == "zorder" and stride % 4 == 0 and stride >= ES and off == 0) else 0
        assert bool((buf[:n, E:E + zero_pad] == 0).all()), what
        assert bool(torch.isnan(buf[:n, E + zero_pad:]).all()), f"{what}: wrote past the row"
        assert bool(torch.isnan(buf[n:]).all()), f"{what}: wrote past the last row"
        assert bool(torch.isnan(flat[:off]).all()) and bool(torch.isnan(flat[off + (n + 2) * stride:]).all()), what


# ---- 3. forward and scatter at F != 2 -------------------------------------------------------------------------
def _strided(d, lead=2, tail=3):
    """d as a column slice of a wider NaN-padded buffer (row stride > L*F, unit column stride)"""
    wide = torch.full((d.shape[0], lead + d.shape[1] + tail), NAN, dtype=torch.float32, device=d.device)
    wide[:, lead:lead + d.shape[1]] = d
    view = wide[:, lead:lead + d.shape[1]]
    assert view.stride(1) == 1 and (view.stride(0) > d.shape[1] or d.shape[0] == 1)
    return view


def _check_scatter(got, ref, kind, what):
    if kind == "lattice":
        assert torch.equal(got, ref), f"{what}: differs from the oracle on exact inputs"
    else:
        scale = ref.abs().max().item()
        assert scale > 0 and (got - ref).abs().max().item() <= 3e-5 * scale, what


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", EC.FN_CASES)
def test_fn_forward_and_scatter(name, mode):
    """encode_fwd_generic_kernel and the F loops of the atomic / small-table / sorted scatters"""
    _, ops = _api()
    g, fm, desc = EC.grid(name), EC.MODES[mode], _desc(name)
    nf = 3 + 2 * g.L
    for n in EC.fn_sizes(name):
        for kind in KINDS:
            what = f"{name}/{mode}/{kind} n={n}"
            x, table, B = _inputs(name, kind, n)
            ref = _dev(EC.oracle_fwd(name, kind, n, mode))
            full = ops.encode_fwd(desc, x, table, B, fm)
            feats = ops.encode_fwd(desc, x, table, B, fm, hash_only=True)
            _check_rows(full, ref, x, g, mode, kind, False, what)
            _check_rows(feats, ref, x, g, mode, kind, True, what + " hash_only")
            assert torch.equal(full[:, nf:], feats), what

            d = _dev(EC.d_feat(name, kind, n, mode))
            sref = _dev(EC.oracle_scatter(name, kind, n, mode))
            got = ops.encode_bwd_table(desc, x, d, fm, deterministic=False)
            _check_scatter(got, sref, kind, what + " scatter")
            det = ops.encode_bwd_table(desc, x, d, fm, deterministic=True)
            _check_scatter(det, sref, kind, what + " deterministic scatter")
            for deterministic in (False, True):
                fill = 3.0 if kind == "lattice" else 0.25
                acc = torch.full_like(got, fill)
                assert ops.encode_bwd_table(desc, x, d, fm, out=acc, deterministic=deterministic) is acc
                _check_scatter(acc - fill if kind == "real" else acc, sref + fill if kind == "lattice" else sref, kind,
                               what + f" accumulating scatter (deterministic={deterministic})")
                sd = ops.encode_bwd_table(desc, x, _strided(d), fm, deterministic=deterministic)
                _check_scatter(sd, sref, kind, what + f" strided d_feat (deterministic={deterministic})")
                if kind == "lattice" or deterministic:
                    assert torch.equal(sd, det if deterministic else got), what + " strided d_feat"
            if kind == "real":      # the scatter is the forward's adjoint (float64 sums)
                lhs = (feats.double() * d.double()).sum().item()
                rhs = (table.double() * got.double()).sum().item()
                mag = (feats.double().abs() * d.double().abs()).sum().item()
                assert abs(lhs - rhs) <= 1e-6 * mag, (what, lhs, rhs, mag)


@pytest.mark.parametrize("mode", MODES)
def test_module_with_four_features_per_level(mode):
    """MultiResHashGridMLP(max_points_per_level = 4) on the G_F4 level table: forward and table.grad against the oracle
    (exact inputs: bit for bit)"""
    from hashmodnffbanks_idr_amd.model.embeddings.hashGridEmbedding import MultiResHashGridMLP
    name, n = "G_F4", EC.N_SMALL
    g = EC.grid(name)
    emb = MultiResHashGridMLP(True, 3, 5, 4, 12, 4, 64, frac_mode=mode).cuda()
    assert emb.desc.res.tolist() == g.res.tolist() and emb.desc.rows.tolist() == g.rows.tolist()
    assert emb.embeddings_dim == g.E and tuple(emb.table.shape) == (g.total_rows, 4)
    x, table, B = _inputs(name, "lattice", n)
    with torch.no_grad():
        emb.table.copy_(table)
        emb.freq_encoding.B.copy_(B)
    ref = _dev(EC.oracle_fwd(name, "lattice", n, mode))
    y = emb(x)
    _check_rows(y.detach(), ref, x, g, mode, "lattice", False, f"module {mode}")
    d = _dev(EC.d_feat(name, "lattice", n, mode))
    d_out = torch.cat([torch.ones((n, 3 + 2 * g.L), device="cuda"), d], 1)
    (y * d_out).sum().backward()
    assert torch.equal(emb.table.grad, _dev(EC.oracle_scatter(name, "lattice", n, mode)))


# ---- 4. z-ordered scatter -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", EC.Z_CASES)
def test_zordered_scatter(name, mode, kind):
    """ops.encode_bwd_table at n = 131109 (zsort_pack_kernel + encode_bwd_table_zorder_kernel), contiguous and strided
    d_feat, and hm_encode_bwd_table on the same inputs (the atomic kernel): exact inputs bit for bit against the oracle
    and each other, real inputs by the criteria of test_zordered_table_backward_vs_oracle"""
    _lib, ops = _api()
    g, fm, desc = EC.grid(name), EC.MODES[mode], _desc(name)
    n = EC.N_BIG
    x, d = _dev(EC.points(name, kind, n)), _dev(EC.d_feat(name, kind, n, mode))
    ref = _dev(EC.oracle_scatter(name, kind, n, mode))
    atomic = torch.zeros_like(ref)
    _lib.check(_lib.lib().hm_encode_bwd_table(desc.handle, _lib.dptr(x), n, _lib.dptr(d), d.stride(0), _lib.dptr(atomic),
                                              fm, _lib.stream_ptr(x)))
    results = {"z-ordered": ops.encode_bwd_table(desc, x, d, fm, deterministic=False),
               "z-ordered, strided d_feat": ops.encode_bwd_table(desc, x, _strided(d), fm, deterministic=False),
               "atomic kernel": atomic}
    ref_sum, ref_abs = ref.double().sum().item(), ref.double().abs().sum().item()
    for what, got in results.items():
        what = f"{name}/{mode}/{kind} {what}"
        _check_scatter(got, ref, kind, what)
        if kind == "lattice":
            assert torch.equal(got, atomic), what
        assert abs(got.double().sum().item() - ref_sum) <= 1e-5 * ref_abs, what


# ---- 5. tracked scatters at F = 1, 3 and 8 --------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ("S_F1", "S_F3", "G_F8"))
def test_tracked_scatters(name, mode, kind):
    """hm_encode_bwd_table_tracked (two calls sharing the tracking buffers) and hm_encode_bwd_table_sorted_tracked:
    dense values against the oracle; listed rows unique, within cap, a superset of the oracle's non-zero rows and a
    subset of the rows some point reaches with a non-zero weight"""
    _lib, ops = _api()
    g, fm, desc = EC.grid(name), EC.MODES[mode], _desc(name)
    n, LF, total = EC.N_SMALL, g.L * g.F, g.total_rows
    x, d = _dev(EC.points(name, kind, n)), _dev(EC.d_feat(name, kind, n, mode))
    ref = _dev(EC.oracle_scatter(name, kind, n, mode))
    corners, skeys, perm, wts = ops.sorted_rows(desc, x, fm)
    assert corners == (1 if mode == "reference" else 8) and skeys.numel() == n * g.L * corners
    reach = set((skeys if wts is None else skeys[wts[perm] != 0]).tolist())
    nonzero = set(torch.nonzero(ref.abs().sum(1) > 0).flatten().tolist())
    assert nonzero <= reach
    cap = n * g.L * corners

    def buffers():
        return (torch.zeros((total, g.F), device="cuda"), torch.zeros((total + 31) // 32, dtype=torch.int32, device="cuda"),
                torch.zeros(1, dtype=torch.int32, device="cuda"), torch.full((cap,), -7, dtype=torch.int32, device="cuda"))

    def check(dense, bits, count, rows_buf, what):
        what = f"{name}/{mode}/{kind} {what}"
        _check_scatter(dense, ref, kind, what)
        cnt = int(count.item())
        listed = rows_buf[:cnt].tolist()
        assert cnt <= cap and len(set(listed)) == cnt, f"{what}: a row was listed twice"
        assert bool((rows_buf[cnt:] == -7).all()), what
        assert nonzero <= set(listed) <= reach, what
        claimed = torch.zeros(bits.numel() * 32, dtype=torch.bool, device="cuda")
        claimed[rows_buf[:cnt].long()] = True
        unpacked = ((bits.view(-1, 1) >> torch.arange(32, device="cuda", dtype=torch.int32)) & 1).bool().flatten()
        assert torch.equal(unpacked, claimed), f"{what}: claim bits and list disagree"

    dense, bits, count, rows_buf = buffers()
    half = n // 2
    for lo, hi in ((0, half), (half, n)):
        _lib.check(_lib.lib().hm_encode_bwd_table_tracked(
            desc.handle, _lib.dptr(x[lo:hi].contiguous()), hi - lo, _lib.dptr(d[lo:hi].contiguous()), LF,
            _lib.dptr(dense), fm, _lib.dptr(bits), _lib.dptr(count), _lib.dptr(rows_buf), cap, _lib.stream_ptr(x)))
    check(dense, bits, count, rows_buf, "hm_encode_bwd_table_tracked")

    ds = _strided(d)
    dense, bits, count, rows_buf = buffers()
    _lib.check(_lib.lib().hm_encode_bwd_table_tracked(
        desc.handle, _lib.dptr(x), n, _lib.dptr(ds), ds.stride(0), _lib.dptr(dense), fm, _lib.dptr(bits),
        _lib.dptr(count), _lib.dptr(rows_buf), cap, _lib.stream_ptr(x)))
    check(dense, bits, count, rows_buf, "hm_encode_bwd_table_tracked, strided d_feat")

    for what, dd in (("", d), (", strided d_feat", ds)):
        dense, bits, count, rows_buf = buffers()
        _lib.check(_lib.lib().hm_encode_bwd_table_sorted_tracked(
            desc.handle, _lib.dptr(skeys), _lib.dptr(perm), skeys.numel(), corners, _lib.dptr(dd), dd.stride(0),
            _lib.dptr(wts), _lib.dptr(dense), _lib.dptr(bits), _lib.dptr(count), _lib.dptr(rows_buf), cap,
            _lib.stream_ptr(x)))
        check(dense, bits, count, rows_buf, "hm_encode_bwd_table_sorted_tracked" + what)
        assert set(rows_buf[:int(count.item())].tolist()) == reach     # every run head with a non-zero weight is listed


# ---- 6. input-gradient kernels --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", EC.DX_CASES)
def test_trilinear_input_gradients(name, kind):
    """the run(...) harness of test_trilinear_input_gradient_first_and_second_order (values, d/dx, second-order d/dx,
    d/dtable, d/d(d_feat)) against autograd on the float64 restatement, at feature counts 2, 3, 4 and 8, with ragged
    last waves (n = 1, 7, 65) and with points on voxel faces and nodes (lattice), where the kernel and the reference
    must pick the same cell"""
    _, ops = _api()
    g, desc = EC.grid(name), _desc(name)
    for n in (1, 7, 65, EC.N_SMALL):
        gen = torch.Generator(device="cpu").manual_seed(11 + n)
        x0 = _dev(EC.points(name, kind, n))
        tab0 = (torch.rand((g.total_rows, g.F), generator=gen) - 0.5).cuda()
        m_out = torch.randn((n, g.L * g.F), generator=gen).cuda()       # stands for the MLP between features and sdf
        r_vec = torch.randn((n, 3), generator=gen).cuda()

        def run(features):
            x = x0.clone().requires_grad_(True)
            tab = tab0.clone().requires_grad_(True)
            m = m_out.clone().requires_grad_(True)
            e = features(x, tab)
            y = (e * m.to(e.dtype)).sum()
            (gx,) = torch.autograd.grad(y, x, create_graph=True)
            loss = (gx * r_vec.to(gx.dtype)).pow(2).sum() + 0.1 * e.pow(2).sum()
            loss.backward()
            return e.detach(), gx.detach(), x.grad, tab.grad, m.grad

        got = run(lambda x, tab: ops.hash_features(x, tab, desc, ops.FRAC_MODES["trilinear"]))
        ref = run(lambda x, tab: EC._trilinear_torch(x, tab, g))
        names = ("features", "d/dx", "loss d/dx (second order)", "loss d/dtable", "loss d/d(d_feat)")
        for what, a, b_ in zip(names, got, ref):
            scale = b_.abs().max().item()
            err = (a.double() - b_.double()).abs().max().item()
            print(f"trilinear {name}/{kind} n={n} {what}: max |d| {err:.3e} (scale {scale:.3e})")
            assert scale > 0 and err <= 2e-4 * scale, (name, kind, n, what)


@pytest.mark.parametrize("name", ("G_F4", "T_F2"))
def test_input_gradient_kernels_take_strided_rows(name):
    """d_feat_stride / out_stride > L*F in hm_encode_bwd_input (first and second order), hm_encode_jvp and
    hm_encode_bwd_table_jvp: the same bits as with contiguous rows (the first three sum in a fixed order; the atomic
    scatter of the fourth is exact on lattice points with integer a and d_feat: every term is a multiple of 2^-8 and a
    cell holds at most n * 3 * max(res) < 2^16), and hm_encode_jvp writes only its window"""
    _lib, _ = _api()
    lib = _lib.lib()
    g, desc = EC.grid(name), _desc(name)
    LF, p = g.L * g.F, _lib.dptr
    for kind, n in (("lattice", 65), ("real", EC.N_SMALL)):
        x, table, _ = _inputs(name, kind, n)
        d = _dev(EC.d_feat(name, kind, n, "trilinear"))
        a = torch.randint(-1, 2, (n, 3), generator=torch.Generator(device="cpu").manual_seed(n)).float().cuda()
        ds, st = _strided(d), _lib.stream_ptr(x)
        for second in (None, a):
            gx, gxs = torch.empty_like(x), torch.empty_like(x)
            _lib.check(lib.hm_encode_bwd_input(desc.handle, p(x), n, p(table), p(d), LF, p(second), p(gx), st))
            _lib.check(lib.hm_encode_bwd_input(desc.handle, p(x), n, p(table), p(ds), ds.stride(0), p(second), p(gxs), st))
            assert torch.equal(gx, gxs) and gx.abs().max().item() > 0
        out = torch.empty((n, LF), device="cuda")
        wide = torch.full((n + 1, LF + 5), NAN, device="cuda")
        _lib.check(lib.hm_encode_jvp(desc.handle, p(x), n, p(table), p(a), p(out), LF, st))
        _lib.check(lib.hm_encode_jvp(desc.handle, p(x), n, p(table), p(a), p(wide[:, 2:]), LF + 5, st))
        assert torch.equal(wide[:n, 2:2 + LF], out) and out.abs().max().item() > 0
        assert bool(torch.isnan(wide[:n, :2]).all()) and bool(torch.isnan(wide[:n, 2 + LF:]).all())
        assert bool(torch.isnan(wide[n:]).all())
        if kind == "lattice":
            assert n * 3 * int(g.res.max()) < 2 ** 16
            t1, t2 = torch.zeros_like(table), torch.zeros_like(table)
            _lib.check(lib.hm_encode_bwd_table_jvp(desc.handle, p(x), n, p(a), p(d), LF, p(t1), st))
            _lib.check(lib.hm_encode_bwd_table_jvp(desc.handle, p(x), n, p(a), p(ds), ds.stride(0), p(t2), st))
            assert torch.equal(t1, t2) and t1.abs().max().item() > 0


# ---- 7. Fourier input-gradient kernels ------------------------------------------------------------------------
def _fourier_reference(x, B, d_row, gg):
    """(gx, d_x, dd_row) by float64 autograd: gx = d(row . d_row)/dx, then the gradients of gg . gx"""
    xd = x.double().requires_grad_(True)
    dr = d_row.double().requires_grad_(True)
    (gx,) = torch.autograd.grad((EC.fourier_row_torch(xd, B) * dr).sum(), xd, create_graph=True)
    d_x, dd_row = torch.autograd.grad((gx * gg.double()).sum(), (xd, dr))
    return gx.detach(), d_x, dd_row


def _close(got, ref, what):
    scale = ref.abs().max().item()
    err = (got.double() - ref).abs().max().item()
    print(f"{what}: max |d| {err:.3e} (scale {scale:.3e})")
    assert scale > 0 and err <= 2e-5 * scale, what


@pytest.mark.parametrize("n_channels", (1, 8, 16, 17, 32))
def test_fourier_input_gradient_kernels(n_channels):
    """hm_fourier_bwd_input / hm_fourier_bwd_input_bwd called directly: channel counts around the 16 lanes per point,
    point counts that leave most of the last wave clamped, a strided d_row, each output of the second-order kernel on
    its own, and the zero fill of a dd_row wider than 3 + 2 n_channels"""
    _lib, _ = _api()
    lib = _lib.lib()
    L, w = n_channels, 3 + 2 * n_channels
    B = _dev(EC.fourier_B(L))
    for n in (1, 3, 5, EC.N_SMALL):
        gen = torch.Generator(device="cpu").manual_seed(100 * L + n)
        x = (torch.rand((n, 3), generator=gen) * 2 - 1).cuda()
        gg = torch.randn((n, 3), generator=gen).cuda()
        ld = w + 4
        d_wide = torch.full((n, ld), NAN, device="cuda")               # the kernels read the first w columns only
        d_wide[:, :w] = torch.randn((n, w), generator=gen).cuda()
        gx_ref, dx_ref, dd_ref = _fourier_reference(x, B, d_wide[:, :w], gg)
        what = f"fourier L={L} n={n}"
        st = _lib.stream_ptr(x)

        gx = torch.full((n + 1, 3), NAN, device="cuda")
        _lib.check(lib.hm_fourier_bwd_input(_lib.dptr(x), n, _lib.dptr(B), L, _lib.dptr(d_wide), ld, _lib.dptr(gx), st))
        _close(gx[:n], gx_ref, what + " gx")
        assert bool(torch.isnan(gx[n:]).all())

        def second(want_dx, want_dd, width, ld2):
            d_x = torch.full((n + 1, 3), NAN, device="cuda") if want_dx else None
            dd = torch.full((n + 1, ld2), NAN, device="cuda") if want_dd else None
            _lib.check(lib.hm_fourier_bwd_input_bwd(_lib.dptr(x), n, _lib.dptr(B), L, _lib.dptr(d_wide), ld, _lib.dptr(gg),
                                                    _lib.dptr(d_x), _lib.dptr(dd), ld2, width, st))
            if want_dx:
                _close(d_x[:n], dx_ref, what + f" d_x (dd_row {'too' if want_dd else 'NULL'})")
                assert bool(torch.isnan(d_x[n:]).all())
            if want_dd:
                _close(dd[:n, :w], dd_ref, what + f" dd_row (d_x {'too' if want_dx else 'NULL'}, width {width})")
                assert torch.equal(dd[:n, :3], gg)
                assert bool((dd[:n, w:width] == 0).all()), what + ": columns [3 + 2L, width) must be exactly 0"
                assert bool(torch.isnan(dd[:n, width:]).all()) and bool(torch.isnan(dd[n:]).all()), what

        second(True, True, w, w)
        second(True, False, w, w)
        second(False, True, w + 5, w + 5 + 3)


def test_fourier_input_gradient_refusals():
    _lib, _ = _api()
    lib = _lib.lib()
    n, L = 5, 4
    w = 3 + 2 * L
    x, gg, gx = (torch.zeros((n, 3), device="cuda") for _ in range(3))
    B = torch.zeros((3, 32), device="cuda")
    d_row, dd = torch.zeros((n, 80), device="cuda"), torch.zeros((n, 80), device="cuda")
    st = _lib.stream_ptr(x)
    p = _lib.dptr
    for bad_L in (0, 33):
        with pytest.raises(_lib.HashmodError):
            _lib.check(lib.hm_fourier_bwd_input(p(x), n, p(B), bad_L, p(d_row), 80, p(gx), st))
        with pytest.raises(_lib.HashmodError):
            _lib.check(lib.hm_fourier_bwd_input_bwd(p(x), n, p(B), bad_L, p(d_row), 80, p(gg), p(gx), p(dd), 80, 80, st))
    with pytest.raises(_lib.HashmodError):          # d_row_stride < 3 + 2L
        _lib.check(lib.hm_fourier_bwd_input(p(x), n, p(B), L, p(d_row), w - 1, p(gx), st))
    with pytest.raises(_lib.HashmodError):
        _lib.check(lib.hm_fourier_bwd_input_bwd(p(x), n, p(B), L, p(d_row), w - 1, p(gg), p(gx), p(dd), 80, w, st))
    with pytest.raises(_lib.HashmodError):          # width < 3 + 2L
        _lib.check(lib.hm_fourier_bwd_input_bwd(p(x), n, p(B), L, p(d_row), 80, p(gg), p(gx), p(dd), 80, w - 1, st))
    with pytest.raises(_lib.HashmodError):          # dd_row_stride < width
        _lib.check(lib.hm_fourier_bwd_input_bwd(p(x), n, p(B), L, p(d_row), 80, p(gg), p(gx), p(dd), w - 1, w, st))
    # the accepted forms of the same calls
    _lib.check(lib.hm_fourier_bwd_input(p(x), n, p(B), L, p(d_row), w, p(gx), st))
    _lib.check(lib.hm_fourier_bwd_input_bwd(p(x), n, p(B), L, p(d_row), w, p(gg), p(gx), p(dd), w, w, st))
