"""The filter-bank embedder case table (tests/nffb_cases.py) is what it claims to be - numpy and the C oracle alone, no
GPU: the recorded error budget is re-measured, the float64 reference agrees with the reference implementation's
fixtures, the bound separates the reference from six wrong versions of itself, unconsumed table levels are dead, and
the host-side argument checks of hm_nffb_fwd / ops.nffb_fwd reject what the kernels would write out of bounds."""
import ctypes as C

import numpy as np
import pytest
import torch

import nffb_cases as NC

IDS = [NC.case_id(c) for c in NC.ALL]
SENTINEL = -777.25


@pytest.mark.parametrize("c", NC.ALL, ids=IDS)
def test_recorded_budget_covers_the_case(c):
    """A and B re-measured on the case: neither exceeds its recorded constant (the upper side is the next test)"""
    a, b, scale = NC.measure(c)
    k = (c.L, c.style)
    print(f"{NC.case_id(c)}: A {a:.3e} (recorded {NC.ERR_A[k]:.3e})  B {b:.3e} (recorded {NC.ERR_B[k]:.3e})  "
          f"output scale {scale:.3f}  bound {NC.bound_of(c):.3e}")
    assert 0.5 < scale < 2.0                      # the absolute bound is stated at output scale ~1
    assert 0 < a <= NC.ERR_A[k] and 0 < b <= NC.ERR_B[k]


@pytest.mark.parametrize("L,style", sorted(NC.ERR_A))
def test_recorded_budget_is_not_loose(L, style):
    """every recorded constant lies within [1, 1.5] x the fresh measurement - the largest over the cases that share
    it - so the bound can neither miss a case nor drift loose"""
    ms = [NC.measure(c) for c in NC.ALL if (c.L, c.style) == (L, style)]
    assert len(ms) == 8
    a, b = max(m[0] for m in ms), max(m[1] for m in ms)
    print(f"L = {L}, style = {style}: A {a:.3e} B {b:.3e}; recorded {NC.ERR_A[L, style]:.3e} {NC.ERR_B[L, style]:.3e}")
    assert a <= NC.ERR_A[L, style] <= NC.RECORD_SLACK * a
    assert b <= NC.ERR_B[L, style] <= NC.RECORD_SLACK * b
    assert NC.MARGIN == 3.0 and NC.RECORD_SLACK == 1.5 and NC.PERTURB_ULPS == 2


def test_case_table_covers_what_it_is_for():
    assert len(set(NC.ALL)) == 32
    for c in NC.ALL + NC.SIZE_CASES + NC.STRIDE_CASES:
        g = NC.grid(c)
        live = list(NC.consumed_levels(c))
        assert live == list(range(c.L - 4)) and len(live) >= 2
        dense = [l for l in live if int(g.rows[l]) == int(g.res[l]) ** 3]
        hashed = [l for l in live if int(g.rows[l]) < int(g.res[l]) ** 3]
        assert dense == [0] and hashed == live[1:]
        pow2 = int(g.rows[0]) & (int(g.rows[0]) - 1) == 0
        assert pow2 == (c.grid == "T14") and (c.grid == "T14" or int(g.rows[0]) == 1728)
        assert c in NC.ALL
    for L in (6, 8):
        assert {c.style for c in NC.SIZE_CASES if c.L == L} == {False, True}
    assert {(c.L, c.style) for c in NC.STRIDE_CASES} == {(8, True), (6, False)}
    assert NC.N_MFMA > NC.SMALL_MAX >= NC.N_VALU and NC.N_POINTS == 8192 + 65 and NC.N_STRIDE == 131072 + 21
    assert {c.mode for c in NC.SIZE_CASES} == set(NC.MODES) and {c.bound for c in NC.SIZE_CASES} == {1.0, 1.5}


@pytest.mark.parametrize("c", NC.SIZE_CASES, ids=[NC.case_id(c) for c in NC.SIZE_CASES])
def test_points_hold_faces_outside_points_and_zeros(c):
    x = NC.points(c)
    _, u = NC.inputs_fp32(c, x)
    assert x.shape == (NC.N_POINTS, 3) and np.isfinite(x).all()
    assert np.abs(x[:-NC.n_adversarial(c)]).max() <= 1.3 * c.bound + 1e-6
    assert (np.abs(x) == 3.0).any() and (np.abs(x) == 1.0).all(1).any()
    assert (x == 0).all(1).sum() >= 2 and np.signbit(x[(x == 0).all(1)]).any()
    assert (u < 0).any() and (u > 1).any()
    for l in NC.consumed_levels(c):
        xs = u.astype(np.float64) * float(NC.grid(c).res[l])
        assert (xs == np.floor(xs)).all(1).sum() >= 3, l          # points with u on a voxel node of the level
    # both kernels' calls of the configuration test see the adversarial tail
    assert NC.n_adversarial(c) < NC.N_VALU


@pytest.mark.parametrize("tag,style", [("ffb", False), ("stylemod", True)])
@pytest.mark.parametrize("L", [6, 8])
def test_reference_agrees_with_the_fixtures(golden, tag, style, L):
    """ref_fwd(float64) on the parameters and points of nffb_{ffb,stylemod}_L{6,8} against the stored output of the
    reference implementation (torch, fp32): an fp32 evaluation by other sin / cos / GEMM routines, so within the
    kernels' own bound, plus half an fp32 step of the stored value"""
    g = golden(f"nffb_{tag}_L{L}")
    prefix = "sd:embedder_obj."
    p = {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}
    c = NC.Case(L, style, "reference", 1.0, "T14")
    grid = NC.O.Grid(L, 5, 16, 512)                                   # the fixtures' log2_max_hash_size = 5
    ref = NC.ref_fwd(c, g["x"], np.float64, p=p, g=grid)
    out = g["out"].astype(np.float64)
    assert ref.shape == out.shape == (256, NC.width(c))
    assert np.array_equal(ref[:, :3], out[:, :3])
    err = np.abs(ref - out)[:, 3:]
    tol = NC.bound_of(c) + 2.0 ** -24 * np.abs(out[:, 3:])
    print(f"nffb_{tag}_L{L}: max |ref_fwd(float64) - fixture| {err.max():.3e}, bound {NC.bound_of(c):.3e}")
    assert (err <= tol).all()


@pytest.mark.parametrize("mutation", NC.MUTATIONS)
@pytest.mark.parametrize("c", NC.SIZE_CASES, ids=[NC.case_id(c) for c in NC.SIZE_CASES])
def test_bound_tells_the_reference_from_its_mutations(c, mutation):
    """each wrong version of the reference is at least 10 bounds away from it on at least 1 % of the rows"""
    if mutation == "unbiased_variance" and not c.style:
        assert np.array_equal(NC.ref_fwd(c, NC.points(c)[:64], mutation=mutation), NC.reference(c)[:64])
        return                                                    # plain FFB has no normalisation to get wrong
    d = np.abs(NC.ref_fwd(c, NC.points(c), mutation=mutation) - NC.reference(c))
    assert np.array_equal(d[:, :3], np.zeros_like(d[:, :3]))
    far = (d[:, 3:].max(1) >= 10.0 * NC.bound_of(c)).mean()
    print(f"{NC.case_id(c)} {mutation}: max {d.max():.3e}, {100 * far:.1f} % of rows >= 10 x {NC.bound_of(c):.3e}")
    assert far >= 0.01


@pytest.mark.parametrize("c", NC.SIZE_CASES, ids=[NC.case_id(c) for c in NC.SIZE_CASES])
def test_fp64_rounded_two_pi_is_inside_the_budget(c):
    """the other reading of 'two_pi as float64': s = fl32(2 pi_64 u) moves a Fourier argument by at most one fp32 step,
    which B allows by construction (two steps of the sin / cos values) - it stays inside the bound, so no test of
    this kind can (or needs to) tell it from the kernel's fl32(fl32(2 pi) u)"""
    xn, u = NC.inputs_fp32(c, NC.points(c))
    row = NC.grid_row_two_pi(c, u, 2.0 * np.pi)
    d = np.abs(NC.forward(c, NC.params(c), xn, u, row, np.float64) - NC.reference(c)).max()
    print(f"{NC.case_id(c)}: fl32(2 pi_64 u) moves the reference by {d:.3e} (bound {NC.bound_of(c):.3e})")
    assert 0 < d < NC.bound_of(c)


@pytest.mark.parametrize("c", NC.SIZE_CASES, ids=[NC.case_id(c) for c in NC.SIZE_CASES])
def test_unconsumed_levels_are_dead_inputs(c):
    p = NC.rerandomised_dead_levels(c)
    changed = [l for l in range(c.L)
               if not np.array_equal(p[f"grid_enc.levels.{l}.embedding.weight"],
                                     NC.params(c)[f"grid_enc.levels.{l}.embedding.weight"])]
    assert changed == list(range(c.L - 4, c.L))
    x = NC.points(c)[-NC.N_VALU:]
    for dtype in (np.float64, np.float32):
        assert np.array_equal(NC.ref_fwd(c, x, dtype, p=p), NC.ref_fwd(c, x, dtype))
    # and the last consumed level is a live one
    live = dict(NC.params(c))
    k = f"grid_enc.levels.{c.L - 5}.embedding.weight"
    live[k] = live[k][::-1].copy()
    assert not np.array_equal(NC.ref_fwd(c, x, p=live), NC.ref_fwd(c, x))


# ---- argument checks of the library entry: no device needed, every check precedes the launch ----------------------
class _HostCall:
    """hm_nffb_fwd on host buffers with valid arguments; `call(**changes)` alters some of them.  Nothing here may reach
    a launch: every call must come back with the invalid-argument status."""

    def __init__(self, L=6, style=True, F=2):
        from hashmodnffbanks_idr_amd import _lib, ops
        self.lib, self.L, self.W = _lib, L, 8 + 8 * L
        res, rows = ops.level_table(L, 12, 12, 512)
        self.desc = ops.GridDesc(res, rows, F)
        W = self.W
        self.bufs = dict(w=np.zeros((W, W), np.float32), b=np.zeros(W, np.float32), x=np.zeros((4, 3), np.float32),
                         table=np.zeros((self.desc.total_rows, F), np.float32), B=np.zeros((3, L), np.float32))
        self.out = np.full((4, 3 + W + 2), SENTINEL, np.float32)
        nf = _lib.NffbDesc()
        nf.n_levels, nf.bound, nf.w0, nf.style_eps = L, 1.0, float(L * L - L), 1e-5
        for l in range(L - 1):
            nf.trunk_w[l], nf.trunk_b[l] = self._p("w"), self._p("b")
        nf.out_w, nf.out_b = self._p("w"), self._p("b")
        if style:
            nf.style_w, nf.style_b = self._p("w"), self._p("b")
        self.nf = nf

    def _p(self, name):
        return self.bufs[name].ctypes.data

    def call(self, out_stride=None, frac_mode=0):
        rc = self.lib.lib().hm_nffb_fwd(self.desc.handle, C.byref(self.nf), C.c_void_p(self._p("x")), 4,
                                        C.c_void_p(self._p("table")), C.c_void_p(self._p("B")),
                                        C.c_void_p(self.out.ctypes.data),
                                        self.out.shape[1] if out_stride is None else out_stride, frac_mode, None, None)
        msg = self.lib.lib().hm_last_error().decode()
        assert np.all(self.out == np.float32(SENTINEL))
        return rc, msg


def test_library_rejects_bad_arguments_before_any_launch():
    """out_stride = width - 1, bound = 0, style_w without style_b, n_levels unlike the grid's L, a grid with F = 4 and
    a bad frac_mode: each is the invalid-argument status (-1) with its own message, the output untouched"""
    h = _HostCall()
    width = 3 + h.W
    assert h.call(out_stride=width - 1) == (-1, "hm_nffb_fwd: bad n / out_stride")
    h.nf.bound = 0.0
    assert h.call() == (-1, "hm_nffb_fwd: bound must be positive")
    h.nf.bound = -1.0
    assert h.call()[0] == -1
    h = _HostCall()
    h.nf.style_b = None
    assert h.call() == (-1, "hm_nffb_fwd: style weight / bias must come together")
    h = _HostCall()
    h.nf.style_w = None
    assert h.call() == (-1, "hm_nffb_fwd: style weight / bias must come together")
    h = _HostCall()
    h.nf.n_levels = 8
    assert h.call() == (-1, "hm_nffb_fwd: descriptor / grid level count mismatch")
    h = _HostCall(F=4)
    assert h.call() == (-1, "hm_nffb_fwd: the filter-bank embedders use F = 2 features per level")
    h = _HostCall()
    for fm in (2, -1):
        assert h.call(frac_mode=fm) == (-1, "hm_nffb_fwd: bad frac_mode")
    with pytest.raises(ValueError):
        h.lib.check(-1)


# ---- ops.nffb_fwd: out / n_dev are checked before anything needs a device --------------------------------------
@pytest.fixture(scope="module")
def cpu_module():
    from hashmodnffbanks_idr_amd.model.custom_embedder_decoder import Custom_Embedding_Network
    return Custom_Embedding_Network(3, [3, 512], "FFB", 6, 12, 2, 12, 512, 1.0).embedder_obj


def test_nffb_fwd_rejects_out_and_n_dev_it_cannot_address(cpu_module):
    from hashmodnffbanks_idr_amd import _lib, ops
    mod, width, n = cpu_module, 3 + 8 + 8 * 6, 5
    x = torch.zeros((n, 3))

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            ops.nffb_fwd(mod, x, **kw)

    bad("2-D float32", out=torch.zeros((n, width), dtype=torch.float64))
    bad("2-D float32", out=torch.zeros((n, width), dtype=torch.float16))
    bad("2-D float32", out=torch.zeros(n * width))
    bad("2-D float32", out=np.zeros((n, width), np.float32))
    bad("smaller than", out=torch.zeros((n - 1, width)))
    bad("smaller than", out=torch.zeros((n, width - 1)))
    bad("stride", out=torch.zeros((n, 2 * width))[:, ::2])                 # column stride 2
    bad("stride", out=torch.zeros((width, n)).t())                         # column stride n, row stride 1
    bad("stride", out=torch.zeros((1, width)).expand(n, width))            # row stride 0: every row is the same memory
    bad("int32", n_dev=torch.tensor([n], dtype=torch.int64))
    bad("int32", n_dev=torch.tensor([float(n)]))
    bad("int32", n_dev=torch.zeros(0, dtype=torch.int32))
    bad("int32", n_dev=n)
    # what the checks accept goes on to the device requirement (these tensors are on the host): padded rows, spare
    # rows and columns, a 0-d count
    for kw in (dict(out=torch.zeros((n, width))), dict(out=torch.zeros((n + 2, width + 5))[:, :width]),
               dict(out=torch.zeros((n + 2, width + 5))), dict(n_dev=torch.tensor(n, dtype=torch.int32)),
               dict(n_dev=torch.tensor([n], dtype=torch.int32), out=torch.zeros((n, width)))):
        with pytest.raises(_lib.HashmodError, match="only on HIP") as e:
            ops.nffb_fwd(mod, x, **kw)
        assert not isinstance(e.value, ValueError)
