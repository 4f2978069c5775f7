"""The device tracer on filter-bank networks (hm_trace_forward_nffb: every SDF evaluation is hm_nffb_fwd into the
workspace's embedding region followed by hm_sdf_fwd_emb on those rows) over the tracer's configuration space
(tests/trace_cases.py), against the generic torch-op tracer.

hm_nffb_fwd picks its kernel by the live count of a launch: up to 8192 points the lanes-per-point kernel, above it the
matrix-core kernel, and the two agree to ~4e-7, not to the bit (tests/test_nffb_cases_gpu.py).  The two tracers group
the sampler's and the closest-approach points into launches differently, so:

  all-VALU regime   layouts of trace_cases.NFFB_LAYOUTS: rays * max(n_steps, 2) <= 8192, no launch of either tracer can
                    leave the lanes-per-point kernel, and with a fixed SDF tile a point's value does not depend on its
                    launch: mask, distances, points and evaluation counts are compared bit for bit (parts A, B, C)
  MFMA regime       3 x 300 rays: bit for bit between runs that form identical launches (repeat, stale workspace), and
                    the criterion for results of different kernels against the generic tracer (part D)

The generic tracer is tied to the oracle over the same settings in test_raytrace_configs_cpu.py, the embedder kernels
to float64 in test_nffb_cases_gpu.py and hm_sdf_fwd_emb in test_sdf_shapes_gpu.py.

Networks (`nets`), the scale of their SDF output row (OUT_SCALE; chosen with the generic tracer so that every stage of
the search has rays on 3 x 21 rays, see test_networks_reach_every_stage) and what that test observed at the bench
setting in training mode, 64-point tiles (generic evaluations with 0 / 1 / 3 line-search iterations; of 63 rays:
sampler rays, network hits; on the device: secant rays, mask-loss rays):

  ffb          FFB L = 6, 8 x 128, fixture nffb_sdf_ffb                 scale 2.0  6898 / 6907 / 7025   20, 13   6, 42
  stylemod     StyleModNFFB L = 6, 8 x 128, fixture nffb_sdf_stylemod   scale 1.0  7199 / 7202 / 7313   29, 16  11, 34
  stylemod_L8  StyleModNFFB L = 8 (embedding width 75), 8 x 128, seeded scale 1.0  7229 / 7237 / 7256   28, 18   9, 33
  c5           StyleModNFFB L = 6, 8 x 512: the C5 shape (part C)       scale 1.0  7115 / 7116 / 7121   27, 16   8, 34

(ffb unscaled and scaled by 1.5 never steps through its surface: 7366 and 7218 evaluations whatever the number of
line-search iterations.)

Part D, observed on an MI355X against the generic tracer on 900 rays, all twelve settings x modes of both networks: no
mask flip and no ray beyond 1e-4 (1 + |d|) anywhere.  Training mode: the two tracers agree to the bit in 9 of 12
searches (both run their coarse scans on the matrix-core embedder kernel), largest |d dist| 9.5e-7 (ffb, n18).
Evaluation mode (the device's 17-sample first pass stays on the lanes-per-point kernel, the generic tracer's single
pass does not): largest |d dist| 1.0e-5 (ffb, default), 4.8e-7 otherwise; n18 stays below 8192 points in every launch of
both tracers on both networks (4338 / 7848) and is bit-identical.  With the single-pass sampler (sampler_head = 0) the
evaluation-mode device search forms the generic tracer's launches exactly and is asserted bit for bit.  Sampler launches of the device at the bench
setting, first + second pass: ffb 67 897 + 14 857 points (training), 4 097 + 14 857 (evaluation).
"""
import contextlib
import ctypes as C
import functools

import pytest
import torch

import trace_cases as TC
from helpers import make_idr_nffb, make_implicit_nffb

pytestmark = pytest.mark.gpu

MODES = ("train", "eval")
TILES = (16, 64)
KINDS = ("ffb", "stylemod", "stylemod_L8", "c5")
L8_CASES = ("bench", "ls0", "st0", "st15", "n2", "n18", "n130", "sec0", "sec64")
OUT_SCALE = {"ffb": 2.0, "stylemod": 1.0, "stylemod_L8": 1.0, "c5": 1.0}
SEED_L8, SEED_C5 = 31, 11
STAT_KEYS = ("sampler_rays", "secant_rays", "mask_loss_rays", "sdf_evals", "sampler_points", "sampler_second_pass_rays")


def build_net(kind, golden, scale=None):
    """one of the four networks, its SDF output row (row 0 of the last layer) scaled by OUT_SCALE[kind]"""
    from hashmodnffbanks_idr_amd.model.implicit_differentiable_renderer import ImplicitNetwork
    if kind in ("ffb", "stylemod"):
        g = golden(f"nffb_sdf_{kind}")
        net = ImplicitNetwork(16, 3, 1, [128] * 8, True, 0.6, [4], True, multires=6,
                              embed_type={"ffb": "FFB", "stylemod": "StyleModNFFB"}[kind], log2_max_hash_size=5,
                              max_points_per_entry=2, base_resolution=16, desired_resolution=512, bound=1.0)
        net.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd:")})
        net = net.cuda()
    elif kind == "stylemod_L8":
        net = make_implicit_nffb("StyleModNFFB", 8, (128,) * 8, 16, SEED_L8)
        assert net.dims[0] == 75
    else:
        net = make_idr_nffb("StyleModNFFB", SEED_C5).implicit_network
    scale = OUT_SCALE[kind] if scale is None else scale
    last = getattr(net, "lin" + str(net.num_layers - 2))
    with torch.no_grad():       # before the first use: nothing has been packed yet
        last.weight_g[0] *= scale
        last.bias[0] *= scale
    net.eval()
    assert net._fusable() and net._hash_embedder() is None and net._nffb_embedder() is not None
    return net


_nets, _generic, _exact = {}, {}, {}


@pytest.fixture(scope="module")
def nets(golden):
    def get(kind):
        if kind not in _nets:
            _nets[kind] = build_net(kind, golden)
        return _nets[kind]
    yield get
    _nets.clear()
    _generic.clear()
    _exact.clear()


@functools.lru_cache(maxsize=None)
def _rays(layout):
    """the all-VALU layouts, and 3 x 300 rays for the MFMA regime"""
    return TC.make_rays(3, 300, 700) if layout == "3x300" else TC.nffb_rays(layout)


def _inputs(rays):
    cam, dirs, om = rays
    return cam.cuda(), dirs.cuda(), om.reshape(-1).cuda()


def _tracer(case, mode, device=True, head=None):
    from hashmodnffbanks_idr_amd.model.ray_tracing import RayTracing
    rt = RayTracing(*TC.tracer_args(case)).cuda()
    rt.train(mode == "train")
    rt.use_device_tracer = device
    if head is not None:
        rt.sampler_head = head
    return rt


def _trace(net, case, mode, rays, tile, device=True, head=None, count=False, rt=None):
    """one search; returns ((points, mask, dists), stats).  count: the SDF is wrapped to note the size of every call,
    which also sends the search to the generic tracer (stats: 'evals', 'calls' and the generic tracer's own
    sampler_rays).  rt: a tracer object to search with (its workspace has served its earlier searches)."""
    assert device != count
    net.sdf_tile_points = tile
    if rt is None:
        rt = _tracer(case, mode, device, head)
    else:       # the constructor's seven settings, in its argument order
        (rt.object_bounding_sphere, rt.sdf_threshold, rt.line_search_step, rt.line_step_iters, rt.sphere_tracing_iters,
         rt.n_steps, rt.n_secant_steps) = TC.tracer_args(case)
    rt.steps_override = TC.steps(case.n_steps)
    calls = []

    def counted(p):
        calls.append(int(p.shape[0]))
        return net.sdf(p)

    cam, dirs, om = _inputs(rays)
    with torch.no_grad():
        out = rt(sdf=counted if count else net.sdf, cam_loc=cam, object_mask=om, ray_directions=dirs)
    st = dict(rt.last_stats)
    if count:
        st["evals"], st["calls"] = sum(calls), calls
    else:
        assert "sdf_evals" in st, "the search did not run on the device tracer"
    return out, st


def generic(kind, net, name, mode, layout, tile):
    """the generic tracer's result, evaluation count and call sizes, computed once per (network, configuration, mode,
    layout, tile); in the all-VALU regime none of its calls may leave the embedder's lanes-per-point kernel"""
    key = (kind, name, mode, layout, tile)
    if key not in _generic:
        _generic[key] = _trace(net, TC.CONFIGS[name], mode, _rays(layout), tile, device=False, count=True)
    if layout in TC.NFFB_LAYOUTS:
        assert max(_generic[key][1]["calls"], default=0) <= TC.NFFB_SMALL_LAUNCH, (key, max(_generic[key][1]["calls"]))
    return _generic[key]


def _assert_equal(out, ref):
    (p1, m1, d1), (p2, m2, d2) = out, ref
    assert p1.shape == p2.shape and m1.shape == m2.shape and d1.shape == d2.shape
    assert torch.equal(m1, m2), f"{int((m1 != m2).sum())} mask mismatches"
    assert torch.equal(d1, d2), (d1 - d2).abs().max()
    assert torch.equal(p1, p2), (p1 - p2).abs().max()


def _assert_clean(st):
    assert st["unfinished"] == 0 and st["nonfinite"] == 0, st


# ---- every other test relies on this one -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_networks_reach_every_stage(nets, kind):
    """seen from the generic tracer on 3 x 21 rays in training mode: 0, 1 and 3 line-search iterations are different
    searches on this network, some rays reach the sampler, some but not all hit the surface; and on the device the
    secant refinement and the closest-approach (mask-loss) scan have rays"""
    net = nets(kind)
    ev = [generic(kind, net, n, "train", "3x21", 64)[1]["evals"] for n in ("ls0", "default", "bench")]
    (_, m, _), st = generic(kind, net, "bench", "train", "3x21", 64)
    _, dst = _trace(net, TC.CONFIGS["bench"], "train", _rays("3x21"), 64)
    print(f"{kind} (output row x {OUT_SCALE[kind]}): generic evaluations with 0 / 1 / 3 line-search iterations {ev}; of "
          f"{m.numel()} rays: sampler {st['sampler_rays']}, hits {int(m.sum())}; device: secant {dst['secant_rays']}, "
          f"mask loss {dst['mask_loss_rays']}")
    _assert_clean(dst)
    assert st["sampler_rays"] > 0
    assert 0 < int(m.sum()) < m.numel()
    assert dst["mask_loss_rays"] > 0 and dst["secant_rays"] > 0
    assert len(set(ev)) == 3, ev


# ---- A. all settings, bit for bit (all-VALU regime) --------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("layout", list(TC.NFFB_LAYOUTS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(TC.CONFIGS))
@pytest.mark.parametrize("kind", ["ffb", "stylemod"])
def test_device_tracer_equals_generic_tracer(nets, kind, name, mode, layout, tile):
    net = nets(kind)
    ref, _ = generic(kind, net, name, mode, layout, tile)
    out, st = _trace(net, TC.CONFIGS[name], mode, _rays(layout), tile)
    _assert_clean(st)
    _assert_equal(out, ref)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", L8_CASES)
def test_device_tracer_equals_generic_tracer_eight_levels(nets, name, mode):
    """L = 8: 75 floats per point in the workspace's embedding region, the embedder's eight-level instantiation"""
    net = nets("stylemod_L8")
    ref, _ = generic("stylemod_L8", net, name, mode, "3x21", 64)
    out, st = _trace(net, TC.CONFIGS[name], mode, _rays("3x21"), 64)
    _assert_clean(st)
    _assert_equal(out, ref)


@pytest.mark.parametrize("attr,value", [("sphere_tracing_iters", 16), ("line_step_iters", 4), ("n_steps", 1),
                                         ("n_steps", 4097), ("n_secant_steps", 65)])
def test_out_of_range_configuration_is_rejected(nets, attr, value):
    from hashmodnffbanks_idr_amd._lib import HashmodError
    net = nets("ffb")
    case = TC.CONFIGS["bench"]
    cam, dirs, om = _inputs(_rays("3x21"))
    net.sdf_tile_points = 16
    rt = _tracer(case, "train")
    rt.steps_override = TC.steps(case.n_steps)
    setattr(rt, attr, value)
    with torch.no_grad():
        with pytest.raises(HashmodError, match="hm_trace_forward"):
            rt(sdf=net.sdf, cam_loc=cam, object_mask=om, ray_directions=dirs)
        setattr(rt, attr, getattr(case, attr))
        out = rt(sdf=net.sdf, cam_loc=cam, object_mask=om, ray_directions=dirs)
    _assert_clean(rt.last_stats)
    _assert_equal(out, generic("ffb", net, "bench", "train", "3x21", 16)[0])


# ---- B. evaluation counts and the lazy sampler (all-VALU regime) -------------------------------------------------------
def _count_case(nets, kind, name, mode, tile):
    net = nets(kind)
    ref, ref_st = generic(kind, net, name, mode, "3x21", tile)
    out, st = _trace(net, TC.CONFIGS[name], mode, _rays("3x21"), tile, head=0)
    _assert_clean(st)
    _assert_equal(out, ref)
    assert st["sampler_rays"] == ref_st["sampler_rays"]
    assert st["sampler_points"] == TC.CONFIGS[name].n_steps * st["sampler_rays"]
    assert st["sdf_evals"] == ref_st["evals"], (st, ref_st)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(TC.CONFIGS))
def test_device_evaluation_count_equals_generic(nets, name, mode, tile):
    """single-pass sampler (sampler_head = 0): the device evaluates exactly the points the generic tracer does - every
    march round and secant iteration a launch pair with its own counter (61 rounds at st15), count_evals_kernel"""
    _count_case(nets, "ffb", name, mode, tile)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(TC.CONFIGS))
def test_device_evaluation_count_equals_generic_eight_levels(nets, name, mode):
    _count_case(nets, "stylemod_L8", name, mode, 64)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["n17", "n18", "n64", "n99", "n130"])
@pytest.mark.parametrize("kind", ["ffb", "stylemod_L8"])
def test_lazy_sampler_equals_single_pass(nets, kind, name, mode):
    """test_raytrace_configs_gpu.py::test_lazy_sampler_equals_single_pass on this route, where both passes, the appended
    closest-approach rows and the secant share one embedding region: every head gives the outputs of head 0 bit for
    bit, and the sampler evaluates (head + 1) points of every sampler ray plus the n_steps - 1 - head others of the
    second-pass rays while 1 <= head <= n_steps - 2, all n_steps otherwise."""
    net = nets(kind)
    case = TC.CONFIGS[name]
    n = case.n_steps
    res = {}
    for head in sorted({0, 1, 16, n - 2, n - 1}):
        res[head] = _trace(net, case, mode, _rays("3x21"), 64, head=head)
        _assert_clean(res[head][1])
    out0, st0 = res[0]
    _assert_equal(out0, generic(kind, net, name, mode, "3x21", 64)[0])
    assert st0["sampler_rays"] > 0
    assert st0["sampler_points"] == n * st0["sampler_rays"] and st0["sampler_second_pass_rays"] == 0
    for head, (out, st) in res.items():
        _assert_equal(out, out0)
        assert st["sampler_rays"] == st0["sampler_rays"] and st["secant_rays"] == st0["secant_rays"], head
        if 1 <= head <= n - 2:
            assert st["sampler_points"] == (head + 1) * st["sampler_rays"] + \
                (n - 1 - head) * st["sampler_second_pass_rays"], (head, st)
            assert st["sampler_second_pass_rays"] <= st["sampler_rays"]
            assert st["sdf_evals"] <= st0["sdf_evals"], head
            assert st["sdf_evals"] - st0["sdf_evals"] == st["sampler_points"] - st0["sampler_points"], head
        else:        # out of the lazy range: single pass
            assert st["sdf_evals"] == st0["sdf_evals"], head
            assert st["sampler_points"] == st0["sampler_points"] and st["sampler_second_pass_rays"] == 0, head
    print(f"lazy sampler {kind}/{name}/{mode}: sampler rays {st0['sampler_rays']}, sampler points "
          + ", ".join(f"head {h}: {r[1]['sampler_points']}" for h, r in res.items()))


# ---- C. 16-bit coarse modes and the guard on this route ----------------------------------------------------------------
COARSE = {"bf16": ("bf16_coarse_search", True, 1), "bf16x2": ("coarse_split", "bf16x2", 2),
          "f16x2": ("coarse_split", "f16x2", 2)}


@contextlib.contextmanager
def _coarse(net, which):
    """the network with one 16-bit mode of the coarse scans chosen; the mode must be accepted, not quietly dropped"""
    attr, value, code = COARSE[which]
    assert not net.bf16_coarse_search and net.coarse_split is None
    setattr(net, attr, value)
    try:
        assert net.coarse_mode() == code, (which, net.coarse_mode())
        yield net
    finally:
        net.bf16_coarse_search, net.coarse_split = False, None


def _exact_c5(net, name, mode):
    """the exact-fp32 search of the C5-shaped network with the tile size left to the library, once per (setting, mode)"""
    if (name, mode) not in _exact:
        assert net.coarse_mode() == 0
        _exact[name, mode] = _trace(net, TC.CONFIGS[name], mode, _rays("3x21"), 0)
        _assert_clean(_exact[name, mode][1])
    return _exact[name, mode]


@pytest.mark.parametrize("which", list(COARSE))
def test_coarse_modes_are_accepted(nets, which):
    net = nets("c5")
    assert net.coarse_mode() == 0
    with _coarse(net, which):
        assert net.coarse_mode() == COARSE[which][2]
    assert net.coarse_mode() == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["bench", "n18", "n130", "sec0"])
@pytest.mark.parametrize("which", list(COARSE))
def test_coarse_modes_leave_small_launches_exact(nets, which, name, mode):
    """no coarse launch of 3 x 21 rays has more than 8192 live points, and the 16-bit kernels leave such launches to the
    small-tile launch hm_sdf_fwd_emb(tile -1) that precedes them (run_min = kSdfSmall + 1): with the tile size left to
    the library every 16-bit mode is the exact mode bit for bit, statistics included"""
    net = nets("c5")
    ref, ref_st = _exact_c5(net, name, mode)
    assert ref_st["sampler_points"] > 0 and (mode == "eval" or ref_st["mask_loss_rays"] > 0)
    with _coarse(net, which):
        out, st = _trace(net, TC.CONFIGS[name], mode, _rays("3x21"), 0)
    _assert_clean(st)
    _assert_equal(out, ref)
    assert {k: st[k] for k in STAT_KEYS} == {k: ref_st[k] for k in STAT_KEYS}


@pytest.mark.parametrize("kind", ["ffb", "c5"])
def test_guard_is_not_chosen_on_filter_bank_networks(nets, kind):
    net = nets(kind)
    assert net.guarded_coarse_scans and not net.bf16_coarse_search and net.coarse_split is None
    assert net.coarse_mode() != 3
    assert net.coarse_mode() == 0 and net._split_kind() is None


def _direct_call(net, case, mode, rays, tile, coarse, ws_fill):
    """hm_trace_forward_nffb itself, on outputs, statistics and a workspace pre-filled with sentinels.
    Returns (return code, (points, mask, dists), statistics, workspace)."""
    from hashmodnffbanks_idr_amd import _lib, ops
    from hashmodnffbanks_idr_amd._lib import dptr
    from hashmodnffbanks_idr_amd.utils import rend_util
    cam, dirs, om = _inputs(rays)
    B, per, _ = dirs.shape
    N = B * per
    t_sphere, hit = rend_util.get_sphere_intersection(cam, dirs, r=case.radius)
    cfg = _lib.TraceCfg(float(case.radius), float(case.threshold), float(case.line_search_step), int(case.line_step_iters),
                        int(case.sphere_tracing_iters), int(case.n_steps), int(case.n_secant_steps),
                        1 if mode == "train" else 0, int(coarse), 16)
    nf = net._nffb_embedder()
    grid = nf.grid_enc
    ws = torch.full((ops.trace_workspace_bytes(N, cfg, nf.n_levels),), ws_fill, dtype=torch.uint8, device="cuda")
    pts = torch.full((N, 3), -77.0, device="cuda")
    mask = torch.full((N,), 0x5A, dtype=torch.uint8, device="cuda")
    dists = torch.full((N,), -77.0, device="cuda")
    stats = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    keep = [cam.contiguous().float(), dirs.reshape(N, 3).contiguous().float(), om.to(torch.uint8).contiguous(),
            t_sphere.reshape(N, 2).contiguous(), hit.reshape(N).to(torch.uint8).contiguous(),
            torch.linspace(0, 1, steps=case.n_steps).cuda(), TC.steps(case.n_steps).cuda(), grid.table.detach()]
    pk, packed = ops.nffb_packed(nf), net.packed_weights()
    rc = _lib.lib().hm_trace_forward_nffb(
        grid.desc.handle, C.byref(pk.desc), C.byref(packed.desc), dptr(keep[7]), dptr(grid.freq_encoding.B),
        ops.FRAC_MODES[grid.frac_mode], int(tile), C.byref(cfg), dptr(keep[0]), dptr(keep[1]), dptr(keep[2]), dptr(keep[3]),
        dptr(keep[4]), N, per, dptr(keep[5]), dptr(keep[6]), dptr(pts), dptr(mask), dptr(dists), dptr(ws), ws.numel(),
        dptr(stats), _lib.stream_ptr(pts))
    torch.cuda.synchronize()
    return rc, (pts, mask, dists), stats, ws


def test_direct_call_with_the_guarded_mode_is_refused(nets):
    """coarse_bf16 = 3 on hm_trace_forward_nffb: the invalid-argument error before anything is enqueued - outputs,
    statistics and workspace keep their sentinels.  The same call with coarse_bf16 = 0 is the tracer module's search
    (so the refusal is that of the mode, not of the test's own arguments)."""
    from hashmodnffbanks_idr_amd import _lib
    net = nets("c5")
    case = TC.CONFIGS["bench"]
    rc, (pts, mask, dists), stats, _ = _direct_call(net, case, "train", _rays("3x21"), 0, 0, 0)
    assert rc == 0
    _assert_equal((pts, mask.bool(), dists), _exact_c5(net, "bench", "train")[0])
    assert int(stats[6]) == _exact_c5(net, "bench", "train")[1]["sdf_evals"]
    rc, (pts, mask, dists), stats, ws = _direct_call(net, case, "train", _rays("3x21"), 0, 3, 0xA5)
    assert rc == -1, rc      # HM_ERR_INVALID
    assert b"guarded coarse scans do not cover filter-bank" in _lib.lib().hm_last_error()
    assert bool((pts == -77.0).all()) and bool((dists == -77.0).all()) and bool((mask == 0x5A).all())
    assert bool((stats == -7).all())
    assert bool((ws == 0xA5).all())


# ---- D. MFMA regime: 3 x 300 rays --------------------------------------------------------------------------------------
D_CASES = ("bench", "default", "n18", "n130", "sec0", "st15")
D_KINDS = ("ffb", "stylemod_L8")


# Evaluation mode has no closest-approach rows, and the lazy sampler's first pass is 17 samples of at most 900 rays: it
# exceeds 8192 points only with more than 481 sampler rays, which neither network has (241 / 436).  There the launch
# that leaves the lanes-per-point kernel is the second pass (the other n_steps - 17 samples of the unresolved rays), for
# these settings on both networks by a wide margin (ffb: 83 x 179 points at the bench setting).  n18 (a second pass of
# one sample per ray) and st15 (few sampler rays) can stay below 8192 in every launch of BOTH tracers; such a search is
# compared bit for bit, as in the all-VALU regime.
EVAL_MFMA_CASES = ("bench", "default", "n130", "sec0")


def _sampler_launch_points(st, case, mode, head=16):
    """(first, second): points of the sampler's two launches from the statistics.  First pass: head + 1 samples per
    sampler ray inside the lazy range (all n_steps otherwise) and, in training mode, the n_steps samples of every
    closest-approach row behind them; second pass: the other samples of the rays the head did not resolve."""
    n = case.n_steps
    lazy = 1 <= head <= n - 2
    first = (head + 1 if lazy else n) * st["sampler_rays"] + (n * st["mask_loss_rays"] if mode == "train" else 0)
    return first, (n - 1 - head) * st["sampler_second_pass_rays"] if lazy else 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", D_CASES)
@pytest.mark.parametrize("kind", D_KINDS)
def test_mfma_regime_repeat_and_stale_workspace(nets, kind, name, mode):
    """identical launches, identical bits: the same search twice on one tracer object, and on a tracer object whose
    workspace has just served a larger search that touches every region (n130), against a fresh tracer object"""
    net = nets(kind)
    case, rays = TC.CONFIGS[name], _rays("3x300")
    rt = _tracer(case, mode)
    out1, st1 = _trace(net, case, mode, rays, 64, rt=rt)
    _assert_clean(st1)
    first, second = _sampler_launch_points(st1, case, mode)
    print(f"MFMA regime {kind}/{name}/{mode}: sampler launches of {first} and {second} points, {st1}")
    if mode == "train":
        assert first > TC.NFFB_SMALL_LAUNCH, "the matrix-core embedder kernel never ran"
    elif name in EVAL_MFMA_CASES:
        assert max(first, second) > TC.NFFB_SMALL_LAUNCH, "the matrix-core embedder kernel never ran"
    out2, st2 = _trace(net, case, mode, rays, 64, rt=rt)
    _assert_equal(out2, out1)
    assert st2 == st1
    used = _tracer(TC.CONFIGS["n130"], mode)
    _, st_big = _trace(net, TC.CONFIGS["n130"], mode, rays, 64, rt=used)
    _assert_clean(st_big)
    assert st_big["sampler_points"] > 0 and st_big["secant_rays"] > 0
    out3, st3 = _trace(net, case, mode, rays, 64, rt=used)
    _assert_equal(out3, out1)
    assert st3 == st1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", D_CASES)
@pytest.mark.parametrize("kind", D_KINDS)
def test_mfma_regime_against_generic_tracer(nets, kind, name, mode):
    """the two tracers' launches fall on different sides of the embedder's kernel switch, so the criterion for results
    of different kernels (test_raytrace_configs_gpu.py::test_just_above_the_one_launch_ray_count): at most
    max(1, N // 200) mask flips, at most 1 % of the rays beyond 1e-4 (1 + |d|).  The march is the same launches of at
    most 1800 points in both, so the sampler receives the same rays.  An evaluation-mode search in which no launch of
    either tracer exceeds 8192 points (see EVAL_MFMA_CASES) is compared bit for bit instead."""
    net = nets(kind)
    case, rays = TC.CONFIGS[name], _rays("3x300")
    (p1, m1, d1), st = _trace(net, case, mode, rays, 64)
    (p2, m2, d2), ref_st = generic(kind, net, name, mode, "3x300", 64)
    _assert_clean(st)
    if mode == "eval":
        # single-pass sampler without closest-approach rows: the device forms exactly the generic tracer's launches (the
        # march, n_steps x sampler rays in one launch, the secant iterations), so both pick the same embedder kernel for
        # every one of them - the matrix-core kernel for the sampler - and agree to the bit
        out0, st0 = _trace(net, case, mode, rays, 64, head=0)
        _assert_clean(st0)
        assert name == "n18" or case.n_steps * st0["sampler_rays"] > TC.NFFB_SMALL_LAUNCH
        _assert_equal(out0, (p2, m2, d2))
        assert st0["sdf_evals"] == ref_st["evals"] and st0["sampler_rays"] == ref_st["sampler_rays"]
    largest = max(max(ref_st["calls"]), *_sampler_launch_points(st, case, mode))
    if largest <= TC.NFFB_SMALL_LAUNCH:
        assert mode == "eval" and name not in EVAL_MFMA_CASES
        print(f"MFMA regime {kind}/{name}/{mode}: largest launch of both tracers {largest} points: bit for bit")
        _assert_equal((p1, m1, d1), (p2, m2, d2))
        return
    flips = int((m1 != m2).sum())
    both = m1 & m2
    dd = (d1 - d2).abs()
    close = dd <= 1e-4 * (1.0 + d2.abs())
    frac_far = 1.0 - float(close.float().mean())
    print(f"MFMA regime {kind}/{name}/{mode}: {flips} mask flips of {m1.numel()}, max |d dist| on common hits "
          f"{float(dd[both].max()):.3e}, over all rays {float(dd.max()):.3e}, rays beyond 1e-4: {frac_far:.5f}, evaluations "
          f"device {st['sdf_evals']} (lazy sampler) generic {ref_st['evals']}, largest generic call {max(ref_st['calls'])}")
    assert st["sampler_rays"] == ref_st["sampler_rays"] > 0
    assert flips <= max(1, m1.numel() // 200)
    assert frac_far <= 0.01
