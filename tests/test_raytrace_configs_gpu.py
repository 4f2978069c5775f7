"""The device tracer (csrc/hm_trace.hip, hm_trace_dev.h and the persistent march, secant and scan kernels of
csrc/hm_sdf.hip) against the generic torch-op tracer over the tracer's configuration space (tests/trace_cases.py).

With a fixed SDF tile size a point's value does not depend on the launch that computed it, so the two tracers must
agree bit for bit - in mask, distances, points and in the number of SDF evaluations.  The generic tracer is tied to the
oracle over the same configurations in test_raytrace_configs_cpu.py.  Network: the raytrace_bumpy fixture (C1, 8 x 512)
with its output layer scaled by OUT_SCALE, see `net`."""
import numpy as np
import pytest
import torch

import trace_cases as TC
from helpers import make_implicit

pytestmark = pytest.mark.gpu

MODES = ("train", "eval")
TILES = (16, 64)
# The fixture network under-estimates distances: on the CPU reference network the generic tracer makes the same 35 646
# (1 x 300 rays) / 27 434 (3 x 77) evaluations with 0, 1 and 3 line-search iterations - it never steps through the surface.
# Its SDF output row scaled by 2.5 it does (33 749 / 33 885 / 33 900), and about a quarter of the rays still reach the
# sampler.  test_fixture_network_runs_line_searches asserts it on the device.
OUT_SCALE = 2.5


@pytest.fixture(scope="module")
def net(golden):
    g = golden("raytrace_bumpy")
    net = make_implicit("C1", (512,) * 8, 256, int(g["seed"]), float(g["perturb"]), float(g["table_scale"]),
                        bias=float(g["bias"]) if "bias" in g.files else 0.6)
    with torch.no_grad():       # before the first use: nothing has been packed yet
        net.lin8.weight_g[0] *= OUT_SCALE
        net.lin8.bias[0] *= OUT_SCALE
    net.eval()
    return net


def _inputs(rays):
    cam, dirs, om = rays
    return cam.cuda(), dirs.cuda(), om.reshape(-1).cuda()


def _trace(net, case, mode, rays, tile, device=True, head=None, count=False):
    """one search; returns ((points, mask, dists), stats).  count: the SDF is wrapped to count its points, which also
    sends the search to the generic tracer (stats: 'evals' and the generic tracer's own sampler_rays)."""
    from hashmodnffbanks_idr_amd.model.ray_tracing import RayTracing
    assert device != count
    net.sdf_tile_points = tile
    rt = RayTracing(*TC.tracer_args(case)).cuda()
    rt.train(mode == "train")
    rt.use_device_tracer = device
    if head is not None:
        rt.sampler_head = head
    rt.steps_override = TC.steps(case.n_steps)
    evals = []

    def counted(p):
        evals.append(int(p.shape[0]))
        return net.sdf(p)

    cam, dirs, om = _inputs(rays)
    with torch.no_grad():
        out = rt(sdf=counted if count else net.sdf, cam_loc=cam, object_mask=om, ray_directions=dirs)
    st = dict(rt.last_stats)
    if count:
        st["evals"] = sum(evals)
    else:
        assert "sdf_evals" in st, "the search did not run on the device tracer"
    return out, st


_generic = {}


def generic(net, name, mode, layout, tile):
    """the generic tracer's result and evaluation count, computed once per (configuration, mode, layout, tile)"""
    key = (name, mode, layout, tile)
    if key not in _generic:
        _generic[key] = _trace(net, TC.CONFIGS[name], mode, TC.rays(layout), tile, device=False, count=True)
    return _generic[key]


def _assert_equal(out, ref):
    (p1, m1, d1), (p2, m2, d2) = out, ref
    assert p1.shape == p2.shape and m1.shape == m2.shape and d1.shape == d2.shape
    assert torch.equal(m1, m2), f"{int((m1 != m2).sum())} mask mismatches"
    assert torch.equal(d1, d2), (d1 - d2).abs().max()
    assert torch.equal(p1, p2), (p1 - p2).abs().max()


def _assert_clean(st):
    assert st["unfinished"] == 0 and st["nonfinite"] == 0, st


# ---- bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("layout", list(TC.LAYOUTS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(TC.CONFIGS))
def test_device_tracer_equals_generic_tracer(net, name, mode, layout, tile):
    ref, _ = generic(net, name, mode, layout, tile)
    out, st = _trace(net, TC.CONFIGS[name], mode, TC.rays(layout), tile)
    _assert_clean(st)
    _assert_equal(out, ref)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("layout", list(TC.LAYOUTS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(TC.CONFIGS))
def test_device_evaluation_count_equals_generic(net, name, mode, layout, tile):
    """single-pass sampler (sampler_head = 0): the device evaluates exactly the points the generic tracer does - the
    per-round counters, the persistent tail's own accounting (tile 16) and count_evals_kernel"""
    ref, ref_st = generic(net, name, mode, layout, tile)
    out, st = _trace(net, TC.CONFIGS[name], mode, TC.rays(layout), tile, head=0)
    _assert_clean(st)
    _assert_equal(out, ref)
    assert st["sampler_rays"] == ref_st["sampler_rays"]
    assert st["sampler_points"] == TC.CONFIGS[name].n_steps * st["sampler_rays"]
    assert st["sdf_evals"] == ref_st["evals"], (st, ref_st)


@pytest.mark.parametrize("layout", ["1x300", "3x77"])
@pytest.mark.parametrize("tile", TILES)
def test_fixture_network_runs_line_searches(net, layout, tile):
    """seen from the generic tracer: 0, 1 and 3 line-search iterations are different searches on this network, and
    sampler, secant and closest-approach stages all have rays at the bench setting"""
    ev = [generic(net, n, "train", layout, tile)[1]["evals"] for n in ("ls0", "default", "bench")]
    print(f"generic evaluations with 0 / 1 / 3 line-search iterations, {layout}, tile {tile}: {ev}")
    assert ev[0] != ev[2] and ev[0] != ev[1] and ev[1] != ev[2], ev
    (_, m, _), st = generic(net, "bench", "train", layout, tile)
    assert st["sampler_rays"] > 8 and 0 < int(m.sum()) < m.numel()
    assert generic(net, "st15", "train", layout, tile)[1]["evals"] != ev[2]     # rays march beyond iteration 10


# ---- lazy sampler ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["1x300", "3x77"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["n17", "n18", "n64", "n99", "n130"])
def test_lazy_sampler_equals_single_pass(net, name, mode, layout):
    """test_raytrace_gpu.py::test_lazy_sampler_equals_single_pass with n_steps in place of 100: every head gives the
    outputs of head 0 bit for bit, and the sampler evaluates (head + 1) points of every sampler ray plus the
    n_steps - 1 - head others of the second-pass rays while 1 <= head <= n_steps - 2, all n_steps otherwise."""
    case = TC.CONFIGS[name]
    n = case.n_steps
    res = {}
    for head in sorted({0, 1, 16, n - 2, n - 1}):
        res[head] = _trace(net, case, mode, TC.rays(layout), 64, head=head)
        _assert_clean(res[head][1])
    out0, st0 = res[0]
    _assert_equal(out0, generic(net, name, mode, layout, 64)[0])
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
    print(f"lazy sampler {name}/{mode}/{layout}: sampler rays {st0['sampler_rays']}, sampler points "
          + ", ".join(f"head {h}: {r[1]['sampler_points']}" for h, r in res.items()))


# ---- persistent tail ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["st15", "default"])
def test_persistent_tail_carries_whole_marches(net, name, mode, monkeypatch):
    """HM_TRACE_TAIL_FIRST=1: every ray's whole march - 15 iterations with up to 3 line searches each (60 rounds), or the
    class default's single line search - runs inside trace_march_tail_kernel, eight rays per workgroup: with 77 rays per
    camera workgroups 9, 19 and 28 carry rays of two cameras.  16-point tiles, bit for bit, same evaluation count."""
    ref, ref_st = generic(net, name, mode, "3x77", 16)
    monkeypatch.setenv("HM_TRACE_TAIL_FIRST", "1")
    for head in (None, 0):
        out, st = _trace(net, TC.CONFIGS[name], mode, TC.rays("3x77"), 16, head=head)
        _assert_clean(st)
        _assert_equal(out, ref)
    assert st["sdf_evals"] == ref_st["evals"], (st, ref_st)


# ---- one-launch scan + secant (tile size left to the library) ----------------------------------------------------------
def _overlap_pair(net, case, rays, monkeypatch):
    res = []
    for ov in ("1", "0"):
        monkeypatch.setenv("HM_TRACE_OVERLAP", ov)
        res.append(_trace(net, case, "train", rays, 0))
    return res


@pytest.mark.parametrize("name", ["n7", "n18", "n130", "sec1", "sec64", "ls0"])
def test_scan_and_secant_in_one_launch(net, name, monkeypatch):
    """test_raytrace_gpu.py::test_scan_and_secant_in_one_launch_edge_cases' criteria away from 100 steps / 8 secant
    iterations / 3 line searches: HM_TRACE_OVERLAP=1 (closest-approach scan and secant refinement in one launch) against
    0, 2048 rays, training.  The small-tile bodies (4 / 8 / 16 points) agree to ~1e-7, not to the bit, so: at most one mask
    flip, distances of agreeing rays to 1e-4 relative, and closest-approach results bit-identical where both forms scan
    on the 64-point kernel."""
    case = TC.CONFIGS[name]
    n = case.n_steps
    rays = TC.make_rays(1, 2048, 21)
    ((p1, m1, d1), s1), ((p2, m2, d2), s2) = _overlap_pair(net, case, rays, monkeypatch)
    _assert_clean(s1)
    _assert_clean(s2)
    assert s1["sdf_evals"] == s2["sdf_evals"] and s1["mask_loss_rays"] == s2["mask_loss_rays"] > 0
    assert s1["secant_rays"] > 0 and s1["sampler_rays"] > 0
    flips = int((m1 != m2).sum())
    both = m1 == m2
    rel = ((d1 - d2).abs() / (1.0 + d2.abs()))[both]
    scan64 = s1["mask_loss_rays"] * n > 8192 and (s1["sampler_points"] + s1["mask_loss_rays"] * n) > 8192
    print(f"one-launch {name}: {flips} mask flips of 2048, max relative |d dist| on agreeing rays {float(rel.max()):.3e}, "
          f"bit-equal {float((rel == 0).float().mean()):.4f}, scan on the 64-point kernel in both forms: {scan64}, stats {s1}")
    assert flips <= 1
    assert float(rel.max()) <= 1e-4
    if scan64:
        miss = ~m1 & ~m2
        assert torch.equal(d1[miss], d2[miss]) and torch.equal(p1[miss], p2[miss])


def test_just_above_the_one_launch_ray_count(net):
    """8193 rays x 8 steps: one ray more than the one-launch form takes, so the scan joins the sampler's launch and the
    secant runs launch by launch; against the generic tracer by the tile-0 criterion of test_raytrace_gpu._device_vs_host"""
    case = TC.CONFIGS["bench"]._replace(n_steps=8, branch="n_rays = kSdfSmall + 1")
    rays = TC.make_rays(1, 8193, 23)
    (p1, m1, d1), st = _trace(net, case, "train", rays, 0)
    (p2, m2, d2), ref_st = _trace(net, case, "train", rays, 0, device=False, count=True)
    _assert_clean(st)
    flips = int((m1 != m2).sum())
    both = m1 & m2
    dd = (d1 - d2).abs()
    close = dd <= 1e-4 * (1.0 + d2.abs())
    frac_far = 1.0 - float(close.float().mean())
    print(f"8193 rays, tile 0: {flips} mask flips, max |d dist| on common hits {float(dd[both].max()):.3e}, rays beyond "
          f"1e-4: {frac_far:.5f}, evaluations device {st['sdf_evals']} (lazy sampler) generic {ref_st['evals']}")
    assert st["sampler_rays"] > 0 and st["secant_rays"] > 0 and st["mask_loss_rays"] > 0
    assert flips <= max(1, m1.numel() // 200)
    assert frac_far <= 0.01


# ---- configurations the C entry point rejects ------------------------------------------------------------------------
@pytest.mark.parametrize("attr,value", [("sphere_tracing_iters", 16), ("line_step_iters", 4), ("n_steps", 1),
                                         ("n_steps", 4097), ("n_secant_steps", 65)])
def test_out_of_range_configuration_is_rejected(net, attr, value):
    from hashmodnffbanks_idr_amd._lib import HashmodError
    from hashmodnffbanks_idr_amd.model.ray_tracing import RayTracing
    case = TC.CONFIGS["bench"]
    cam, dirs, om = _inputs(TC.rays("3x77"))
    net.sdf_tile_points = 16
    rt = RayTracing(*TC.tracer_args(case)).cuda()
    rt.train(True)
    rt.steps_override = TC.steps(case.n_steps)
    setattr(rt, attr, value)
    with torch.no_grad():
        with pytest.raises(HashmodError, match="hm_trace_forward"):
            rt(sdf=net.sdf, cam_loc=cam, object_mask=om, ray_directions=dirs)
        setattr(rt, attr, getattr(case, attr))
        out = rt(sdf=net.sdf, cam_loc=cam, object_mask=om, ray_directions=dirs)
    _assert_clean(rt.last_stats)
    fresh, _ = _trace(net, case, "train", TC.rays("3x77"), 16)
    _assert_equal(out, fresh)
