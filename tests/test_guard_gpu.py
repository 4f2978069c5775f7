"""Guarded coarse scans (ImplicitNetwork.guarded_coarse_scans, hm_trace_cfg.coarse_bf16 = 3): the tracer's coarse rows on
the f16x2 split kernel behind an fp32 guard (csrc/hm_trace.hip: guard_select_sampler_kernel) against all-fp32 scans.  The
guard is a floating-point filter - every sample whose approximate value cannot settle what the search reads from a row is
re-evaluated by the exact-fp32 kernel - so the comparison is torch.equal on every output and equality of every counter,
with the tile size left to the library (the default, what bench.py times)."""
import json
import os

import numpy as np
import pytest
import torch

import bench
from helpers import idr_conf, make_implicit

pytestmark = pytest.mark.gpu

TOL = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "guard_tolerances.json")))
TAU, TAU_TRIP = float(TOL["tau"]), float(TOL["tau_trip"])
GUARD_KEYS = ("guard_refined", "guard_max_dev", "guard_tripped")
_NETS = {}


def _fixture(golden, tag):
    """(fixture arrays, its network) - built once per tag"""
    if tag not in _NETS:
        g = golden(f"raytrace_{tag}")
        net = make_implicit("C2" if tag == "C2" else "C1", (512,) * 8, 256, int(g["seed"]), float(g["perturb"]),
                            float(g["table_scale"]), bias=float(g["bias"]) if "bias" in g.files else 0.6)
        net.eval()
        _NETS[tag] = (g, net)
    return _NETS[tag]


def _tracer(g, mode, head):
    from hashmodnffbanks_idr_amd.model.ray_tracing import RayTracing
    rt = RayTracing(1.0, 5.0e-5, 0.5, 3, 10, 100, 8).cuda()
    rt.train(mode == "train")
    rt.sampler_head = head
    rt.steps_override = torch.from_numpy(g["steps"])
    return rt


def _rays(g, n_rays=None, half_mask=False):
    cam, dirs, om = g["cam_loc"], g["ray_dirs"], g["object_mask"].copy()
    if half_mask:
        om.reshape(-1)[::2] = False
    if n_rays is not None:
        dirs, om = dirs[:, :n_rays], om[..., :n_rays]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return T(cam), T(om), T(dirs)


def _call(rt, net, rays, guard):
    net.guarded_coarse_scans = guard
    try:
        assert net.coarse_mode() == (3 if guard else 0)
        with torch.no_grad():
            out = rt(sdf=net.sdf, cam_loc=rays[0], object_mask=rays[1], ray_directions=rays[2])
        return out, dict(rt.last_stats)
    finally:
        net.guarded_coarse_scans = True


def _coarse_points(st):
    return st["sampler_points"] + 100 * st["mask_loss_rays"]


def _launches(st, head):
    """live points of the coarse launches of a 2048-ray-or-fewer call with the tile size left to the library: the
    sampler's first pass, its second pass, the closest-approach rows"""
    if 1 <= head <= 98:
        return st["sampler_rays"] * (head + 1), st["sampler_second_pass_rays"] * (99 - head), 100 * st["mask_loss_rays"]
    return st["sampler_points"], 0, 100 * st["mask_loss_rays"]


def _assert_same(got, ref, what):
    (o1, s1), (o2, s2) = got, ref
    for name, x, y in zip(("points", "mask", "distances"), o1, o2):
        assert torch.equal(x, y), f"{what}: {name} differ in {int((x != y).sum())} entries"
    for k in s2:
        if k not in GUARD_KEYS:
            assert s1[k] == s2[k], f"{what}: counter {k}: {s1[k]} != {s2[k]}"
    assert s1["unfinished"] == 0 and s1["nonfinite"] == 0


def test_tolerance_record_matches_the_library():
    """tests/golden/guard_tolerances.json: tau is the smallest power of two >= 16 D, tau_trip = tau / 4, and both are the
    library's constants"""
    from hashmodnffbanks_idr_amd import ops
    D = max(float(v) for v in TOL["D"].values())
    assert TAU >= 16 * D > TAU / 2 and np.log2(TAU) == round(np.log2(TAU)) and TAU_TRIP == TAU / 4
    assert TAU <= 2.0 ** -14
    assert ops.trace_guard_tolerances() == (np.float32(TAU), np.float32(TAU_TRIP))


@pytest.mark.parametrize("head", [0, 1, 16, 98])
@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("tag", ["init", "bumpy", "C2", "C2_halfmask"])
def test_bit_identity_guard_on_against_off(golden, tag, mode, head):
    g, net = _fixture(golden, tag.split("_")[0])
    rays = _rays(g, half_mask=tag.endswith("halfmask"))
    on = _call(_tracer(g, mode, head), net, rays, True)
    off = _call(_tracer(g, mode, head), net, rays, False)
    st = on[1]
    print(f"{tag} {mode} head {head}: refined {st['guard_refined']} of {_coarse_points(st)} coarse points, max dev "
          f"{st['guard_max_dev']:.3e}, stats {st}")
    _assert_same(on, off, f"{tag} {mode} head {head}")
    assert off[1]["guard_refined"] == 0
    # the guard has work exactly where a coarse launch has more than 8192 live points (smaller launches run on the exact
    # small-tile kernel in both modes, e.g. raytrace_init in eval mode with head 16: 7418 coarse points in all)
    assert (st["guard_refined"] > 0) == (max(_launches(st, head)) > 8192), _launches(st, head)
    assert st["guard_refined"] > 0 or tag in ("init", "bumpy")
    assert not st["guard_tripped"] and st["guard_max_dev"] <= TAU_TRIP


def test_small_count_edge(golden):
    """a prefix of raytrace_C2's rays whose coarse launches all have <= 8192 live points runs them on the exact small-tile
    kernel: nothing to refine; a few rays more and the guard works.  (Training, single-pass sampler: the sampler's rows
    and the closest-approach rows are launches of their own, sampler_points and 100 * mask_loss_rays points.)"""
    g, net = _fixture(golden, "C2")
    small = big = None
    for k in range(96, 400, 4):
        rays = _rays(g, n_rays=k)
        on = _call(_tracer(g, "train", 0), net, rays, True)
        off = _call(_tracer(g, "train", 0), net, rays, False)
        _assert_same(on, off, f"{k} rays")
        st = on[1]
        launch = max(st["sampler_points"], 100 * st["mask_loss_rays"])
        if launch <= 8192:
            small = (k, st)
            assert st["guard_refined"] == 0, (k, st)
        else:
            big = (k, st)
            assert st["guard_refined"] > 0, (k, st)
            break
    assert small is not None and big is not None and big[0] - small[0] == 4, (small, big)
    print(f"small-count edge: {small[0]} rays -> launches of {small[1]['sampler_points']} and "
          f"{100 * small[1]['mask_loss_rays']} points, refined 0; {big[0]} rays -> {big[1]['sampler_points']} and "
          f"{100 * big[1]['mask_loss_rays']}, refined {big[1]['guard_refined']}")


@pytest.mark.parametrize("head", [0, 16])
@pytest.mark.parametrize("tag", ["C2", "bumpy"])
def test_worst_case_errors(golden, tag, head, monkeypatch):
    """HM_TRACE_GUARD_NOISE=0.75: every approximate value off by up to 0.75 tau - the outputs stay those of the all-fp32
    scans, the monitor trips (0.75 tau > tau / 4), the next call refines every coarse point, and clearing the flag brings
    the refined count back.  nan:37: every 37th approximate value NaN / +Inf - patched, the non-finite counter stays."""
    g, net = _fixture(golden, tag)
    rays = _rays(g)
    off = _call(_tracer(g, "train", head), net, rays, False)
    rt = _tracer(g, "train", head)
    clean = _call(rt, net, rays, True)
    _assert_same(clean, off, "clean")
    assert not clean[1]["guard_tripped"]
    monkeypatch.setenv("HM_TRACE_GUARD_NOISE", "0.75")
    noisy = _call(rt, net, rays, True)
    _assert_same(noisy, off, "noise 0.75")
    print(f"{tag} head {head}: clean refined {clean[1]['guard_refined']}, noise 0.75 refined {noisy[1]['guard_refined']} "
          f"max dev {noisy[1]['guard_max_dev']:.3e}")
    assert noisy[1]["guard_tripped"] and TAU_TRIP < noisy[1]["guard_max_dev"] <= TAU
    monkeypatch.delenv("HM_TRACE_GUARD_NOISE")
    after = _call(rt, net, rays, True)
    _assert_same(after, off, "tripped")
    # every point of the launches the split kernel took (launches of <= 8192 points are exact already; the lazy sampler's
    # second pass may re-evaluate first-pass samples of its rows: >=)
    approx = sum(n for n in _launches(after[1], head) if n > 8192)
    assert after[1]["guard_tripped"] and after[1]["guard_refined"] >= approx > 0, (approx, after[1])
    assert after[1]["guard_refined"] <= _coarse_points(after[1]) + 17 * after[1]["sampler_second_pass_rays"]
    rt.clear_guard()
    again = _call(rt, net, rays, True)
    _assert_same(again, off, "cleared")
    assert not again[1]["guard_tripped"] and again[1]["guard_refined"] == clean[1]["guard_refined"]
    monkeypatch.setenv("HM_TRACE_GUARD_NOISE", "nan:37")
    nan = _call(rt, net, rays, True)
    _assert_same(nan, off, "nan:37")
    assert nan[1]["nonfinite"] == off[1]["nonfinite"] and nan[1]["guard_refined"] > clean[1]["guard_refined"]
    assert not nan[1]["guard_tripped"]


def test_refined_share(golden):
    """a condition, not a measurement: at most 10 % of the coarse points are re-evaluated, on raytrace_C2 and on the
    benchmark's workload (the reference's own values give 2.8 % and 7.9 % at tau = 2^-14)"""
    assert TAU <= 2.0 ** -14
    g, net = _fixture(golden, "C2")
    _, st = _call(_tracer(g, "train", 16), net, _rays(g), True)
    share = st["guard_refined"] / _coarse_points(st)
    print(f"raytrace_C2: refined {st['guard_refined']} of {_coarse_points(st)} coarse points = {100 * share:.2f} %")
    assert 0 < share <= 0.10
    model = bench._build("C2", torch.device("cuda"), 1e-4)
    inp, _ = bench.synthetic_batch(1234, 2048, "cuda")
    assert model.implicit_network.coarse_mode() == 3
    for head in (0, 16):     # the headline's single-pass sampler, the product's lazy one
        model.ray_tracer.sampler_head = head
        model(inp)
        st = dict(model.ray_tracer.last_stats)
        share = st["guard_refined"] / _coarse_points(st)
        print(f"bench workload, head {head}: refined {st['guard_refined']} of {_coarse_points(st)} coarse points = "
              f"{100 * share:.2f} %, max dev {st['guard_max_dev']:.3e}")
        if head == 0:
            assert _coarse_points(st) == 204800 and st["sdf_evals"] == 250260
        assert 0 < share <= 0.10 and not st["guard_tripped"]


def test_captured_step(golden):
    """GraphedTrainStep(deterministic=True) at C2, 512 rays, 3 steps at lr 1e-4 from the same state: the guard's launches
    are driven by device counters, so the captured step replays them, and every parameter ends bit-identical to the run
    with all-fp32 scans"""
    from hashmodnffbanks_idr_amd.model.implicit_differentiable_renderer import IDRNetwork
    from hashmodnffbanks_idr_amd.model.loss import IDRLoss
    from hashmodnffbanks_idr_amd.training.graph_step import GraphedTrainStep
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    finals = []
    for guard in (True, False):
        torch.manual_seed(3)
        model = IDRNetwork(idr_conf("C2")).cuda()
        with torch.no_grad():  # let the hash features matter
            model.implicit_network.lin0.weight_v[:, 3:].normal_(0, 0.02)
            model.implicit_network.embed_model.embedder_obj.table.uniform_(-0.05, 0.05)
        model.train()
        model.implicit_network.guarded_coarse_scans = guard
        inp, gt = bench.synthetic_batch(21, 512, "cuda")
        rs = np.random.RandomState(4)
        inp["object_mask"] = torch.from_numpy(rs.uniform(0, 1, (1, 512)) < 0.8).cuda()
        gt["rgb"] = torch.from_numpy(rs.uniform(-1, 1, (1, 512, 3)).astype(np.float32)).cuda()
        stepper = GraphedTrainStep(model, IDRLoss(eikonal_weight=0.1, mask_weight=100.0, alpha=50.0),
                                   ClipAdam(model.parameters(), lr=1e-4), warmup=2, deterministic=True)
        torch.manual_seed(9)
        for _ in range(3):
            stepper.step(inp, gt)
        assert stepper.g_fb is not None, "graph capture fell back to eager"
        st = model.ray_tracer.last_stats
        assert st["unfinished"] == 0 and st["nonfinite"] == 0 and (st["guard_refined"] > 0) == guard, st
        torch.cuda.synchronize()
        finals.append({n: p.detach().clone() for n, p in model.named_parameters()})
    for n in finals[0]:
        assert torch.equal(finals[0][n], finals[1][n]), f"parameter {n}"
