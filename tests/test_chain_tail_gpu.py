"""The secant chain cut in two launches (csrc/hm_trace.hip: k_tail; hm_sdf.hip: sdf_split_scan_secant_kernel for the first
rounds beside the rest of the closest-approach scan, sdf_scan_secant_kernel<., true> for the last rounds beside the quarter
tiles that refine the closest-approach rows' marks).  The chain's state lives in global memory between rounds and a tile's
values depend on neither the workgroup nor the launch that runs it, so the cut changes no bit: every output is compared
with torch.equal and every counter with == between HM_TRACE_CHAIN_TAIL=0 (the chain in one launch, the list in a launch of
its own behind it) and the default, and between 0 and the tail lengths the switch sets."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import make_idr, make_implicit

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REFINED = json.load(open(os.path.join(HERE, "golden", "guard_refined_counts.json")))["guard_refined"]
COUNTERS = ("sdf_evals", "guard_refined", "guard_max_dev", "secant_rays", "mask_loss_rays", "unfinished", "nonfinite")
UNDER_NOISE = tuple(k for k in COUNTERS if k not in ("guard_refined", "guard_max_dev"))     # (see test_noisy_approximate_values)
_NETS = {}
_PARENT = {}


def _fixture(golden, tag):
    if tag not in _NETS:
        g = golden(f"raytrace_{tag}")
        net = make_implicit("C2" if tag == "C2" else "C1", (512,) * 8, 256, int(g["seed"]), float(g["perturb"]),
                            float(g["table_scale"]), bias=float(g["bias"]) if "bias" in g.files else 0.6)
        net.eval()
        _NETS[tag] = (g, net)
    return _NETS[tag]


def _tracer(g, head, n_secant=8, train=True):
    from hashmodnffbanks_idr_amd.model.ray_tracing import RayTracing
    rt = RayTracing(1.0, 5.0e-5, 0.5, 3, 10, 100, n_secant).cuda()
    rt.train(train)
    rt.sampler_head = head
    rt.steps_override = torch.from_numpy(g["steps"])
    return rt


def _rays(g, mask="fixture"):
    cam, dirs, om = g["cam_loc"], g["ray_dirs"], g["object_mask"].copy()
    if mask == "off":
        om[...] = False
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return T(cam), T(om), T(dirs)


def _call(rt, net, rays):
    assert net.coarse_mode() == 3
    with torch.no_grad():
        out = rt(sdf=net.sdf, cam_loc=rays[0], object_mask=rays[1], ray_directions=rays[2])
    return out, dict(rt.last_stats)


def _run(monkeypatch, golden, tag, head, tail, n_secant=8, train=True, mask="fixture", noise=None):
    """one call on a tracer of its own under HM_TRACE_CHAIN_TAIL=tail (None: unset) and HM_TRACE_GUARD_NOISE=noise; the
    HM_TRACE_CHAIN_TAIL=0 result of a case is computed once"""
    key = (tag, head, n_secant, train, mask, noise)
    if tail == 0 and key in _PARENT:
        return _PARENT[key]
    g, net = _fixture(golden, tag)
    for name, val in (("HM_TRACE_CHAIN_TAIL", tail), ("HM_TRACE_GUARD_NOISE", noise)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    monkeypatch.delenv("HM_TRACE_OVERLAP", raising=False)
    monkeypatch.delenv("HM_TRACE_POOL_CHAIN_TILES", raising=False)
    try:
        res = _call(_tracer(g, head, n_secant, train), net, _rays(g, mask))
    finally:
        monkeypatch.delenv("HM_TRACE_CHAIN_TAIL", raising=False)
        monkeypatch.delenv("HM_TRACE_GUARD_NOISE", raising=False)
    if tail == 0:
        _PARENT[key] = res
    return res


def _assert_identical(new, old, what, counters=COUNTERS, tripped=True):
    (o1, s1), (o2, s2) = new, old
    for name, x, y in zip(("points", "mask", "dists"), o1, o2):
        assert torch.equal(x, y), f"{what}: {name} differ in {int((x != y).sum())} entries"
    for k in counters:
        assert s1[k] == s2[k], f"{what}: counter {k}: {s1[k]} != {s2[k]}"
    assert not tripped or s1["guard_tripped"] == s2["guard_tripped"], what


@pytest.mark.parametrize("head", [0, 16])
@pytest.mark.parametrize("tag", ["init", "bumpy", "C2"])
def test_default_against_uncut_chain(golden, monkeypatch, tag, head):
    old = _run(monkeypatch, golden, tag, head, 0)
    new = _run(monkeypatch, golden, tag, head, None)
    st = new[1]
    print(f"{tag} head {head}: secant rays {st['secant_rays']}, closest rows {st['mask_loss_rays']}, refined "
          f"{st['guard_refined']}, max dev {st['guard_max_dev']:.3e}, evals {st['sdf_evals']}")
    _assert_identical(new, old, f"{tag} head {head}")
    assert st["unfinished"] == 0 and st["nonfinite"] == 0 and not st["guard_tripped"]
    key = f"{tag} train head {head}"
    if key in REFINED:
        assert st["guard_refined"] == old[1]["guard_refined"] == REFINED[key], key


@pytest.mark.parametrize("head", [0, 16])
@pytest.mark.parametrize("n_secant", [1, 2, 3, 8])
@pytest.mark.parametrize("tag", ["init", "bumpy", "C2"])
def test_chain_lengths(golden, monkeypatch, tag, n_secant, head):
    """chains of 1 and 2 rounds are not cut (the tail is 2 rounds: nothing would be left in front of it); 3 is the smallest
    cut chain: one round beside the scan, two beside the list"""
    old = _run(monkeypatch, golden, tag, head, 0, n_secant=n_secant)
    new = _run(monkeypatch, golden, tag, head, None, n_secant=n_secant)
    _assert_identical(new, old, f"{tag} head {head} chain of {n_secant}")
    assert new[1]["unfinished"] == 0 and new[1]["nonfinite"] == 0


@pytest.mark.parametrize("head", [0, 16])
@pytest.mark.parametrize("tail", [1, 2, 3])
@pytest.mark.parametrize("tag", ["init", "bumpy", "C2"])
def test_tail_lengths_by_the_switch(golden, monkeypatch, tag, tail, head):
    old = _run(monkeypatch, golden, tag, head, 0)
    _assert_identical(_run(monkeypatch, golden, tag, head, tail), old, f"{tag} head {head} tail {tail}")
    # (a tail as long as the chain: not cut)
    old3 = _run(monkeypatch, golden, tag, head, 0, n_secant=3)
    _assert_identical(_run(monkeypatch, golden, tag, head, tail, n_secant=3), old3, f"{tag} head {head} tail {tail} of 3")


@pytest.mark.parametrize("head", [0, 16])
@pytest.mark.parametrize("tag", ["init", "bumpy", "C2"])
def test_no_secant_ray(golden, monkeypatch, tag, head):
    """object mask off everywhere: no ray enters the secant refinement, which only the device knows - the launch behind the
    cut is the list's alone"""
    old = _run(monkeypatch, golden, tag, head, 0, mask="off")
    new = _run(monkeypatch, golden, tag, head, None, mask="off")
    _assert_identical(new, old, f"{tag} head {head} no secant ray")
    assert new[1]["secant_rays"] == 0 and new[1]["mask_loss_rays"] > 0


@pytest.mark.parametrize("head", [0, 16])
@pytest.mark.parametrize("tag", ["init", "bumpy", "C2"])
def test_no_closest_row(golden, monkeypatch, tag, head):
    """eval mode: no closest-approach rows, no pooled sequence - the switch changes nothing"""
    old = _run(monkeypatch, golden, tag, head, 0, train=False)
    new = _run(monkeypatch, golden, tag, head, None, train=False)
    _assert_identical(new, old, f"{tag} head {head} eval")
    assert new[1]["mask_loss_rays"] == 0
    key = f"{tag} eval head {head}"
    if key in REFINED:
        assert new[1]["guard_refined"] == REFINED[key], key


@pytest.mark.parametrize("head", [0, 16])
@pytest.mark.parametrize("noise", ["0.9", "nan:7"])
@pytest.mark.parametrize("tag", ["init", "bumpy", "C2"])
def test_noisy_approximate_values(golden, monkeypatch, tag, noise, head):
    """approximate values off by up to 0.9 tau (which also trips the monitor), or every 7th of them NaN / Inf: far longer
    lists behind the cut.  The test noise is a function of a sample's slot, and the slots of the compact ray lists come from
    atomic tickets: which samples are disturbed, and with them guard_refined and guard_max_dev, differ from call to call of
    ONE sequence (tests/test_scan_pool_gpu.py, test_tripped_guard: 42 251 .. 42 265) - those two are bounded here; every
    output and every other counter is compared as everywhere."""
    old = _run(monkeypatch, golden, tag, head, 0, noise=noise)
    new = _run(monkeypatch, golden, tag, head, None, noise=noise)
    print(f"{tag} head {head} noise {noise}: refined {new[1]['guard_refined']} (uncut chain {old[1]['guard_refined']}), "
          f"max dev {new[1]['guard_max_dev']:.3e} ({old[1]['guard_max_dev']:.3e}), tripped {new[1]['guard_tripped']}")
    _assert_identical(new, old, f"{tag} head {head} noise {noise}", UNDER_NOISE)
    clean = _run(monkeypatch, golden, tag, head, 0)
    _assert_identical(new, clean, f"{tag} head {head} noise {noise} against the clean call", UNDER_NOISE, tripped=False)
    coarse = clean[1]["sampler_points"] + 100 * clean[1]["mask_loss_rays"] + 17 * clean[1]["sampler_second_pass_rays"]
    for st in (new[1], old[1]):
        assert (st["guard_refined"] > 0) == (clean[1]["guard_refined"] > 0) and st["guard_refined"] <= coarse
        assert noise == "0.9" or not st["guard_tripped"]


@pytest.mark.parametrize("head", [0, 16])
@pytest.mark.parametrize("tag", ["init", "bumpy", "C2"])
def test_forced_trip_largest_list(golden, monkeypatch, tag, head):
    """noise of 0.75 tau on the sampler's launch trips the monitor; the call after it marks EVERY closest-approach sample:
    the list behind the cut is n_sel x n_steps points - full 64-point tiles over many rounds, which the secant's workgroups
    join when their rounds are done.  The call after the trip is compared in every counter."""
    g, net = _fixture(golden, tag)
    rays = _rays(g)
    results = {}
    for tail in ("0", None):
        if tail is None:
            monkeypatch.delenv("HM_TRACE_CHAIN_TAIL", raising=False)
        else:
            monkeypatch.setenv("HM_TRACE_CHAIN_TAIL", tail)
        rt = _tracer(g, head)
        monkeypatch.setenv("HM_TRACE_GUARD_NOISE", "0.75")
        noisy = _call(rt, net, rays)
        monkeypatch.delenv("HM_TRACE_GUARD_NOISE")
        after = _call(rt, net, rays)
        monkeypatch.delenv("HM_TRACE_CHAIN_TAIL", raising=False)
        results[tail] = (noisy, after)
    (n_old, a_old), (n_new, a_new) = results["0"], results[None]
    print(f"{tag} head {head}: refined in the tripping call {n_new[1]['guard_refined']} (uncut chain "
          f"{n_old[1]['guard_refined']}), in the call after {a_new[1]['guard_refined']}")
    _assert_identical(n_new, n_old, f"{tag} head {head} tripping call", UNDER_NOISE)
    _assert_identical(a_new, a_old, f"{tag} head {head} call after the trip")
    assert n_new[1]["guard_tripped"] and a_new[1]["guard_tripped"]
    if 100 * a_new[1]["mask_loss_rays"] > 8192:       # (shorter scans are exact already: nothing to mark)
        assert a_new[1]["guard_refined"] >= 100 * a_new[1]["mask_loss_rays"]


def test_captured_step(golden, monkeypatch):
    """the captured training step at the benchmarked configuration (idr_step_C2: C2, 2048 rays), lr 0, three replays from
    the same draws: default against HM_TRACE_CHAIN_TAIL=0 (read when the step is captured).  points, masks, sdf_output and
    the loss terms bit for bit; gradients within 4 x the atomic-order noise that replays of the SAME sequence show (the
    uncut chain's three replays and a second run of it)."""
    from hashmodnffbanks_idr_amd.model.loss import IDRLoss
    from hashmodnffbanks_idr_amd.training.graph_step import GraphedTrainStep
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    g = golden("idr_step_C2")
    inp = {k: torch.from_numpy(g[k]).cuda() for k in ("intrinsics", "uv", "pose", "object_mask")}
    gt = {"rgb": torch.from_numpy(g["rgb_gt"]).cuda()}
    exact = ("points", "network_object_mask", "object_mask", "sdf_output")

    def run(tail):
        if tail is None:
            monkeypatch.delenv("HM_TRACE_CHAIN_TAIL", raising=False)
        else:
            monkeypatch.setenv("HM_TRACE_CHAIN_TAIL", tail)
        model = make_idr("C2", int(g["seed"]), float(g["bias"]) if "bias" in g.files else 0.6)
        model.train()
        assert model.implicit_network.coarse_mode() == 3
        stepper = GraphedTrainStep(model, IDRLoss(eikonal_weight=0.1, mask_weight=100.0, alpha=50.0),
                                   ClipAdam(model.parameters(), lr=0.0, max_norm=1.0), warmup=2)
        steps = []
        for it in range(2 + 3):
            torch.manual_seed(1000)
            out, lo = stepper.step(inp, gt)
            if it >= 2:
                torch.cuda.synchronize()
                steps.append(({k: out[k].detach().clone() for k in exact}, {k: v.detach().clone() for k, v in lo.items()},
                              {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None},
                              dict(model.ray_tracer.last_stats)))
        assert stepper.g_fb is not None, "graph capture fell back to eager"
        monkeypatch.delenv("HM_TRACE_CHAIN_TAIL", raising=False)
        return steps

    old, old2, new = run("0"), run("0"), run(None)
    noise = {n: 0.0 for n in old[0][2]}
    for a in old + old2:
        for n in noise:
            noise[n] = max(noise[n], float((a[2][n] - old[0][2][n]).abs().max()))
    worst = (0.0, 0.0, "")
    for s_new, s_old in zip(new, old):
        for k in exact:
            assert torch.equal(s_new[0][k], s_old[0][k]), k
        for k in s_old[1]:
            assert torch.equal(s_new[1][k], s_old[1][k]), f"loss term {k}"
        for k in COUNTERS:
            assert s_new[3][k] == s_old[3][k], k
        assert s_new[3]["guard_refined"] > 0 and s_new[3]["unfinished"] == 0 and s_new[3]["nonfinite"] == 0
        for n in noise:
            d = float((s_new[2][n] - old[0][2][n]).abs().max())
            worst = max(worst, (d, noise[n], n))
            assert d <= 4.0 * noise[n], f"gradient of {n}: {d:.3e} against same-sequence noise {noise[n]:.3e}"
    print(f"captured step: largest gradient difference {worst[0]:.3e} ({worst[2]}, same-sequence noise {worst[1]:.3e}); "
          f"largest same-sequence noise {max(noise.values()):.3e}; stats {new[-1][3]}")
