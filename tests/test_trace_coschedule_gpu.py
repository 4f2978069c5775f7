"""Co-scheduled guard refinements (csrc/hm_trace.hip: cosched).  With guarded coarse scans, training, the tile size left to
the library and a secant refinement, the exact refinement of the sampler's marked samples runs in the launch of the
closest-approach rows' split tiles (hm_sdf.hip: sdf_refine_scan_kernel) and the refinement of the closest-approach rows'
marks in the launch of the secant chain (sdf_scan_secant_kernel with that list as its scan).  HM_TRACE_OVERLAP=1 (read per
call) is the sequence before: every launch on its own, one refinement list.  Same tiles, same tile bodies: every output
and every counter is compared with torch.equal / ==."""
import numpy as np
import pytest
import torch

import bench
from helpers import idr_conf, make_implicit

pytestmark = pytest.mark.gpu

SMALL = 8192     # launches of at most this many live points run on the exact small-tile kernel (nothing to refine)
_NETS = {}
_SERIAL = {}


def _fixture(golden, tag):
    if tag not in _NETS:
        g = golden(f"raytrace_{tag}")
        net = make_implicit("C2" if tag == "C2" else "C1", (512,) * 8, 256, int(g["seed"]), float(g["perturb"]),
                            float(g["table_scale"]), bias=float(g["bias"]) if "bias" in g.files else 0.6)
        net.eval()
        _NETS[tag] = (g, net)
    return _NETS[tag]


def _tracer(g, head):
    from hashmodnffbanks_idr_amd.model.ray_tracing import RayTracing
    rt = RayTracing(1.0, 5.0e-5, 0.5, 3, 10, 100, 8).cuda()
    rt.train(True)
    rt.sampler_head = head
    rt.steps_override = torch.from_numpy(g["steps"])
    return rt


def _rays(g, n_rays=None, mask="fixture", index=None):
    """a prefix (n_rays) or a subset (index) of the fixture's rays; mask: fixture | half | on | off"""
    cam, dirs, om = g["cam_loc"], g["ray_dirs"], g["object_mask"].copy()
    if mask == "half":
        om.reshape(-1)[::2] = False
    elif mask in ("on", "off"):
        om[...] = mask == "on"
    if index is not None:
        dirs, om = dirs[:, index], om[..., index]
    if n_rays is not None:
        dirs, om = dirs[:, :n_rays], om[..., :n_rays]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return T(cam), T(om), T(dirs)


def _call(rt, net, rays, guard=True):
    net.guarded_coarse_scans = guard
    try:
        with torch.no_grad():
            out = rt(sdf=net.sdf, cam_loc=rays[0], object_mask=rays[1], ray_directions=rays[2])
        return out, dict(rt.last_stats)
    finally:
        net.guarded_coarse_scans = True


def _pair(monkeypatch, g, net, rays, head):
    """(new sequence, HM_TRACE_OVERLAP=1), each on a tracer of its own"""
    monkeypatch.delenv("HM_TRACE_OVERLAP", raising=False)
    new = _call(_tracer(g, head), net, rays)
    monkeypatch.setenv("HM_TRACE_OVERLAP", "1")
    old = _call(_tracer(g, head), net, rays)
    monkeypatch.delenv("HM_TRACE_OVERLAP")
    return new, old


def _assert_identical(new, old, what, counters=None):
    (o1, s1), (o2, s2) = new, old
    for name, x, y in zip(("points", "mask", "distances"), o1, o2):
        assert torch.equal(x, y), f"{what}: {name} differ in {int((x != y).sum())} entries"
    for k in (counters or s2):
        assert s1[k] == s2[k], f"{what}: counter {k}: {s1[k]} != {s2[k]}"
    assert s1["unfinished"] == 0 and s1["nonfinite"] == s2["nonfinite"]


@pytest.mark.parametrize("head", [0, 16])
@pytest.mark.parametrize("tag", ["init", "bumpy", "C2", "C2_halfmask"])
def test_new_sequence_against_serial(golden, monkeypatch, tag, head):
    g, net = _fixture(golden, tag.split("_")[0])
    rays = _rays(g, mask="half" if tag.endswith("halfmask") else "fixture")
    new, old = _pair(monkeypatch, g, net, rays, head)
    st = new[1]
    print(f"{tag} head {head}: sampler {st['sampler_points']} points, closest {100 * st['mask_loss_rays']}, secant rays "
          f"{st['secant_rays']}, refined {st['guard_refined']} (serial {old[1]['guard_refined']}), max dev "
          f"{st['guard_max_dev']:.3e}")
    _assert_identical(new, old, f"{tag} head {head}")
    assert not st["guard_tripped"]


def _serial_counts(golden, monkeypatch, tag, n_rays, mask):
    key = (tag, n_rays, mask)
    if key not in _SERIAL:
        g, net = _fixture(golden, tag)
        monkeypatch.setenv("HM_TRACE_OVERLAP", "1")
        _, st = _call(_tracer(g, 0), net, _rays(g, n_rays=n_rays, mask=mask))
        monkeypatch.delenv("HM_TRACE_OVERLAP")
        _SERIAL[key] = (st["sampler_points"], 100 * st["mask_loss_rays"])
    return _SERIAL[key]


PREFIXES = (2048, 1024, 512, 256, 128, 96, 64, 1536, 768, 384, 192)


@pytest.mark.parametrize("closest_big", [False, True])
@pytest.mark.parametrize("sampler_big", [False, True])
def test_counts_around_the_small_tile_limit(golden, monkeypatch, sampler_big, closest_big):
    """single-pass sampler: the sampler's rows and the closest-approach rows are launches of sampler_points and
    100 * mask_loss_rays points; each side of 8192 for either, reached with a ray prefix and an object mask chosen from the
    counts of the serial sequence"""
    found = None
    for tag in ("C2", "bumpy", "init"):
        for mask in ("fixture", "on", "off"):
            for k in PREFIXES:
                ns, nc = _serial_counts(golden, monkeypatch, tag, k, mask)
                if (ns > SMALL) == sampler_big and (nc > SMALL) == closest_big and (ns > 0 or nc > 0):
                    found = (tag, mask, k, ns, nc)
                    break
            if found:
                break
        if found:
            break
    assert found is not None, f"no prefix / mask of the fixtures gives sampler_big={sampler_big}, closest_big={closest_big}"
    tag, mask, k, ns, nc = found
    g, net = _fixture(golden, tag)
    new, old = _pair(monkeypatch, g, net, _rays(g, n_rays=k, mask=mask), 0)
    st = new[1]
    print(f"sampler_big={sampler_big} closest_big={closest_big}: raytrace_{tag}, {k} rays, mask {mask}: sampler launch "
          f"{st['sampler_points']} points, closest launch {100 * st['mask_loss_rays']}, refined {st['guard_refined']}")
    assert (st["sampler_points"], 100 * st["mask_loss_rays"]) == (ns, nc)
    assert (st["sampler_points"] > SMALL) == sampler_big and (100 * st["mask_loss_rays"] > SMALL) == closest_big
    _assert_identical(new, old, f"{found}")
    assert (st["guard_refined"] > 0) == (sampler_big or closest_big)


def test_closest_rows_without_a_secant_ray(golden, monkeypatch):
    """object mask off everywhere: no ray enters the secant refinement (training refines in-mask rays only), every ray the
    sampler does not take is a closest-approach row - the secant launch carries the closest list alone"""
    g, net = _fixture(golden, "C2")
    new, old = _pair(monkeypatch, g, net, _rays(g, mask="off"), 0)
    st = new[1]
    print(f"no secant ray: {st}")
    assert st["secant_rays"] == 0 and 100 * st["mask_loss_rays"] > SMALL and st["guard_refined"] > 0
    _assert_identical(new, old, "no secant ray")


def test_sampler_marks_without_a_closest_row(golden, monkeypatch):
    """the rays of raytrace_C2 that end on the surface with the object mask on everywhere: none is a mask-loss ray, so the
    closest-approach scan and its list are empty while the sampler's list is not"""
    g, net = _fixture(golden, "C2")
    index = np.arange(g["ray_dirs"].shape[1])
    monkeypatch.setenv("HM_TRACE_OVERLAP", "1")
    for _ in range(4):     # (a smaller batch marches on other tile sizes: a ray may change sides in the last bit)
        (_, hit, _), st = _call(_tracer(g, 0), net, _rays(g, mask="on", index=index))
        if st["mask_loss_rays"] == 0:
            break
        index = index[hit.reshape(-1).cpu().numpy()]
    monkeypatch.delenv("HM_TRACE_OVERLAP")
    new, old = _pair(monkeypatch, g, net, _rays(g, mask="on", index=index), 0)
    st = new[1]
    print(f"no closest row: {len(index)} rays, {st}")
    assert st["mask_loss_rays"] == 0 and st["sampler_points"] > SMALL and st["guard_refined"] > 0
    _assert_identical(new, old, "no closest row")


def test_tripped_guard(golden, monkeypatch):
    """HM_TRACE_GUARD_NOISE=0.75 trips the monitor in the sampler's patch; the closest-approach rows, selected behind it, are
    then refined in full in that call already (HM_TRACE_OVERLAP=1: from the next call on).  The clean call after it refines
    every approximated point of both lists - 2575 and 607 fp32 tiles through the two cursors - and the outputs of both calls
    are those of the all-fp32 scans"""
    g, net = _fixture(golden, "C2")
    rays = _rays(g)
    monkeypatch.delenv("HM_TRACE_OVERLAP", raising=False)
    off = _call(_tracer(g, 0), net, rays, guard=False)
    plain = ("sampler_rays", "secant_rays", "mask_loss_rays", "sdf_evals", "unfinished", "nonfinite", "sampler_points",
             "sampler_second_pass_rays")
    results = {}
    for ov in (None, "1"):
        if ov:
            monkeypatch.setenv("HM_TRACE_OVERLAP", ov)
        rt = _tracer(g, 0)
        monkeypatch.setenv("HM_TRACE_GUARD_NOISE", "0.75")
        noisy = _call(rt, net, rays)
        monkeypatch.delenv("HM_TRACE_GUARD_NOISE")
        after = _call(rt, net, rays)
        monkeypatch.delenv("HM_TRACE_OVERLAP", raising=False)
        _assert_identical(noisy, off, f"overlap {ov}: noise 0.75", plain)
        _assert_identical(after, off, f"overlap {ov}: tripped", plain)
        assert noisy[1]["guard_tripped"] and after[1]["guard_tripped"]
        results[ov] = (noisy[1], after[1])
    (n_new, a_new), (n_old, a_old) = results[None], results["1"]
    ns, nc = a_new["sampler_points"], 100 * a_new["mask_loss_rays"]
    print(f"sampler launch {ns} points, closest launch {nc}; refined in the tripping call {n_new['guard_refined']} "
          f"(serial {n_old['guard_refined']}), in the call after {a_new['guard_refined']} (serial {a_old['guard_refined']})")
    # raytrace_C2: 2575 fp32 tiles in the sampler's list, 607 in the closest-approach rows' (1648 of its 2048 rays are sampler
    # rays) - several tiles per workgroup through either cursor
    assert ns > 1000 * 64 and nc > 2 * 256 * 64
    assert a_new["guard_refined"] == a_old["guard_refined"] == ns + nc
    assert n_old["guard_refined"] <= n_new["guard_refined"] <= ns + nc
    assert a_new["guard_max_dev"] == a_old["guard_max_dev"]


def test_captured_step(monkeypatch):
    """GraphedTrainStep(deterministic=True) at C2, 512 rays: the captured step replays the co-scheduled launches (device
    counters and cursors, zeroed inside the call); over three replays the counters and in the end every parameter are those
    of the HM_TRACE_OVERLAP=1 step"""
    from hashmodnffbanks_idr_amd.model.implicit_differentiable_renderer import IDRNetwork
    from hashmodnffbanks_idr_amd.model.loss import IDRLoss
    from hashmodnffbanks_idr_amd.training.graph_step import GraphedTrainStep
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    finals, stats = [], []
    for ov in (None, "1"):
        if ov:
            monkeypatch.setenv("HM_TRACE_OVERLAP", ov)     # (read when the step is captured)
        torch.manual_seed(3)
        model = IDRNetwork(idr_conf("C2")).cuda()
        with torch.no_grad():  # let the hash features matter
            model.implicit_network.lin0.weight_v[:, 3:].normal_(0, 0.02)
            model.implicit_network.embed_model.embedder_obj.table.uniform_(-0.05, 0.05)
        model.train()
        assert model.implicit_network.coarse_mode() == 3
        inp, gt = bench.synthetic_batch(21, 512, "cuda")
        rs = np.random.RandomState(4)
        inp["object_mask"] = torch.from_numpy(rs.uniform(0, 1, (1, 512)) < 0.8).cuda()
        gt["rgb"] = torch.from_numpy(rs.uniform(-1, 1, (1, 512, 3)).astype(np.float32)).cuda()
        stepper = GraphedTrainStep(model, IDRLoss(eikonal_weight=0.1, mask_weight=100.0, alpha=50.0),
                                   ClipAdam(model.parameters(), lr=1e-4), warmup=2, deterministic=True)
        torch.manual_seed(9)
        per_step = []
        for _ in range(3 + 2):     # two eager warm-up steps, then three replays
            stepper.step(inp, gt)
            per_step.append(dict(model.ray_tracer.last_stats))
        assert stepper.g_fb is not None, "graph capture fell back to eager"
        monkeypatch.delenv("HM_TRACE_OVERLAP", raising=False)
        torch.cuda.synchronize()
        stats.append(per_step)
        finals.append({n: p.detach().clone() for n, p in model.named_parameters()})
    print(f"captured step: last replay {stats[0][-1]}")
    for s_new, s_old in zip(*stats):
        assert s_new == s_old and s_new["guard_refined"] > 0 and s_new["unfinished"] == 0 and s_new["nonfinite"] == 0
    for n in finals[0]:
        assert torch.equal(finals[0][n], finals[1][n]), f"parameter {n}"
