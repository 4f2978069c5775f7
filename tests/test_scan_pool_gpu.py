"""The closest-approach scan shared out between the launches of the guarded search (csrc/hm_trace.hip: pool;
csrc/hm_scan_pool.h).  By default the refine-scan launches in front of the secant chain take only as many of the scan's split
tiles as they have idle workgroups (plus what would not fit under the chain), the secant launch
(hm_sdf.hip: sdf_split_scan_secant_kernel) runs the rest beside the chain, and the closest-approach rows are refined behind
it.  HM_TRACE_OVERLAP=2 is the sequence before (whole scan in front of the chain, closest list beside it), =1 every launch
on its own; HM_TRACE_POOL_CHAIN_TILES=k sets the tiles per workgroup the chain is taken to hide.  Same tiles, same tile
bodies, whichever launch and workgroup runs them: every output is compared with torch.equal, every counter with ==."""
import numpy as np
import pytest
import torch

import bench
from helpers import idr_conf, make_implicit

pytestmark = pytest.mark.gpu

SMALL = 8192     # launches of at most this many live points run on the exact small-tile kernel (nothing to refine)
_NETS = {}
_COUNTS = {}


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


def _run(monkeypatch, g, net, rays, head, overlap=None, chain=None):
    """one call on a tracer of its own under HM_TRACE_OVERLAP=overlap / HM_TRACE_POOL_CHAIN_TILES=chain (None: unset)"""
    for name, val in (("HM_TRACE_OVERLAP", overlap), ("HM_TRACE_POOL_CHAIN_TILES", chain)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    try:
        return _call(_tracer(g, head), net, rays)
    finally:
        monkeypatch.delenv("HM_TRACE_OVERLAP", raising=False)
        monkeypatch.delenv("HM_TRACE_POOL_CHAIN_TILES", raising=False)


def _assert_identical(new, old, what, counters=None):
    (o1, s1), (o2, s2) = new, old
    for name, x, y in zip(("points", "mask", "distances"), o1, o2):
        assert torch.equal(x, y), f"{what}: {name} differ in {int((x != y).sum())} entries"
    for k in (counters or s2):
        assert s1[k] == s2[k], f"{what}: counter {k}: {s1[k]} != {s2[k]}"
    assert s1["unfinished"] == 0 and s1["nonfinite"] == s2["nonfinite"]


def _against_both(monkeypatch, g, net, rays, head, what, chains=(None,)):
    """the default sequence (and the given chain capacities) against HM_TRACE_OVERLAP=1 and =2; returns the default's stats"""
    serial = _run(monkeypatch, g, net, rays, head, overlap=1)
    before = _run(monkeypatch, g, net, rays, head, overlap=2)
    _assert_identical(before, serial, f"{what}: overlap 2 against 1")
    st = None
    for chain in chains:
        new = _run(monkeypatch, g, net, rays, head, chain=chain)
        _assert_identical(new, serial, f"{what}: chain tiles {chain} against overlap 1")
        _assert_identical(new, before, f"{what}: chain tiles {chain} against overlap 2")
        st = st or new[1]
    return st


@pytest.mark.parametrize("head", [0, 16])
@pytest.mark.parametrize("tag", ["init", "bumpy", "C2", "C2_halfmask"])
def test_new_sequence_against_both_others(golden, monkeypatch, tag, head):
    g, net = _fixture(golden, tag.split("_")[0])
    rays = _rays(g, mask="half" if tag.endswith("halfmask") else "fixture")
    st = _against_both(monkeypatch, g, net, rays, head, f"{tag} head {head}")
    print(f"{tag} head {head}: sampler {st['sampler_points']} points, closest {100 * st['mask_loss_rays']}, secant rays "
          f"{st['secant_rays']}, refined {st['guard_refined']}, max dev {st['guard_max_dev']:.3e}")
    assert not st["guard_tripped"]


def _serial_counts(golden, monkeypatch, tag, n_rays, mask):
    key = (tag, n_rays, mask)
    if key not in _COUNTS:
        g, net = _fixture(golden, tag)
        _, st = _run(monkeypatch, g, net, _rays(g, n_rays=n_rays, mask=mask), 0, overlap=1)
        _COUNTS[key] = (st["sampler_points"], 100 * st["mask_loss_rays"])
    return _COUNTS[key]


PREFIXES = (2048, 1024, 512, 256, 128, 96, 64, 1536, 768, 384, 192)


def _search(golden, monkeypatch, accept):
    for tag in ("C2", "bumpy", "init"):
        for mask in ("fixture", "on", "off"):
            for k in PREFIXES:
                ns, nc = _serial_counts(golden, monkeypatch, tag, k, mask)
                if accept(ns, nc):
                    return tag, mask, k, ns, nc
    return None


@pytest.mark.parametrize("closest_big", [False, True])
@pytest.mark.parametrize("sampler_big", [False, True])
def test_counts_around_the_small_tile_limit(golden, monkeypatch, sampler_big, closest_big):
    """single-pass sampler: the sampler's rows and the closest-approach rows are launches of sampler_points and
    100 * mask_loss_rays points; each side of 8192 for either, reached with a ray prefix and an object mask chosen from the
    counts of the serial sequence"""
    found = _search(golden, monkeypatch,
                    lambda ns, nc: (ns > SMALL) == sampler_big and (nc > SMALL) == closest_big and (ns > 0 or nc > 0))
    assert found is not None, f"no prefix / mask of the fixtures gives sampler_big={sampler_big}, closest_big={closest_big}"
    tag, mask, k, ns, nc = found
    g, net = _fixture(golden, tag)
    st = _against_both(monkeypatch, g, net, _rays(g, n_rays=k, mask=mask), 0, f"{found}", chains=(None, 1, 0))
    print(f"sampler_big={sampler_big} closest_big={closest_big}: raytrace_{tag}, {k} rays, mask {mask}: sampler launch "
          f"{st['sampler_points']} points, closest launch {100 * st['mask_loss_rays']}, refined {st['guard_refined']}")
    assert (st["sampler_points"], 100 * st["mask_loss_rays"]) == (ns, nc)
    assert (st["guard_refined"] > 0) == (sampler_big or closest_big)


def _plan(n_scan, n_ref1, n_sec_bound, chain=-1):
    import ctypes
    from hashmodnffbanks_idr_amd import _lib
    first, quota = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    _lib.check(_lib.lib().hm_trace_scan_pool_plan(n_scan, n_ref1, 0, 0, 256, n_sec_bound, 8, chain, first, quota))
    return list(quota)


def test_scan_just_above_the_small_tile_limit(golden, monkeypatch):
    """the smallest closest-approach scan above 8192 points the fixtures' prefixes give, beside a sampler list that leaves
    workgroups idle: the launch in front of the chain takes all of its tiles, the secant launch none"""
    found = None
    for lim in (160, 200, 256, 400):      # tiles
        found = found or _search(golden, monkeypatch, lambda ns, nc: SMALL < nc <= lim * 64 and ns > 0)
    assert found is not None, "no prefix / mask of the fixtures gives a closest-approach scan just above 8192 points"
    tag, mask, k, ns, nc = found
    g, net = _fixture(golden, tag)
    st = _against_both(monkeypatch, g, net, _rays(g, n_rays=k, mask=mask), 0, f"{found}", chains=(None, 1, 0))
    quota = _plan(nc, 0, st["sampler_rays"])       # (an empty list leaves every workgroup idle: the upper bound of X1)
    print(f"scan just above the limit: raytrace_{tag}, {k} rays, mask {mask}: closest launch {nc} points = {-(-nc // 64)} "
          f"tiles, sampler rays {st['sampler_rays']}; ranges with an empty list {quota}")
    assert 100 * st["mask_loss_rays"] == nc and nc > SMALL


def test_large_scan_under_the_chain(golden, monkeypatch):
    """raytrace_C2, the fixtures' largest closest-approach scan (388 rays = 607 tiles whatever the object mask; with secant
    rays beside them where a mask gives both): the secant launch takes a large part of the scan; chain capacities 1 and 0
    send most / all of it back in front"""
    g, net = _fixture(golden, "C2")
    cands = []
    for mask in ("fixture", "half", "off"):
        _, st = _run(monkeypatch, g, net, _rays(g, mask=mask), 0, overlap=1)
        if 100 * st["mask_loss_rays"] > 2 * 256 * 64:
            cands.append((mask, st))
    assert cands, "no mask of raytrace_C2 gives a closest-approach scan of more than two rounds of tiles"
    mask, st1 = next((c for c in cands if c[1]["secant_rays"] > 0), cands[0])
    nc = 100 * st1["mask_loss_rays"]
    quotas = {c: _plan(nc, 64 * 190, st1["sampler_rays"], c) for c in (-1, 1, 0)}
    print(f"large scan: mask {mask}, closest launch {nc} points, secant rays {st1['secant_rays']}, sampler rays "
          f"{st1['sampler_rays']}; ranges (list of 190 tiles) {quotas}")
    assert quotas[-1][2] > 0 and quotas[1][2] <= quotas[-1][2] and quotas[0][2] == 0
    for head in (0, 16):
        _against_both(monkeypatch, g, net, _rays(g, mask=mask), head, f"large scan head {head}", chains=(None, 1, 0))


def test_closest_rows_without_a_secant_ray(golden, monkeypatch):
    """object mask off everywhere: no ray enters the secant refinement (training refines in-mask rays only), every ray the
    sampler does not take is a closest-approach row - the secant launch carries split tiles alone"""
    g, net = _fixture(golden, "C2")
    st = _against_both(monkeypatch, g, net, _rays(g, mask="off"), 0, "no secant ray", chains=(None, 1, 0))
    print(f"no secant ray: {st}")
    assert st["secant_rays"] == 0 and 100 * st["mask_loss_rays"] > SMALL and st["guard_refined"] > 0


def test_sampler_marks_without_a_closest_row(golden, monkeypatch):
    """the rays of raytrace_C2 that end on the surface with the object mask on everywhere: none is a mask-loss ray, so the
    closest-approach scan and its list are empty while the sampler's list is not"""
    g, net = _fixture(golden, "C2")
    index = np.arange(g["ray_dirs"].shape[1])
    for _ in range(4):     # (a smaller batch marches on other tile sizes: a ray may change sides in the last bit)
        (_, hit, _), st = _run(monkeypatch, g, net, _rays(g, mask="on", index=index), 0, overlap=1)
        if st["mask_loss_rays"] == 0:
            break
        index = index[hit.reshape(-1).cpu().numpy()]
    for head in (0, 16):
        st = _against_both(monkeypatch, g, net, _rays(g, mask="on", index=index), head, f"no closest row head {head}")
        assert st["mask_loss_rays"] == 0 and st["sampler_points"] > SMALL and st["guard_refined"] > 0
    print(f"no closest row: {len(index)} rays, {st}")


def test_empty_sampler_list_with_a_large_scan(golden, monkeypatch):
    """a sampler launch of at most 8192 points marks nothing (it is exact already): every workgroup of the launch in front
    of the chain is idle and takes a split tile of a closest-approach scan of several hundred tiles.
    No prefix of the fixtures has both, so: 64 rays of raytrace_C2 inside the object mask (a sampler launch below 8192 points,
    and secant rays) followed by 700 of its rays turned away from the scene outside the mask - they miss the bounding sphere
    and are closest-approach rows, 100 samples each"""
    g, net = _fixture(golden, "C2")
    cam, om, dirs = _rays(g, n_rays=64 + 700, mask="on")
    om[..., 64:] = False
    dirs[:, 64:] = -dirs[:, 64:]
    for head in (0, 16):
        st = _against_both(monkeypatch, g, net, (cam, om, dirs), head, f"empty sampler list head {head}", chains=(None, 1))
        # (at least 49 152 scan points: the secant runs 16-point tiles, as on the bench step)
        assert 0 < st["sampler_points"] <= SMALL and st["mask_loss_rays"] >= 600 and st["secant_rays"] > 0
        assert st["guard_refined"] > 0       # (closest-approach rows only)
    print(f"empty sampler list: {st}")


def test_tripped_guard(golden, monkeypatch):
    """HM_TRACE_GUARD_NOISE=0.75 trips the monitor in the sampler's patch; the closest-approach rows, selected behind it (and
    now behind the secant launch), are refined in full in that call already.  The clean call after it refines every
    approximated point of both lists; the outputs of both calls are those of the all-fp32 scans, and the counts those of both
    other sequences"""
    g, net = _fixture(golden, "C2")
    rays = _rays(g)
    monkeypatch.delenv("HM_TRACE_OVERLAP", raising=False)
    off = _call(_tracer(g, 0), net, rays, guard=False)
    plain = ("sampler_rays", "secant_rays", "mask_loss_rays", "sdf_evals", "unfinished", "nonfinite", "sampler_points",
             "sampler_second_pass_rays")
    results = {}
    for ov in (None, "2", "1"):
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
    (n_new, a_new), (n_two, a_two), (n_old, a_old) = results[None], results["2"], results["1"]
    ns, nc = a_new["sampler_points"], 100 * a_new["mask_loss_rays"]
    print(f"sampler launch {ns} points, closest launch {nc}; refined in the tripping call {n_new['guard_refined']} "
          f"(overlap 2: {n_two['guard_refined']}, serial {n_old['guard_refined']}), in the call after "
          f"{a_new['guard_refined']}")
    assert ns > 1000 * 64 and nc > 2 * 256 * 64
    assert a_new["guard_refined"] == a_two["guard_refined"] == a_old["guard_refined"] == ns + nc
    # (the tripping call's own count is not reproducible in any of the sequences: over three fresh tracers each it was
    #  42 251 .. 42 265 here, 42 248 .. 42 260 with HM_TRACE_OVERLAP=2 and 5 080 .. 5 089 with =1 - bounds only)
    for n_seq in (n_new, n_two):
        assert n_old["guard_refined"] <= n_seq["guard_refined"] <= ns + nc
    assert a_new["guard_max_dev"] == a_two["guard_max_dev"] == a_old["guard_max_dev"]


def test_captured_step(monkeypatch):
    """GraphedTrainStep(deterministic=True) at C2, 512 rays: the captured step replays the new launches (device counters
    and cursors, zeroed inside the call); over two eager and three replayed steps the counters and in the end every
    parameter are those of the HM_TRACE_OVERLAP=1 step"""
    from hashmodnffbanks_idr_amd.model.implicit_differentiable_renderer import IDRNetwork
    from hashmodnffbanks_idr_amd.model.loss import IDRLoss
    from hashmodnffbanks_idr_amd.training.graph_step import GraphedTrainStep
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    finals, stats = [], []
    for ov in (None, "1"):
        monkeypatch.delenv("HM_TRACE_POOL_CHAIN_TILES", raising=False)
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
