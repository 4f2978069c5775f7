"""The guarded ray search with quarter tiles in the refinement of the closest-approach rows' list (csrc/hm_trace.hip:
guard_refine(C_GUARD_NC, quarter) -> hm_sdf_fwd(HM_SDF_TILE64_QUARTER)): a list of at most 16 points per workgroup runs
on 16-point quarter tiles, a longer one as before.  HM_TRACE_OVERLAP=1 / =2 are the sequences that refine the list on the
plain 64-point launch / beside the secant chain (tests/test_scan_pool_gpu.py), without quarter tiles: every output is
compared with torch.equal and every counter with ==, at a few hundred rays."""
import numpy as np
import pytest
import torch

from test_scan_pool_gpu import SMALL, _assert_identical, _call, _fixture, _rays, _run, _tracer

pytestmark = pytest.mark.gpu

QUARTER_MAX = 16 * 256      # points of a list that runs quarter tiles (one per workgroup of the refinement launch)


def _all_three(monkeypatch, g, net, rays, head, what):
    serial = _run(monkeypatch, g, net, rays, head, overlap=1)
    before = _run(monkeypatch, g, net, rays, head, overlap=2)
    new = _run(monkeypatch, g, net, rays, head)
    _assert_identical(new, serial, f"{what}: default against overlap 1")
    _assert_identical(new, before, f"{what}: default against overlap 2")
    assert new[1]["guard_refined"] == serial[1]["guard_refined"] and not new[1]["guard_tripped"]
    return new[1]


@pytest.mark.parametrize("head", [0, 16])
@pytest.mark.parametrize("n_rays,mask", [(512, "half"), (1024, "off"), (768, "half")])
def test_short_list_on_quarter_tiles(golden, monkeypatch, n_rays, mask, head):
    """closest-approach scans above 8192 points (about a fifth of the fixture's rays miss the surface: 100 samples each)
    whose marked samples are a list of a few hundred points"""
    g, net = _fixture(golden, "C2")
    st = _all_three(monkeypatch, g, net, _rays(g, n_rays=n_rays, mask=mask), head, f"{n_rays} rays mask {mask} head {head}")
    print(f"{n_rays} rays, mask {mask}, head {head}: sampler {st['sampler_points']} points, closest "
          f"{100 * st['mask_loss_rays']}, refined {st['guard_refined']}")
    assert 100 * st["mask_loss_rays"] > SMALL and st["guard_refined"] > 0


@pytest.mark.parametrize("head", [0, 16])
def test_scan_below_the_small_tile_limit(golden, monkeypatch, head):
    """64 rays outside the object mask: a closest-approach scan of at most 6400 points runs on the exact small tiles,
    marks nothing, and the quarter launch sees an empty list (no pool, no filler)"""
    g, net = _fixture(golden, "C2")
    st = _all_three(monkeypatch, g, net, _rays(g, n_rays=64, mask="off"), head, f"small scan head {head}")
    assert 0 < 100 * st["mask_loss_rays"] <= SMALL and st["sampler_points"] <= SMALL and st["guard_refined"] == 0


@pytest.mark.parametrize("head", [0, 16])
def test_no_closest_row(golden, monkeypatch, head):
    """rays that end on the surface with the object mask on: no closest-approach row, an empty scan and an empty list"""
    g, net = _fixture(golden, "C2")
    index = np.arange(g["ray_dirs"].shape[1])
    for _ in range(4):     # (a smaller batch marches on other tile sizes: a ray may change sides in the last bit)
        (_, hit, _), st = _run(monkeypatch, g, net, _rays(g, mask="on", index=index), 0, overlap=1)
        if st["mask_loss_rays"] == 0:
            break
        index = index[hit.reshape(-1).cpu().numpy()]
    st = _all_three(monkeypatch, g, net, _rays(g, mask="on", index=index), head, f"no closest row head {head}")
    assert st["mask_loss_rays"] == 0


def test_list_above_the_quarter_limit(golden, monkeypatch):
    """a tripped guard refines every point of the closest-approach scan (512 rays: 9000 points > 16 x 256): the flagged
    launch runs the schedule of the plain one.  Outputs: those of the all-fp32 scans; counts: those of the HM_TRACE_OVERLAP=1 sequence"""
    g, net = _fixture(golden, "C2")
    rays = _rays(g, n_rays=512, mask="half")
    monkeypatch.delenv("HM_TRACE_OVERLAP", raising=False)
    off = _call(_tracer(g, 0), net, rays, guard=False)
    plain = ("sampler_rays", "secant_rays", "mask_loss_rays", "sdf_evals", "unfinished", "nonfinite", "sampler_points",
             "sampler_second_pass_rays")
    after = {}
    for ov in (None, "1"):
        if ov:
            monkeypatch.setenv("HM_TRACE_OVERLAP", ov)
        rt = _tracer(g, 0)
        monkeypatch.setenv("HM_TRACE_GUARD_NOISE", "0.75")
        noisy = _call(rt, net, rays)
        monkeypatch.delenv("HM_TRACE_GUARD_NOISE")
        after[ov] = _call(rt, net, rays)
        monkeypatch.delenv("HM_TRACE_OVERLAP", raising=False)
        _assert_identical(noisy, off, f"overlap {ov}: noise 0.75", plain)
        _assert_identical(after[ov], off, f"overlap {ov}: tripped", plain)
        assert after[ov][1]["guard_tripped"]
    nc = 100 * after[None][1]["mask_loss_rays"]
    assert nc > SMALL and nc > QUARTER_MAX and after[None][1]["guard_refined"] == after["1"][1]["guard_refined"] >= nc
    assert after[None][1]["guard_max_dev"] == after["1"][1]["guard_max_dev"]
