"""The generic (torch op) tracer of model/ray_tracing.py against oracle/ray_ref.RayTraceRef over the tracer's
configuration space (tests/trace_cases.py), on the CPU with analytic elementwise fp32 SDFs.

Both are fp32 restatements of the same elementwise expressions and the SDFs give a point the same value in any batch,
so the comparison is exact: torch.equal on mask, distances and points, equal numbers of SDF evaluations.  The device
tracer is tied to the generic one in test_raytrace_configs_gpu.py; this file ties the generic one to the oracle, which
tests/test_oracle_golden.py pins to the reference's outputs at the bench setting.

The second half asserts, from the ORACLE's side only (its call log and counts), that every configuration reaches the
branch it is listed for with these inputs."""
import functools

import pytest
import torch

import trace_cases as TC
from oracle import ray_ref

MODES = ("train", "eval")


class LoggedRef(ray_ref.RayTraceRef):
    """RayTraceRef that notes how many rays each stage received and the size of every SDF call"""

    def __init__(self, *args):
        super().__init__(*args)
        self.log = {"sampler": 0, "secant": 0, "closest": 0, "calls": []}

    def _sdf(self, sdf, pts):
        self.log["calls"].append(int(pts.shape[0]))
        return super()._sdf(sdf, pts)

    def _sample(self, sdf, cams, dirs, object_mask, t_near, t_far, which):
        self.log["sampler"] = int(which.sum())
        return super()._sample(sdf, cams, dirs, object_mask, t_near, t_far, which)

    def _secant(self, sdf, v_lo, v_hi, z_lo, z_hi, c, d):
        self.log["secant"] = int(c.shape[0])
        return super()._secant(sdf, v_lo, v_hi, z_lo, z_hi, c, d)

    def _closest(self, sdf, c, d, lo, hi):
        self.log["closest"] = int(c.shape[0])
        return super()._closest(sdf, c, d, lo, hi)


@functools.lru_cache(maxsize=None)
def oracle_run(name, mode, layout, sdf_name):
    """((points, mask, dists), log) of the oracle; log also holds 'evals', 'hit' (rays that meet the bounding sphere) and
    'rays'.  Cached: the branch assertions below reuse the runs of the comparison."""
    case = TC.CONFIGS[name]
    cam, dirs, om = TC.rays(layout)
    rt = LoggedRef(*TC.tracer_args(case))
    rt.training = mode == "train"
    rt.steps = TC.steps(case.n_steps)
    with torch.no_grad():
        out = rt(TC.SDFS[sdf_name], cam, om, dirs)
        _, hit = ray_ref.sphere_intersection(cam, dirs, case.radius)
    log = dict(rt.log, evals=rt.sdf_evals, hit=int(hit.sum()), rays=hit.numel(), net=int(out[1].sum()))
    return out, log


def generic_run(name, mode, layout, sdf_name):
    from hashmodnffbanks_idr_amd.model.ray_tracing import RayTracing
    case = TC.CONFIGS[name]
    cam, dirs, om = TC.rays(layout)
    rt = RayTracing(*TC.tracer_args(case))
    rt.train(mode == "train")
    rt.steps_override = TC.steps(case.n_steps)
    evals = []
    fn = TC.SDFS[sdf_name]

    def sdf(p):
        evals.append(int(p.shape[0]))
        return fn(p)

    with torch.no_grad():
        pts, mask, dists = rt(sdf=sdf, cam_loc=cam, object_mask=om.reshape(-1), ray_directions=dirs)
    return (pts, mask, dists), sum(evals)


@pytest.mark.parametrize("layout", list(TC.LAYOUTS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sdf_name", list(TC.SDFS))
@pytest.mark.parametrize("name", list(TC.CONFIGS))
def test_generic_tracer_equals_oracle(name, sdf_name, mode, layout):
    (p_ref, m_ref, t_ref), log = oracle_run(name, mode, layout, sdf_name)
    (p, m, t), evals = generic_run(name, mode, layout, sdf_name)
    assert p.shape == p_ref.shape and m.shape == m_ref.shape and t.shape == t_ref.shape
    assert torch.equal(m, m_ref), f"{int((m != m_ref).sum())} mask mismatches"
    assert torch.equal(t, t_ref), (t - t_ref).abs().max()
    assert torch.equal(p, p_ref), (p - p_ref).abs().max()
    assert evals == log["evals"]


# ---- every configuration reaches its branch (oracle side only) ------------------------------------------------------
BIG = ("1x300", "3x77")          # the one-ray layout is an edge case of its own, not a carrier of branches


def _log(name, mode, layout, sdf_name):
    return oracle_run(name, mode, layout, sdf_name)[1]


@pytest.mark.parametrize("layout", BIG)
@pytest.mark.parametrize("name", list(TC.CONFIGS))
def test_case_runs_sampler_secant_and_closest_approach(name, layout):
    """on the bumpy sphere every stage of the search has rays, but for the cases whose point is that one has none"""
    lg = _log(name, "train", layout, "bumpy")
    ev = _log(name, "eval", layout, "bumpy")
    assert lg["net"] > 0 and lg["rays"] - lg["net"] > 0
    if name == "thr1e-2":        # rays stop 1e-2 in front of the surface: (almost) none is left for the sampler
        assert lg["sampler"] < _log("bench", "train", layout, "bumpy")["sampler"] // 4
        assert lg["closest"] > 0
        return
    assert lg["sampler"] > 0 and ev["sampler"] > 0
    if name == "n2":             # two samples are the ends of the interval, both outside the surface: nothing to refine
        assert lg["secant"] == 0 and ev["secant"] == 0
    else:
        assert lg["secant"] > 0 and ev["secant"] >= lg["secant"]      # (eval refines outside the object mask too)
    if name == "st0":            # every ray that meets the sphere is a sampler ray, none is left for the mask loss
        assert lg["closest"] == 0
    else:
        assert lg["closest"] > 0
    assert ev["closest"] == 0


@pytest.mark.parametrize("layout", BIG)
@pytest.mark.parametrize("mode", MODES)
def test_line_search_cases_run_line_searches(mode, layout):
    """the overshooting SDF steps through the surface: 0, 1 and 3 line-search iterations are three different searches"""
    ev = [_log(n, mode, layout, "overshoot")["evals"] for n in ("ls0", "default", "bench")]
    assert len(set(ev)) == 3, ev
    calls = [len(_log(n, mode, layout, "overshoot")["calls"]) for n in ("ls0", "default", "bench")]
    assert calls[0] < calls[1] < calls[2], calls
    # and the pull-back factor matters: other line_search_steps, other searches
    for n in ("step03", "step09"):
        assert _log(n, mode, layout, "overshoot")["evals"] != ev[2]


@pytest.mark.parametrize("sdf_name", list(TC.SDFS))
@pytest.mark.parametrize("layout", BIG)
@pytest.mark.parametrize("mode", MODES)
def test_sphere_tracing_iters_cases(mode, layout, sdf_name):
    st0, st1, bench, st15 = (_log(n, mode, layout, sdf_name) for n in ("st0", "st1", "bench", "st15"))
    # no iteration: the march is the evaluation of both sphere intersections, then every sphere-hitting ray is sampled
    assert st0["sampler"] == st0["hit"] > 0
    assert st0["calls"][:2] == [st0["hit"], st0["hit"]] and st0["calls"][2] == min(st0["hit"] * 100, 10000)
    assert st0["sampler"] > st1["sampler"] > bench["sampler"] > st15["sampler"]
    assert len(st15["calls"]) > len(bench["calls"])          # rays were still marching after iteration 10


@pytest.mark.parametrize("layout", BIG)
@pytest.mark.parametrize("mode", MODES)
def test_secant_step_cases(mode, layout):
    s0, s1, s8, s64 = (_log(n, mode, layout, "bumpy") for n in ("sec0", "sec1", "bench", "sec64"))
    assert s0["secant"] == s1["secant"] == s8["secant"] == s64["secant"] > 0
    for k, lg in ((1, s1), (8, s8), (64, s64)):
        assert lg["evals"] == s0["evals"] + k * s0["secant"]


@pytest.mark.parametrize("layout", BIG)
def test_n_steps_cases(layout):
    for name in ("n2", "n3", "n7", "n17", "n18", "n64", "n99", "n130"):
        lg, n = _log(name, "train", layout, "bumpy"), TC.CONFIGS[name].n_steps
        # the coarse scans are n_steps samples per sampler ray and per mask-loss ray
        assert n * lg["sampler"] in lg["calls"] or n * lg["sampler"] > 10000
        assert n * lg["closest"] in lg["calls"] or n * lg["closest"] > 10000
        assert lg["sampler"] > 0 and lg["closest"] > 0


@pytest.mark.parametrize("layout", BIG)
def test_radius_and_threshold_cases(layout):
    bench, r08, r15 = (_log(n, "train", layout, "bumpy") for n in ("bench", "r08", "r15"))
    assert 0 < r08["hit"] < r08["rays"] == bench["hit"] == r15["hit"]       # rays that miss the smaller sphere
    assert r15["evals"] != bench["evals"]
    thr0 = _log("thr0", "train", layout, "bumpy")
    assert thr0["sampler"] > bench["sampler"]                                # fewer rays converge by the threshold


def test_filter_bank_layouts_stay_within_the_small_embedder_launch():
    """no launch of either tracer holds more than rays * max(n_steps, 2) points: with these layouts every launch of every
    configuration runs the embedder's lanes-per-point kernel (test_raytrace_nffb_gpu.py, all-VALU regime)"""
    assert set(TC.NFFB_LAYOUTS) == {"1x1", "3x21", "1x63"}
    for layout, (B, P) in TC.NFFB_LAYOUTS.items():
        cam, dirs, om = TC.nffb_rays(layout)
        assert cam.shape == (B, 3) and dirs.shape == (B, P, 3) and om.shape == (B, P)
        for name, case in TC.CONFIGS.items():
            assert B * P * max(case.n_steps, 2) <= TC.NFFB_SMALL_LAUNCH, (layout, name)
    assert 63 * TC.CONFIGS["n130"].n_steps == 8190      # the largest: two points below the kernel switch
    assert TC.LAYOUTS == {"1x300": (1, 300), "3x77": (3, 77), "1x1": (1, 1)}     # the hash-grid tests' own set


def test_layouts_and_table():
    cam, dirs, om = TC.rays("3x77")
    assert cam.shape == (3, 3) and dirs.shape == (3, 77, 3) and om.shape == (3, 77)
    assert not torch.equal(cam[0], cam[1]) and not torch.equal(cam[1], cam[2])
    assert 77 % 8 != 0                   # a workgroup of the persistent march tail (8 rays) carries rays of two cameras
    assert TC.rays("1x1")[1].shape == (1, 1, 3)
    c = TC.CONFIGS
    assert TC.tracer_args(c["bench"]) == (1.0, 5.0e-5, 0.5, 3, 10, 100, 8)
    assert TC.tracer_args(c["default"]) == (1.0, 5.0e-5, 0.5, 1, 10, 100, 8)
    assert {v.n_steps for v in c.values()} >= {2, 3, 7, 17, 18, 64, 99, 100, 130}
    assert {v.n_secant_steps for v in c.values()} >= {0, 1, 8, 64}
    assert {v.sphere_tracing_iters for v in c.values()} >= {0, 1, 10, 15} and c["st15"].line_step_iters == 3
    assert {v.line_step_iters for v in c.values()} >= {0, 1, 3}
    assert {v.line_search_step for v in c.values()} >= {0.3, 0.5, 0.9}
    assert {v.radius for v in c.values()} >= {0.8, 1.0, 1.5}
    assert {v.threshold for v in c.values()} >= {0.0, 5.0e-5, 1.0e-2}
    assert all(v.branch for v in c.values())
