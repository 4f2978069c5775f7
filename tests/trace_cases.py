"""Shared inputs of the ray tracer's configuration tests (torch / numpy only): the table of RayTracing constructor
settings, the ray layouts, object masks and injected closest-approach fractions, and the analytic SDFs of the CPU test.

  CONFIGS            name -> (TraceCase: the seven constructor arguments + the branch the entry exists for)
  LAYOUTS            name -> (cameras, rays per camera)
  rays(layout)       (cam_loc [B,3], ray_dirs [B,P,3], object_mask [B,P]) as torch CPU tensors
  NFFB_LAYOUTS       the same for the filter-bank tests, with nffb_rays(layout)
  steps(n_steps)     the injected U(0,1) fractions of the closest-approach search
  SDFS               name -> analytic elementwise fp32 SDF (CPU test only)

Everything is computed once per process and must be treated as read-only."""
import collections
import functools

import numpy as np
import torch

import params as P

TraceCase = collections.namedtuple(
    "TraceCase", "radius threshold line_search_step line_step_iters sphere_tracing_iters n_steps n_secant_steps branch")


def _case(branch, radius=1.0, threshold=5.0e-5, step=0.5, ls=3, st=10, n=100, sec=8):
    return TraceCase(radius, threshold, step, ls, st, n, sec, branch)


# every entry differs from the bench setting in ONE argument (st15 keeps line_step_iters 3: 61 march rounds)
CONFIGS = {
    "bench": _case("the benchmarked and so far only tested setting"),
    "default": _case("class default: line_step_iters 1", ls=1),
    "ls0": _case("no line search: no persistent tail, back[] unused", ls=0),
    "st0": _case("no march iteration: every sphere-hitting ray goes to the sampler, tail called with first == rounds", st=0),
    "st1": _case("one march iteration", st=1),
    "st15": _case("61 march rounds: next to the 64-entry counter array and the r + 1 < 64 clamp", st=15),
    "n2": _case("max(n_steps, 2) workspace sizing; the samples are the interval's ends: sampler without secant rays", n=2),
    "n3": _case("smallest n_steps with an inner sample; scalar reduce loops", n=3),
    "n7": _case("scalar reduce loops; scans below the 64-point kernel's range", n=7),
    "n17": _case("head 16 == n_steps - 1: the lazy sampler must switch itself off", n=17),
    "n18": _case("head 16 == n_steps - 2: smallest second pass, one sample per ray; scalar loops", n=18),
    "n64": _case("float4 reduce path at another row length", n=64),
    "n99": _case("odd n_steps: scalar reduce loops, unaligned rows", n=99),
    "n130": _case("n_steps above 128, not a multiple of 4", n=130),
    "sec0": _case("initial secant estimate is the answer: no secant launch, no one-launch scan", sec=0),
    "sec1": _case("one secant iteration: the first is also the last", sec=1),
    "sec64": _case("upper end of n_secant_steps", sec=64),
    "step03": _case("back[k] not a power of two: t - back * cur rounds", step=0.3),
    "step09": _case("back[k] not a power of two, small pull-back", step=0.9),
    "r08": _case("smaller bounding sphere: other hit set, shorter search interval", radius=0.8),
    "r15": _case("larger bounding sphere: search starts outside the unit cube", radius=1.5),
    "thr0": _case("threshold 0: a ray converges only on a non-positive value", threshold=0.0),
    "thr1e-2": _case("large threshold: rays stop far from the surface", threshold=1.0e-2),
}

LAYOUTS = {"1x300": (1, 300), "3x77": (3, 77), "1x1": (1, 1)}
_LAYOUT_SEED = {"1x300": 100, "3x77": 200, "1x1": 300}

# Filter-bank networks (tests/test_raytrace_nffb_gpu.py): the fused embedder picks its kernel by the live count of a launch
# (<= 8192 points: the lanes-per-point kernel), so these layouts keep rays * max(n_steps, 2) - the tracer's largest launch
# - within 8192 for every entry of CONFIGS (n130: 63 * 130 = 8190; asserted in test_raytrace_configs_cpu.py).  A table of
# its own: the hash-grid tests keep their parameter sets.
NFFB_LAYOUTS = {"1x1": (1, 1), "3x21": (3, 21), "1x63": (1, 63)}
_NFFB_LAYOUT_SEED = {"1x1": 400, "3x21": 500, "1x63": 600}
NFFB_SMALL_LAUNCH = 8192


def tracer_args(case):
    return tuple(case[:7])


def make_rays(cameras, per_camera, seed):
    """`cameras` cameras (params.make_rays with seeds seed, seed + 1, ..) and the uniform < 0.6 object mask"""
    cams, dirs = zip(*(P.make_rays(seed + b, per_camera) for b in range(cameras)))
    om = np.random.RandomState(seed).uniform(0, 1, (cameras, per_camera)) < 0.6
    return (torch.from_numpy(np.concatenate(cams, 0)), torch.from_numpy(np.concatenate(dirs, 0)), torch.from_numpy(om))


@functools.lru_cache(maxsize=None)
def rays(layout):
    B, n = LAYOUTS[layout]
    return make_rays(B, n, _LAYOUT_SEED[layout])


@functools.lru_cache(maxsize=None)
def nffb_rays(layout):
    B, n = NFFB_LAYOUTS[layout]
    return make_rays(B, n, _NFFB_LAYOUT_SEED[layout])


@functools.lru_cache(maxsize=None)
def steps(n_steps, seed=7):
    return torch.from_numpy(np.random.RandomState(seed).uniform(0, 1, n_steps).astype(np.float32))


# ---- analytic SDFs -------------------------------------------------------------------------------------------------
# Only +, -, *, floor and sqrt on fp32 columns: each is correctly rounded in torch's vector and scalar CPU loops alike,
# so a point's value does not depend on the batch (or the position in it) it was evaluated in.
def _hump(x, freq):
    u = x * freq
    u = u - torch.floor(u)
    return 4.0 * u * (1.0 - u)          # 0 at the cell borders, 1 in the middle


def sdf_bumpy(p):
    """a sphere of radius ~0.55 with a lattice of dents; Lipschitz constant a little above 1"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r = torch.sqrt(x * x + y * y + z * z)
    return r - 0.55 + 0.03 * _hump(x, 3.0) * _hump(y, 3.0) * _hump(z, 3.0)


def sdf_overshoot(p):
    """the same surface, values scaled by 1.8: marching overshoots and the line searches run"""
    return 1.8 * sdf_bumpy(p)


SDFS = {"bumpy": sdf_bumpy, "overshoot": sdf_overshoot}
