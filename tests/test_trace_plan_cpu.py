"""hm_diag_trace_plan: the launch sequence the ray search enqueues for a configuration (csrc/hm_trace.hip: trace_plan),
asked on the host.  A literal decision table - the expected plans are written out from the rules of the tracer as they
stood before the plan existed, not computed by a copy of them: which of the five sequences runs, whether the
closest-approach rows get a launch of their own, how the secant chain is cut, when the march hands over to its persistent
kernel and which form the secant refinement takes, under every environment switch the GPU tests flip."""
import ctypes

import pytest

JOINT, FILL, SERIAL, COSCHED, POOLED = range(5)                    # include/hashmod.h: HM_TRACE_SEQ_*
SEC_NONE, SEC_IN_SEQ, SEC_PERSISTENT, SEC_PER_ITER = range(4)       # HM_TRACE_SECANT_*
C_NSAMP_PTS, C_HEAD_PTS, C_GUARD_N2 = 65, 75, 81                    # csrc/hm_trace_dev.h: counters
SMALL = 8192                                                        # csrc/hm_common.h: kSdfSmall
TAU = 2.0 ** -16                                                    # csrc/hm_trace_dev.h: kGuardTau

SWITCHES = ("HM_TRACE_OVERLAP", "HM_TRACE_POOL_CHAIN_TILES", "HM_TRACE_CHAIN_TAIL", "HM_TRACE_TAIL_FIRST",
            "HM_TRACE_GUARD_NOISE")

# The base: training, hash grid, tile size left to the library, 2048 rays of 100 samples, 8 secant steps, 10 sphere-tracing
# iterations of up to 3 line-search steps - the bench step's ray tracer.
BASE = dict(n_rays=2048, tile_points=0, nffb=0, training=1, n_steps=100, n_secant_steps=8, sphere_tracing_iters=10,
            line_step_iters=3, coarse_bf16=0, sampler_head=0)
# ... and its plan in the exact mode: 41 march rounds of which 11 are launches of their own, one sampler pass
BASE_PLAN = dict(sequence=FILL, sel_own=1, head=0, per_ray=100, c_first=C_NSAMP_PTS, k_tail=0, c_ref2=-1, march_tail=1,
                 march_launched=11, march_rounds=41, secant=SEC_IN_SEQ, scan_rule=0, noise_nan=0, noise_amp=0.0,
                 chain_tiles=0, guard_min=SMALL + 1)
# ... and in the guarded mode: pooled, the chain's last two rounds behind the cut, 7 tiles per workgroup under the chain
GUARD = dict(coarse_bf16=3)
GUARD_PLAN = dict(sequence=POOLED, k_tail=2, chain_tiles=7)
# the guarded sequence with every launch on its own, where the shape rules the others out
SERIAL_PLAN = dict(sequence=SERIAL, sel_own=0, secant=SEC_PERSISTENT)

# (name, what differs from BASE, environment, what differs from BASE_PLAN)
TABLE = [
    ("exact", {}, {}, {}),
    ("exact_overlap0", {}, {"HM_TRACE_OVERLAP": "0"}, dict(sequence=JOINT, sel_own=0, secant=SEC_PERSISTENT)),
    ("exact_overlap1", {}, {"HM_TRACE_OVERLAP": "1"}, {}),
    ("exact_head16", dict(sampler_head=16), {}, dict(head=16, per_ray=17, c_first=C_HEAD_PTS)),
    ("guard", GUARD, {}, GUARD_PLAN),
    ("guard_head16", dict(GUARD, sampler_head=16), {},
     dict(GUARD_PLAN, head=16, per_ray=17, c_first=C_HEAD_PTS, c_ref2=C_GUARD_N2)),
    ("guard_head_out_of_range", dict(GUARD, sampler_head=99), {}, GUARD_PLAN),
    ("guard_overlap0", GUARD, {"HM_TRACE_OVERLAP": "0"}, SERIAL_PLAN),
    ("guard_overlap1", GUARD, {"HM_TRACE_OVERLAP": "1"}, dict(sequence=SERIAL, sel_own=1, secant=SEC_PERSISTENT, scan_rule=1)),
    ("guard_overlap1_head16", dict(GUARD, sampler_head=16), {"HM_TRACE_OVERLAP": "1"},
     dict(sequence=SERIAL, sel_own=1, secant=SEC_PERSISTENT, scan_rule=1, head=16, per_ray=17, c_first=C_HEAD_PTS)),
    ("guard_overlap2", GUARD, {"HM_TRACE_OVERLAP": "2"}, dict(sequence=COSCHED)),
    ("guard_overlap2_head16", dict(GUARD, sampler_head=16), {"HM_TRACE_OVERLAP": "2"},
     dict(sequence=COSCHED, head=16, per_ray=17, c_first=C_HEAD_PTS)),
    ("guard_secant1", dict(GUARD, n_secant_steps=1), {}, dict(sequence=POOLED, k_tail=0, chain_tiles=0)),
    ("guard_secant2", dict(GUARD, n_secant_steps=2), {}, dict(sequence=POOLED, k_tail=0, chain_tiles=1)),
    ("guard_secant3", dict(GUARD, n_secant_steps=3), {}, dict(sequence=POOLED, k_tail=2, chain_tiles=2)),
    ("guard_chain_tail0", GUARD, {"HM_TRACE_CHAIN_TAIL": "0"}, dict(GUARD_PLAN, k_tail=0)),
    ("guard_chain_tail3", GUARD, {"HM_TRACE_CHAIN_TAIL": "3"}, dict(GUARD_PLAN, k_tail=3)),
    ("guard_chain_tail7", GUARD, {"HM_TRACE_CHAIN_TAIL": "7"}, dict(GUARD_PLAN, k_tail=7)),
    ("guard_chain_tail8", GUARD, {"HM_TRACE_CHAIN_TAIL": "8"}, dict(GUARD_PLAN, k_tail=0)),
    ("guard_chain_tail_negative", GUARD, {"HM_TRACE_CHAIN_TAIL": "-1"}, GUARD_PLAN),
    ("guard_chain_tiles0", GUARD, {"HM_TRACE_POOL_CHAIN_TILES": "0"}, dict(GUARD_PLAN, chain_tiles=0)),
    ("guard_chain_tiles5", GUARD, {"HM_TRACE_POOL_CHAIN_TILES": "5"}, dict(GUARD_PLAN, chain_tiles=5)),
    ("guard_chain_tiles_overlap2", GUARD, {"HM_TRACE_POOL_CHAIN_TILES": "5", "HM_TRACE_OVERLAP": "2"}, dict(sequence=COSCHED)),
    ("guard_8192_rays", dict(GUARD, n_rays=SMALL), {}, GUARD_PLAN),
    ("guard_8193_rays", dict(GUARD, n_rays=SMALL + 1), {}, dict(SERIAL_PLAN, secant=SEC_PER_ITER)),
    ("guard_eval", dict(GUARD, training=0), {}, SERIAL_PLAN),
    ("guard_tile16", dict(GUARD, tile_points=16), {}, dict(SERIAL_PLAN, guard_min=1)),
    ("guard_tile64", dict(GUARD, tile_points=64), {},
     dict(SERIAL_PLAN, guard_min=1, secant=SEC_PER_ITER, march_tail=0, march_launched=41)),
    ("guard_secant0", dict(GUARD, n_secant_steps=0), {}, dict(SERIAL_PLAN, secant=SEC_NONE)),
    ("guard_noise", GUARD, {"HM_TRACE_GUARD_NOISE": "0.5"}, dict(GUARD_PLAN, noise_amp=0.5 * TAU)),
    ("guard_noise_nan", GUARD, {"HM_TRACE_GUARD_NOISE": "nan:7"}, dict(GUARD_PLAN, noise_nan=7)),
    ("guard_noise_out_of_range", GUARD, {"HM_TRACE_GUARD_NOISE": "1.5"}, GUARD_PLAN),
    ("exact_noise", {}, {"HM_TRACE_GUARD_NOISE": "0.5"}, {}),
    ("bf16", dict(coarse_bf16=1), {}, dict(sequence=JOINT, sel_own=0, secant=SEC_PERSISTENT)),
    ("split", dict(coarse_bf16=2), {}, dict(sequence=JOINT, sel_own=0, secant=SEC_PERSISTENT)),
    ("exact_8193_rays", dict(n_rays=SMALL + 1), {}, dict(sequence=JOINT, sel_own=0, secant=SEC_PER_ITER)),
    ("exact_eval", dict(training=0), {}, dict(sequence=JOINT, sel_own=0, secant=SEC_PERSISTENT)),
    ("exact_tile4", dict(tile_points=4), {},
     dict(sequence=JOINT, sel_own=0, secant=SEC_PERSISTENT, guard_min=1, march_tail=0, march_launched=41)),
    ("exact_tile16_8193_rays", dict(tile_points=16, n_rays=SMALL + 1), {},
     dict(sequence=JOINT, sel_own=0, secant=SEC_PERSISTENT, guard_min=1)),
    ("nffb", dict(nffb=1), {},
     dict(sequence=JOINT, sel_own=0, secant=SEC_PER_ITER, march_tail=0, march_launched=41)),
    ("nffb_bf16", dict(nffb=1, coarse_bf16=1), {},
     dict(sequence=JOINT, sel_own=0, secant=SEC_PER_ITER, march_tail=0, march_launched=41)),
    ("nffb_tail_first", dict(nffb=1), {"HM_TRACE_TAIL_FIRST": "1"},
     dict(sequence=JOINT, sel_own=0, secant=SEC_PER_ITER, march_tail=0, march_launched=41)),
    ("line_steps0", dict(line_step_iters=0), {}, dict(march_tail=0, march_launched=11, march_rounds=11)),
    ("line_steps1", dict(line_step_iters=1), {}, dict(march_rounds=21)),
    ("tail_first1", {}, {"HM_TRACE_TAIL_FIRST": "1"}, dict(march_launched=1)),
    ("tail_first10", GUARD, {"HM_TRACE_TAIL_FIRST": "10"}, dict(GUARD_PLAN, march_launched=10)),
    ("tail_first11", {}, {"HM_TRACE_TAIL_FIRST": "11"}, {}),
    ("tail_first0", {}, {"HM_TRACE_TAIL_FIRST": "0"}, {}),
]


@pytest.fixture(scope="module")
def L():
    from hashmodnffbanks_idr_amd import _lib, build
    build.build(verbose=False)
    return _lib


def plan_of(L, monkeypatch, cfg, env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    c = dict(BASE, **cfg)
    tc = L.TraceCfg(object_bounding_sphere=1.0, sdf_threshold=5.0e-5, line_search_step=0.5,
                    line_step_iters=c["line_step_iters"], sphere_tracing_iters=c["sphere_tracing_iters"],
                    n_steps=c["n_steps"], n_secant_steps=c["n_secant_steps"], training=c["training"],
                    coarse_bf16=c["coarse_bf16"], sampler_head=c["sampler_head"])
    info = L.TracePlanInfo()
    L.check(L.lib().hm_diag_trace_plan(c["n_rays"], ctypes.byref(tc), c["tile_points"], c["nffb"], ctypes.byref(info)))
    return {name: getattr(info, name) for name, _ in L.TracePlanInfo._fields_}


@pytest.mark.parametrize("name,cfg,env,want", TABLE, ids=[t[0] for t in TABLE])
def test_configuration_gets_its_plan(L, monkeypatch, name, cfg, env, want):
    assert plan_of(L, monkeypatch, cfg, env) == dict(BASE_PLAN, **want)


@pytest.mark.parametrize("head", [0, 16])
def test_bench_guarded_step_is_pooled_with_the_cut_chain(L, monkeypatch, head):
    """bench.py's guarded legs (2048 rays, the headline's single pass and the lazy sampler's head of 16): until the plan
    could be asked, only the device counters implied which sequence the measured step runs"""
    p = plan_of(L, monkeypatch, dict(GUARD, sampler_head=head), {})
    assert p["sequence"] == POOLED and p["k_tail"] == 2 and p["chain_tiles"] == 7 and p["sel_own"] == 1
    assert p["secant"] == SEC_IN_SEQ and (p["c_ref2"] == C_GUARD_N2) == (head > 0)


def test_switches_are_read_per_call(L, monkeypatch):
    assert plan_of(L, monkeypatch, GUARD, {"HM_TRACE_OVERLAP": "1"})["sequence"] == SERIAL
    assert plan_of(L, monkeypatch, GUARD, {})["sequence"] == POOLED


def test_plan_rejects_bad_arguments(L):
    tc = L.TraceCfg(n_steps=100)
    info = L.TracePlanInfo()
    with pytest.raises(ValueError, match="hm_diag_trace_plan"):
        L.check(L.lib().hm_diag_trace_plan(-1, ctypes.byref(tc), 0, 0, ctypes.byref(info)))
    with pytest.raises(ValueError, match="hm_diag_trace_plan"):
        L.check(L.lib().hm_diag_trace_plan(16, ctypes.byref(tc), 0, 0, None))
