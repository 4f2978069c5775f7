"""hm_diag_gemm_plan: the route of every case of tests/test_gemm_paths_gpu.py, and that together they launch every
kernel instance hm_gemm_f32 / _ep / _det can launch.  Host only - the plan reads no memory, so addresses with the
cases' alignments stand in for device pointers."""
import pytest

import gemm_cases as GC


@pytest.fixture(scope="module")
def lib():
    from hashmodnffbanks_idr_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


@pytest.mark.parametrize("case", GC.ALL, ids=lambda c: c.name)
def test_case_takes_its_route(lib, case):
    GC.check_route(case, GC.plan(case, GC.fake_ptr(case, "A"), GC.fake_ptr(case, "B")))


def test_cases_reach_every_instantiation(lib):
    got = {GC.check_route(c, GC.plan(c, GC.fake_ptr(c, "A"), GC.fake_ptr(c, "B"))) for c in GC.ALL}
    want = GC.all_instantiations()
    assert want - got == set(), f"kernel instances no GEMM case launches: {sorted(want - got)}"
    assert got - want == set(), f"unexpected instances: {sorted(got - want)}"


def test_plan_edges(lib):
    from hashmodnffbanks_idr_amd import _lib
    import ctypes
    info = _lib.GemmPlanInfo()
    for M, N in ((0, 5), (5, 0), (0, 0)):            # nothing to compute: no kernel
        assert lib.hm_diag_gemm_plan(0, 0, M, N, 7, None, 7, None, 5, 0, 0, ctypes.byref(info)) == 0
        assert (info.kernel, info.split) == (0, 0)
    with pytest.raises(ValueError):
        _lib.check(lib.hm_diag_gemm_plan(0, 0, -1, 5, 7, None, 7, None, 5, 0, 0, ctypes.byref(info)))
    # an epilogue never splits K; the deterministic flag only matters where K is split
    c = GC._case("x", 0, 0, 256, 256, 2048, GC.PIPE64, split=True)
    assert GC.plan(c, 0, 0).split > 1 and not GC.plan(c, 0, 0).part
    assert GC.plan(c._replace(det=True), 0, 0).part
    assert GC.plan(c._replace(ep="relu"), 0, 0).split == 1
    # alignment alone decides the generic kernel's vector loads
    c = GC._case("y", 0, 1, 300, 200, 100, GC.GENERIC)
    assert (GC.plan(c, 0x1000, 0x1000).vec_a, GC.plan(c, 0x1000, 0x1000).vec_b) == (1, 1)
    assert (GC.plan(c, 0x1004, 0x1008).vec_a, GC.plan(c, 0x1004, 0x1008).vec_b) == (0, 0)
