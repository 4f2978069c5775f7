"""The device DTU evaluation against its numpy restatements (tests/dtu_cases.py): the greedy radius thinning and the
point flags bit for bit, the whole pipeline against the reference's with cKDTree distances."""
import numpy as np
import pytest
import torch

import dtu_cases as DC
import nn_cases as NC
from hashmodnffbanks_idr_amd import ops
from hashmodnffbanks_idr_amd._lib import HashmodError
from hashmodnffbanks_idr_amd.evaluation import dtu_chamfer, mesh_chamfer

pytestmark = pytest.mark.gpu

BELOW_5 = float(np.nextafter(np.float32(5), np.float32(0)))
BELOW_1 = float(np.nextafter(np.float32(1), np.float32(0)))


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # a copy: the shared inputs are read-only


def _thin(points, radius, cell=None, stats=None):
    keep = ops.radius_downsample(_dev(NC._f4(points)), radius, cell=cell, stats=stats)
    assert keep.dtype == torch.bool and keep.shape == (len(points),)
    return keep.cpu().numpy()


def _check_thin(points, radius, want, cell=None):
    stats = {}
    got = _thin(points, radius, cell, stats)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} of {len(want)} differ from the sequential loop, first at {bad[:5]}"
    assert 1 <= stats["rounds"] <= len(points)
    return stats["rounds"]


# ---- sizes and ties --------------------------------------------------------------------------------------------
def test_single_and_identical_points():
    assert _thin(np.ones((1, 3)), 0.5).tolist() == [True]
    assert _thin(np.ones((2, 3)), 0.5).tolist() == [True, False]
    keep = _thin(np.tile([[0.25, -1.5, 3.0]], (300, 1)), 1e-3)
    assert keep[0] and not keep[1:].any()
    assert ops.radius_downsample(torch.zeros((0, 3), device="cuda"), 1.0).shape == (0,)


@pytest.mark.parametrize("n", [63, 64, 65])
def test_wave_edges(n):
    p = NC.cloud("uniform_%d_%d" % (n, {63: 64, 64: 65, 65: 63}[n]))[0]
    want = DC.downsample_ref(p, 0.3)
    assert 0 < want.sum() < n
    _check_thin(p, 0.3, want)


def test_equality_counts():
    pair = np.array([[0, 0, 0], [3, 4, 0]], np.float32)              # d2 == 25 exactly
    assert _thin(pair, 5.0).tolist() == [True, False]
    assert _thin(pair, BELOW_5).tolist() == [True, True]
    assert _thin(pair[::-1], 5.0).tolist() == [True, False]


@pytest.mark.parametrize("cell", [1, None, 0.25, 100.0])
def test_lattice_on_cell_faces(cell):
    p = NC.lattice()                                                 # every neighbour at d2 == radius2, on a cell face
    want = DC.reference("lattice", 1.0)
    assert want.sum() == 256
    _check_thin(p, 1.0, want, cell)
    assert _thin(p, BELOW_1, cell).all()


@pytest.mark.parametrize("which", range(3), ids=["default", "one_cell", "fine"])
def test_uniform_cloud_on_three_grids(which):
    p = NC.cloud("uniform_4097_1000")[0]
    radius = 0.0835                                                  # about 10 neighbours per point
    want = DC.reference("uniform_4097_1000", radius)
    assert 0 < want.sum() < len(p)
    _check_thin(p, radius, want, NC.cells(p)[which])


def test_clusters():
    p = NC.cloud("clusters")[0]
    want = DC.reference("clusters", 0.228)
    assert 0 < want.sum() < len(p)
    _check_thin(p, 0.228, want)


# ---- order and chains ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["default", "third", "one_cell"])
@pytest.mark.parametrize("radius", [0.02, 0.05])
def test_shuffled_sphere(radius, cell):
    p = DC.sphere("shuffled")
    rounds = _check_thin(p, radius, DC.reference("sphere_shuffled", radius),
                         {"default": None, "third": radius / 3, "one_cell": 8.0}[cell])
    print("rounds:", rounds)


def test_swept_sphere_has_long_chains():
    p = DC.sphere("swept")
    rounds = _check_thin(p, 0.05, DC.reference("sphere_swept", 0.05))
    print("rounds:", rounds)


@pytest.mark.parametrize("name", ["line", "line_reversed"])
def test_line_chain_as_long_as_the_input(name):
    p = DC.line() if name == "line" else DC.line()[::-1]
    want = DC.reference(name, 1.0)
    assert want.sum() == 513
    rounds = _check_thin(p, 1.0, want)
    print("rounds:", rounds)


def test_long_chain_through_the_batched_rounds():
    # 4097 points: the list is longer than the one-workgroup tail, so the chain starts in the batched launches
    p = DC.line(4097)
    _check_thin(p, 1.0, np.arange(4097) % 2 == 0)


def test_block_counts_span_two_scan_chunks():
    # 87 553 groups of three points = 262 659 points = 1027 blocks of 256: the scan of the blocks' counts takes two
    # chunks of 1024, the second partial, and carries the first one's total.  Group g has its points m = 0, 1, 2 at
    # ((g % 512)*4 + 0.5*m, (g // 512)*4, 0), index 3g + m: every coordinate and squared distance is exact in fp32,
    # 0.5 is inside the radius 0.75, 1.0 and the 2.0 or more between groups are outside.  Point 0 has no lower
    # neighbour, point 1 sees the kept point 0, point 2 sees only the removed point 1: the mask is m != 1.
    groups = 87553
    g, m = np.divmod(np.arange(3 * groups), 3)
    p = np.stack([(g % 512) * 4 + 0.5 * m, (g // 512) * 4, np.zeros(len(g))], 1).astype(np.float32)
    assert len(p) == 262659 and -(-len(p) // 256) == 1027
    want = m != 1
    assert np.array_equal(DC.downsample_ref(p[:900], 0.75), want[:900])
    _check_thin(p, 0.75, want)


def test_two_calls_agree_and_nan_raises():
    p = _dev(DC.sphere("shuffled"))
    a, b = ops.radius_downsample(p, 0.05), ops.radius_downsample(p, 0.05)
    assert torch.equal(a, b)
    for bad in (float("nan"), float("inf")):
        q = p.clone()
        q[1234, 1] = bad
        with pytest.raises(HashmodError, match="non-finite"):
            ops.radius_downsample(q, 0.05)
    with pytest.raises(HashmodError, match="CPU"):
        ops.radius_downsample(p.cpu(), 0.05)


# ---- flags ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("name", sorted(DC.FLAG_CASES))
def test_point_flags(name, n):
    shape, bb, res, patch, plane = DC.FLAG_CASES[name]
    mask = DC.flag_volume(name)
    pts = DC.flag_points(name, n)
    want = DC.flags_ref(pts, mask, bb, res, patch, plane)
    got = ops.dtu_point_flags(_dev(pts), _dev(mask), bb, res, patch, plane)
    assert got.dtype == torch.uint8 and got.shape == (n,)
    assert np.array_equal(got.cpu().numpy(), want), np.nonzero(got.cpu().numpy() != want)[0][:10]
    if n >= 255:
        edge = DC.flag_boundary_points(name)
        assert np.array_equal(pts[:len(edge)], edge, equal_nan=True) and np.all(want[len(edge) - 3:len(edge)] == 0)


def test_point_flags_empty_and_errors():
    shape, bb, res, patch, plane = DC.FLAG_CASES["4x4x4"]
    mask = _dev(DC.flag_volume("4x4x4"))
    assert ops.dtu_point_flags(torch.zeros((0, 3), device="cuda"), mask, bb, res, patch, plane).shape == (0,)
    with pytest.raises(ValueError, match="devices"):
        ops.dtu_point_flags(torch.zeros((4, 3), device="cuda"), mask.cpu(), bb, res, patch, plane)
    with pytest.raises(HashmodError, match="CPU"):
        ops.dtu_point_flags(torch.zeros((4, 3)), mask.cpu(), bb, res, patch, plane)


# ---- end to end -------------------------------------------------------------------------------------------------
def _close(a, b):
    return abs(a - b) <= 1e-6 * abs(b)           # the fp32-d2 bound of test_chamfer_gpu.py carried through a mean


COUNTS = ("n_cloud", "n_down", "n_in", "n_in_obs", "n_stl_above", "n_d2s", "n_s2d")


def test_dtu_chamfer_against_the_reference_pipeline():
    c, want = DC.dtu_case(), DC.dtu_case_reference()
    for d in (want["d2s"], want["s2d"]):
        assert np.abs(d / c["max_dist"] - 1).min() > 1e-6             # no distance hinges on rounding at the cut-off
    assert 0 < want["n_down"] < want["n_cloud"] and 0 < want["n_in"] < want["n_down"]
    assert 0 < want["n_in_obs"] < want["n_in"] and 0 < want["n_stl_above"] < len(c["stl"])
    assert 0 < want["n_d2s"] < want["n_in_obs"] and 0 < want["n_s2d"] < want["n_stl_above"]

    def run():
        return dtu_chamfer((_dev(c["verts"]), _dev(c["faces"])), _dev(c["stl"]), obs_mask=_dev(c["mask"]), bb=c["bb"],
                           res=c["res"], plane=c["plane"], density=c["density"], patch=c["patch"],
                           max_dist=c["max_dist"], order=_dev(c["order"]))

    r = run()
    print("dtu_chamfer", r, "reference", {k: want[k] for k in ("accuracy", "completeness", "overall") + COUNTS})
    assert {k: getattr(r, k) for k in COUNTS} == {k: want[k] for k in COUNTS}
    assert _close(r.accuracy, want["accuracy"]) and _close(r.completeness, want["completeness"])
    assert _close(r.overall, want["overall"]) and r.overall == 0.5 * (r.accuracy + r.completeness)
    assert tuple(run()) == tuple(r)

    # the seeded device shuffle: another order, the same protocol; two calls agree
    def shuffled(seed):
        return dtu_chamfer((_dev(c["verts"]), _dev(c["faces"])), _dev(c["stl"]), obs_mask=_dev(c["mask"]), bb=c["bb"],
                           res=c["res"], plane=c["plane"], density=c["density"], patch=c["patch"],
                           max_dist=c["max_dist"], shuffle_seed=seed)

    s = shuffled(1)
    assert tuple(shuffled(1)) == tuple(s) and s.n_cloud == r.n_cloud and 0 < s.n_down < s.n_cloud
    assert abs(s.overall - r.overall) < 0.05 * r.overall


def test_one_sided_distance_is_chamfer_distance_one_way():
    p, q = (_dev(a) for a in NC.cloud("uniform_4097_1000"))
    for max_dist in (None, 0.05):
        r = ops.chamfer_distance(q, p, max_dist)
        assert ops.one_sided_distance(q, p, max_dist) == (r.mean_a2b, r.n_a2b)
        assert ops.one_sided_distance(p, q, max_dist) == (r.mean_b2a, r.n_b2a)
    mean, count = ops.one_sided_distance(q, p + 50.0, 0.05)
    assert np.isnan(mean) and count == 0
    assert ops.one_sided_distance(q[:0], p)[1] == 0 and ops.one_sided_distance(q, p[:0])[1] == 0


def _chamfer_distance_before(a, b, max_dist):
    """ops.chamfer_distance's body as it was before one_sided_distance was split off, on the same helpers"""
    import math
    md2 = math.inf if max_dist is None else float(np.nextafter(np.float32(min(float(max_dist) ** 2 * (1.0 + 1e-6),
                                                                             3.0e38)), np.float32(np.inf)))
    sa, ca, sb, cb = torch.cat([ops._one_sided(a, ops.NNIndex(b), max_dist, md2),
                                ops._one_sided(b, ops.NNIndex(a), max_dist, md2)]).tolist()
    return ops.ChamferResult(sa / ca if ca else math.nan, sb / cb if cb else math.nan, int(ca), int(cb))


def test_chamfer_results_are_unchanged():
    """mesh_chamfer and chamfer_distance on the inputs of test_chamfer_against_fp64_reference return what the code
    before the change returns, bit for bit"""
    vol, spacing = NC.sphere_volume()
    verts, faces, _ = ops.marching_cubes(_dev(vol), 0.0, spacing)
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    density = 0.02
    cloud = _dev(np.concatenate([v, NC.sample_ref(v, f, density)[0]]))
    target = _dev(NC.perturbed_target(v, 20000, 0.02))
    for max_dist in (0.03, None):
        before = _chamfer_distance_before(cloud, target, max_dist)
        assert before.n_a2b > 0 and before.n_b2a > 0
        assert tuple(ops.chamfer_distance(cloud, target, max_dist)) == tuple(before)
        m = mesh_chamfer((verts, faces), target, density, max_dist)
        assert tuple(m) == tuple(before)[:5] + (cloud.shape[0],)
