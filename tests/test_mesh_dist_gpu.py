"""The device point-to-mesh distance (csrc/hm_mesh_dist.hip) against its numpy restatement
(tests/mesh_dist_cases.closest_ref): bit for bit over every grid and big-face setting, independent of batching and
order, the layout of the triangle grid, the errors, and the evaluation entry points built on it."""
import functools
import math

import numpy as np
import pytest
import torch

import mesh_dist_cases as MC
import nn_cases as NC
from hashmodnffbanks_idr_amd import ops
from hashmodnffbanks_idr_amd._lib import HashmodError
from hashmodnffbanks_idr_amd.evaluation import mesh_chamfer, mesh_to_mesh

pytestmark = pytest.mark.gpu

CELL_IDS = ["default", "one_cell", "fine"]


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # a copy: the shared inputs are read-only


def _big(big_face):
    return ops.MESH_DIST_BIG_FACE if big_face is None else big_face


def _check(got, want, what=""):
    """d2, face, point, feature torch.equal to the reference (a NaN point of a cut query compared as NaN)"""
    d2, face, point, feature = got
    assert d2.dtype == torch.float32 and face.dtype == torch.int32
    assert point.dtype == torch.float32 and feature.dtype == torch.int32
    assert torch.equal(face.cpu(), torch.from_numpy(want[1].copy())), f"face differs from the brute force {what}"
    assert torch.equal(d2.cpu(), torch.from_numpy(want[0].copy())), f"d2 differs from the brute force {what}"
    assert torch.equal(feature.cpu(), torch.from_numpy(want[3].copy())), f"feature differs {what}"
    cut = want[1] < 0
    got_p = point.cpu().numpy()
    assert np.isnan(got_p[cut]).all(), f"a cut query has a point {what}"
    assert torch.equal(torch.from_numpy(got_p[~cut]), torch.from_numpy(want[2][~cut])), f"point differs {what}"


def _closest(q, v, f, **kw):
    return ops.mesh_closest_point(_dev(q), _dev(v), _dev(f), return_feature=True, **kw)


# ---- G1: bit for bit against closest_ref --------------------------------------------------------------------
@pytest.mark.parametrize("which", range(3), ids=CELL_IDS)
@pytest.mark.parametrize("name", MC.CASES)
def test_closest_point_equals_brute_force(name, which):
    v, f, q = MC.case(name)
    cell = MC.cells(v)[which]
    for big_face in MC.BIG_FACES:
        _check(_closest(q, v, f, cell=cell, big_face=_big(big_face)), MC.reference(name),
               f"(cell {cell}, big_face {big_face})")


def test_outputs_are_optional_and_empty_queries_give_empty_outputs():
    v, f, q = MC.case("icosphere1")
    want = MC.reference("icosphere1")
    index = ops.mesh_index(_dev(v), _dev(f))
    out = index.query(_dev(q), return_point=False)
    assert len(out) == 2 and torch.equal(out[0].cpu(), torch.from_numpy(want[0].copy()))
    out = index.query(_dev(q), return_point=False, return_feature=True)
    assert len(out) == 3 and torch.equal(out[2].cpu(), torch.from_numpy(want[3].copy()))
    out = index.query(_dev(q))
    assert len(out) == 3 and torch.equal(out[2].cpu(), torch.from_numpy(want[2].copy()))
    d2, face, point, feature = index.query(torch.zeros((0, 3), device="cuda"), return_feature=True)
    assert d2.shape == (0,) and face.shape == (0,) and point.shape == (0, 3) and feature.shape == (0,)
    assert ops.point_mesh_distance(torch.zeros((0, 3), device="cuda"), index) == (pytest.approx(math.nan, nan_ok=True),
                                                                                0)


# ---- G2: independence ---------------------------------------------------------------------------------------
def test_result_does_not_depend_on_batching_or_order():
    v, f, q = MC.case("queries_1000")
    want = MC.reference("queries_1000")
    index = ops.mesh_index(_dev(v), _dev(f))
    qd = _dev(q)
    first = index.query(qd, return_feature=True)
    _check(first, want)
    again = index.query(qd, return_feature=True)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for k in (1, 63, 65):
        part = index.query(qd[:k].contiguous(), return_feature=True)
        assert all(torch.equal(a, b[:k]) for a, b in zip(part, first)), k
    perm = torch.from_numpy(np.random.default_rng(8).permutation(len(q))).cuda()
    shuffled = index.query(qd[perm].contiguous(), return_feature=True)
    assert all(torch.equal(a, b[perm]) for a, b in zip(shuffled, first))


@pytest.mark.parametrize("name", ["icosphere2", "big_among_small", "planar"])
def test_permuting_the_faces_maps_the_winner(name):
    v, f, q = MC.case(name)
    d2, face, _, _ = MC.reference(name)
    perm = np.random.default_rng(12).permutation(len(f))              # new face i is old face perm[i]
    got = _closest(q, v, f[perm])
    assert torch.equal(got[0].cpu(), torch.from_numpy(d2.copy()))
    unique = MC.n_minimisers(q, v, f) == 1
    assert unique.any()
    assert np.array_equal(perm[got[1].cpu().numpy()[unique]], face[unique])
    # and in general the winner is the lowest NEW index among the minimisers: the brute force over the permuted mesh
    _check(got, MC.closest_ref(q, v, f[perm]))


# ---- G3: max_dist -------------------------------------------------------------------------------------------
def test_max_dist_boundary_is_reported():
    v, f, q = MC.case("planar")
    at = [i for i, (_, d, _) in enumerate(MC.PLANAR_QUERIES) if d == 4.0][0]
    want = [w[at:at + 1] for w in MC.reference("planar")]
    assert want[0].tolist() == [4.0]                                  # distance exactly 2
    below = float(np.nextafter(np.float32(2.0), np.float32(0.0)))
    for cell in MC.cells(v):
        for big_face in MC.BIG_FACES:
            kw = dict(cell=cell, big_face=_big(big_face))
            _check(_closest(q[at:at + 1], v, f, max_dist=2.0, **kw), want)
            d2, face, point, feature = _closest(q[at:at + 1], v, f, max_dist=below, **kw)
            assert d2.tolist() == [math.inf] and face.tolist() == [-1] and feature.tolist() == [-1]
            assert torch.isnan(point).all()


@pytest.mark.parametrize("which", range(3), ids=CELL_IDS)
def test_max_dist_on_the_way_between_two_clusters(which):
    v, f, q = MC.case("clusters")
    md2 = float(np.float32(MC.CLUSTERS_MAX_DIST) ** 2)
    want = MC.reference("clusters", md2)
    assert 0 < (want[1] < 0).sum() < len(q)
    for big_face in MC.BIG_FACES:
        _check(_closest(q, v, f, max_dist=MC.CLUSTERS_MAX_DIST, cell=MC.cells(v)[which], big_face=_big(big_face)),
               want, f"(big_face {big_face})")


# ---- G4: the layout of the triangle grid --------------------------------------------------------------------
def _cell_np(p, lo, h, g):
    """nn_cell in numpy: clamp(floor((p - lo) / h), 0, g - 1) per axis, fp32, every operation rounded once"""
    t = np.floor((p.astype(np.float32) - np.asarray(lo, np.float32)) / np.float32(h))
    return np.minimum(np.clip(t, 0, 2.0 ** 30).astype(np.int64), np.asarray(g, np.int64) - 1)


@pytest.mark.parametrize("big_face", [None, 1, 8, 1 << 40])
@pytest.mark.parametrize("name,cell", [("big_among_small", None), ("big_among_small", 0.25), ("icosphere2", 0.3),
                                      ("planar", 1.0), ("soup_257", None)])
def test_index_layout(name, cell, big_face):
    v, f, _ = MC.case(name)
    big_face = _big(big_face)
    index = ops.mesh_index(_dev(v), _dev(f), cell=cell, big_face=big_face)
    g = index.g
    cs = index.cell_start.cpu().numpy()
    rec = index.records.cpu().numpy()
    n_pairs, n_big = index.n_pairs, index.n_big
    assert rec.shape == (n_pairs + n_big, 12) and len(cs) == g[0] * g[1] * g[2] + 1
    assert cs[0] == 0 and cs[-1] == n_pairs and np.all(np.diff(cs) >= 0)
    face_of = rec[:, 9].view(np.int32)
    assert np.array_equal(rec[:, :9], v[f[face_of]].reshape(-1, 9)) and (rec[:, 10:] == 0).all()
    # what the layout must be: every face in exactly the cells of its box, or in the big list
    tri = v[f]
    c0, c1 = _cell_np(tri.min(1), index.lo, index.h, g), _cell_np(tri.max(1), index.lo, index.h, g)
    n_cells = np.prod(c1 - c0 + 1, axis=1)
    is_big = n_cells > big_face
    assert np.array_equal(face_of[n_pairs:], np.nonzero(is_big)[0])                  # ascending
    assert n_pairs == n_cells[~is_big].sum()
    want = []
    for face in np.nonzero(~is_big)[0]:
        x, y, z = np.meshgrid(*(np.arange(c0[face, a], c1[face, a] + 1) for a in range(3)), indexing="ij")
        keys = ((x * g[1] + y) * g[2] + z).ravel()
        want.append(np.stack([keys, np.full(len(keys), face)], 1))
    want = np.concatenate(want) if want else np.zeros((0, 2), np.int64)
    want = want[np.lexsort((want[:, 1], want[:, 0]))]                                # by cell, ascending face inside
    got_key = np.repeat(np.arange(len(cs) - 1), np.diff(cs))
    assert np.array_equal(np.stack([got_key, face_of[:n_pairs]], 1), want)


# ---- G5: errors ---------------------------------------------------------------------------------------------
def test_bad_inputs_raise_and_leave_the_library_usable():
    v, f, q = MC.case("icosphere1")
    want = MC.reference("icosphere1")
    for bad in (np.nan, np.inf):
        vb = np.array(v)
        vb[int(f[7, 1]), 2] = bad
        with pytest.raises(HashmodError, match="non-finite"):
            ops.mesh_index(_dev(vb), _dev(f))
        with pytest.raises(HashmodError, match="non-finite"):
            ops.mesh_closest_point(_dev(q), _dev(vb), _dev(f))
    for bad in (-1, len(v)):
        fb = np.array(f)
        fb[11, 2] = bad
        with pytest.raises(HashmodError, match="face index"):
            ops.mesh_index(_dev(v), _dev(fb))
    qb = np.array(q)
    qb[5, 1] = np.nan
    index = ops.mesh_index(_dev(v), _dev(f))
    with pytest.raises(HashmodError, match="non-finite"):
        index.query(_dev(qb))
    with pytest.raises(HashmodError, match="non-finite"):
        ops.point_mesh_distance(_dev(qb), index)
    _check(index.query(_dev(q), return_feature=True), want)
    _check(_closest(q, v, f), want)


# ---- G6: evaluation -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sphere_target():
    v, f = NC.icosphere(3)
    return v, f, NC.perturbed_target(v, 1000, 0.01)


def test_mesh_chamfer_default_is_unchanged_and_surface_is_exact():
    v, f, target = _sphere_target()
    vd, fd, td = _dev(v), _dev(f), _dev(target)
    density = 0.05
    cloud = torch.cat([vd, ops.mesh_sample_surface(vd, fd, density)])
    for max_dist in (None, 0.02):
        today = ops.chamfer_distance(cloud, td, max_dist)
        sampled = mesh_chamfer((vd, fd), td, density, max_dist)
        assert tuple(sampled) == tuple(today)[:5] + (int(cloud.shape[0]),)
        assert tuple(mesh_chamfer((vd, fd), td, density, max_dist, surface=False)) == tuple(sampled)
        exact = mesh_chamfer((vd, fd), td, density, max_dist, surface=True)
        # accuracy is the same bits; the sampled cloud lies on the surface, so the exact distance cannot exceed it
        assert exact.mean_a2b == sampled.mean_a2b and exact.n_a2b == sampled.n_a2b and exact.n_cloud == sampled.n_cloud
        d2 = ops.mesh_closest_point(td, vd, fd, return_point=False)[0]
        d = np.sqrt(d2.cpu().numpy().astype(np.float64))
        keep = d < max_dist if max_dist is not None else np.ones(len(d), bool)
        assert exact.n_b2a == int(keep.sum()) >= sampled.n_b2a > 0
        if max_dist is None:
            print(f"completeness: sampled {sampled.mean_b2a:.6e}, exact {d.mean():.6e}")
            assert d.mean() <= sampled.mean_b2a + 1e-6
        ref = np.sqrt(MC.closest_ref(target, v, f)[0].astype(np.float64))
        assert exact.mean_b2a == pytest.approx(ref[keep].mean(), rel=1e-12, abs=0)
        assert ops.point_mesh_distance(td, (vd, fd), max_dist) == (exact.mean_b2a, exact.n_b2a)
        assert ops.point_mesh_distance(td, ops.mesh_index(vd, fd, cell=0.5), max_dist) == (exact.mean_b2a, exact.n_b2a)


def test_mesh_to_mesh_of_a_mesh_with_itself_is_zero():
    """the planar grid: its samples have z = 0 and exact products, so the interior candidate of the face that holds a
    sample returns the sample itself (an icosphere's fp32 samples are an ulp off their faces' planes)"""
    v, f = MC.planar()
    r = mesh_to_mesh((_dev(v), _dev(f)), (_dev(v), _dev(f)), 0.21)
    assert r.n_a2b == r.n_b2a == len(v) + len(NC.sample_ref(v, f, 0.21)[0])
    assert (r.mean_a2b, r.mean_b2a, r.max_a2b, r.max_b2a) == (0.0, 0.0, 0.0, 0.0)


def test_mesh_to_mesh_of_two_icosphere_levels():
    """Both meshes are inscribed in the unit sphere and level 3 refines level 2: every point of one is a radial lift
    of a point of the other by at most the sagitta of level 2's longest edge (a level-3 point is a convex combination
    of level-2 vertices, which are not moved, and of lifted edge midpoints, which move by their edge's sagitta, and the
    unlifted combination lies on the level-2 face).  The lifted midpoint of the longest edge attains the sagitta, so
    the maxima get the rounding of the fp32 vertices, 4 * 2^-24, on top; the means are strictly below."""
    (v3, f3), (v2, f2) = NC.icosphere(3), NC.icosphere(2)
    edge = np.sqrt(((v2.astype(np.float64)[f2] - v2.astype(np.float64)[np.roll(f2, 1, axis=1)]) ** 2).sum(-1)).max()
    sagitta = 1.0 - math.sqrt(1.0 - edge * edge / 4.0)
    r = mesh_to_mesh((_dev(v3), _dev(f3)), (_dev(v2), _dev(f2)), 0.02)
    print(f"sagitta {sagitta:.6e}: {r}")
    assert 0.0 < r.mean_a2b < sagitta and 0.0 < r.mean_b2a < sagitta
    assert 0.0 < r.max_a2b <= sagitta + 4 * 2.0 ** -24 and 0.0 < r.max_b2a <= sagitta + 4 * 2.0 ** -24
    assert r.mean_a2b <= r.max_a2b and r.mean_b2a <= r.max_b2a
    assert r.n_a2b == len(v3) + len(NC.sample_ref(v3, f3, 0.02)[0])
    cut = mesh_to_mesh((_dev(v3), _dev(f3)), (_dev(v2), _dev(f2)), 0.02, max_dist=r.mean_a2b)
    assert 0 < cut.n_a2b < r.n_a2b and cut.max_a2b < r.mean_a2b and cut.mean_a2b < r.mean_a2b


# ---- G7: medium size ----------------------------------------------------------------------------------------
def test_medium_size_against_the_fp64_rule():
    v, f = NC.icosphere(5)
    q = NC.sphere_clouds()[0]
    assert len(f) == 20480 and len(q) == 200000
    index = ops.mesh_index(_dev(v), _dev(f))
    qd = _dev(q)
    d2, face, point = index.query(qd)
    d64 = MC.closest_ref_near(q, v, f)
    got = d2.cpu().numpy().astype(np.float64)
    err = np.abs(np.sqrt(got) - np.sqrt(d64)) / MC.unit(q, v, d64)
    print(f"max |sqrt(d2) - sqrt(d2_64)| = {err.max():.3f} units of 2^-24 max(M, d)")
    assert err.max() <= 8.0
    # the reported point is at the reported distance and on the reported face's box
    w = q.astype(np.float64) - point.cpu().numpy().astype(np.float64)
    assert np.abs(np.sqrt((w * w).sum(1)) - np.sqrt(got)).max() <= 2.0 ** -22
    assert face.min() >= 0 and face.max() < len(f)
    again = index.query(qd)
    assert all(torch.equal(a, b) for a, b in zip((d2, face, point), again))
