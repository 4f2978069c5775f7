"""The device Chamfer evaluation against its numpy restatements (tests/nn_cases.py): exact nearest neighbours bit for
bit against the fp32 brute force, triangle upsampling bit for bit against the fp64 rule, the metric against cKDTree."""
import functools

import numpy as np
import pytest
import torch

import nn_cases as NC
from hashmodnffbanks_idr_amd import ops
from hashmodnffbanks_idr_amd._lib import HashmodError
from hashmodnffbanks_idr_amd.evaluation import mesh_chamfer
from hashmodnffbanks_idr_amd.utils.plots import TriMesh

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # a copy: the shared inputs are read-only


def _check_nn(got, want):
    d2, idx = got
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32
    assert torch.equal(idx.cpu(), torch.from_numpy(want[1].copy())), "index differs from the brute force"
    assert torch.equal(d2.cpu(), torch.from_numpy(want[0].copy())), "d2 differs from the brute force"


# ---- G1: bit-exact against nn_ref -----------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(3), ids=["default", "one_cell", "fine"])
@pytest.mark.parametrize("name", NC.CLOUDS)
def test_nearest_neighbors_equal_brute_force(name, which):
    p, q = NC.cloud(name)
    cell = NC.cells(p)[which]
    _check_nn(ops.nearest_neighbors(_dev(q), _dev(p), cell=cell), NC.reference(name))


def test_lattice_points_on_cell_faces():
    p, q = NC.cloud("lattice")
    index = ops.nn_index(_dev(p), cell=1)
    assert index.lo == [0.0, 0.0, 0.0] and index.h == 1.0 and index.g == [8, 8, 8]
    _check_nn(index.query(_dev(q)), NC.reference("lattice"))
    # the records are the points by cell, ascending original index inside a cell; here one point per cell
    cs = index.cell_start.cpu().numpy()
    assert np.array_equal(cs, np.arange(513))
    rec = index.records.cpu().numpy()
    assert np.array_equal(rec[:, :3], p) and np.array_equal(rec[:, 3].view(np.int32), np.arange(512))


def test_records_keep_index_order_inside_a_cell():
    p, _ = NC.cloud("uniform_4097_1000")
    index = ops.nn_index(_dev(p), cell=0.25)
    cs = index.cell_start.cpu().numpy()
    orig = index.records.cpu().numpy()[:, 3].view(np.int32)
    assert cs[0] == 0 and cs[-1] == len(p) and np.all(np.diff(cs) >= 0) and len(cs) == int(np.prod(index.g)) + 1
    assert np.array_equal(np.sort(orig), np.arange(len(p)))
    for c in range(len(cs) - 1):
        assert np.all(np.diff(orig[cs[c]:cs[c + 1]]) > 0)


def test_empty_query():
    p, _ = NC.cloud("uniform_63_64")
    d2, idx = ops.nearest_neighbors(torch.zeros((0, 3), device="cuda"), _dev(p))
    assert d2.shape == (0,) and idx.shape == (0,) and d2.dtype == torch.float32 and idx.dtype == torch.int32


# ---- G2: max_dist ---------------------------------------------------------------------------------------------
def test_max_dist_boundary_is_reported():
    p = _dev(NC.lattice())
    q = _dev(np.array([[10, 11, 7]], np.float32))                    # (7, 7, 7) + (3, 4, 0): d2 == 25 exactly
    d2, idx = ops.nearest_neighbors(q, p, max_dist=5.0, cell=1)
    assert d2.tolist() == [25.0] and idx.tolist() == [511]
    below = float(np.nextafter(np.float32(5.0), np.float32(0.0)))
    for cell in (1, None, 100.0):
        d2, idx = ops.nearest_neighbors(q, p, max_dist=below, cell=cell)
        assert d2.tolist() == [float("inf")] and idx.tolist() == [-1]
        d2, idx = ops.nearest_neighbors(q, p, max_dist=5.0, cell=cell)
        assert d2.tolist() == [25.0] and idx.tolist() == [511]


@pytest.mark.parametrize("which", range(3), ids=["default", "one_cell", "fine"])
def test_max_dist_on_clusters(which):
    p, q = NC.cloud("clusters")
    max_dist = 10.0
    md2 = float(np.float32(max_dist) * np.float32(max_dist))
    want = NC.reference("clusters", md2)
    full = NC.reference("clusters")
    far = full[0] > np.float32(md2)
    assert far.any() and not far.all()
    assert np.all(want[1][far] == -1) and np.array_equal(want[1][~far], full[1][~far])
    _check_nn(ops.nearest_neighbors(_dev(q), _dev(p), max_dist=max_dist, cell=NC.cells(p)[which]), want)


# ---- G3: medium size against fp64 -----------------------------------------------------------------------------
def test_medium_size_against_fp64():
    p, q = NC.sphere_clouds()
    dist = NC.one_sided_ref(q, p)
    pd, qd = _dev(p), _dev(q)
    d2, idx = ops.nearest_neighbors(qd, pd)
    # the difference, the square and the two sums round once each: <= 5 * 2^-24 ~ 3e-7 relative
    got = d2.cpu().numpy().astype(np.float64)
    rel = np.abs(got - dist * dist) / (dist * dist)
    print("max relative error of d2 against fp64:", rel.max())
    assert rel.max() <= 1e-6
    chosen = np.linalg.norm(p[idx.cpu().numpy()].astype(np.float64) - q.astype(np.float64), axis=1)
    print("max ratio of the chosen point's distance to the minimum:", (chosen / dist).max())
    assert np.all(chosen <= dist * (1 + 1e-6))
    again = ops.nearest_neighbors(qd, pd)
    assert torch.equal(again[0], d2) and torch.equal(again[1], idx)
    index = ops.nn_index(pd)
    built = index.query(qd)
    assert torch.equal(built[0], d2) and torch.equal(built[1], idx)
    part = index.query(qd[:1000])                                    # the result does not depend on m
    assert torch.equal(part[0], d2[:1000]) and torch.equal(part[1], idx[:1000])


# ---- G4: errors -----------------------------------------------------------------------------------------------
def test_bad_coordinates_and_indices_raise():
    p, q = (_dev(a) for a in NC.cloud("uniform_4097_1000"))
    for bad in (float("nan"), float("inf"), -float("inf")):
        pb = p.clone()
        pb[1234, 1] = bad
        with pytest.raises(HashmodError, match="non-finite"):
            ops.nn_index(pb)
        with pytest.raises(HashmodError, match="non-finite"):
            ops.nearest_neighbors(q, pb)
        qb = q.clone()
        qb[77, 2] = bad
        with pytest.raises(HashmodError, match="non-finite"):
            ops.nearest_neighbors(qb, p)
        with pytest.raises(HashmodError, match="non-finite"):
            ops.chamfer_distance(qb, p)
    _check_nn(ops.nearest_neighbors(q, p), NC.reference("uniform_4097_1000"))
    verts, faces = (_dev(a) for a in NC.icosphere())
    for bad in (verts.shape[0], -1):
        f = faces.clone()
        f[17, 2] = bad
        with pytest.raises(HashmodError, match="outside"):
            ops.mesh_sample_surface(verts, f, 0.05)
    with pytest.raises(HashmodError, match="CPU"):
        ops.nn_index(p.cpu())
    with pytest.raises(HashmodError, match="CPU"):
        ops.mesh_sample_surface(verts.cpu(), faces.cpu(), 0.05)
    with pytest.raises(ValueError, match="devices"):
        ops.nearest_neighbors(q.cpu(), p)


# ---- G5: mesh_sample_surface equals sample_ref ------------------------------------------------------------------
def _check_samples(verts, faces, density):
    want_pts, want_face = NC.sample_ref(verts, faces, density)
    pts, face_of = ops.mesh_sample_surface(_dev(verts), _dev(np.asarray(faces, np.int32)), density, return_face=True)
    assert pts.dtype == torch.float32 and face_of.dtype == torch.int32 and pts.shape == (len(want_pts), 3)
    got_count = np.bincount(face_of.cpu().numpy(), minlength=len(faces))
    want_count = np.bincount(want_face, minlength=len(faces))
    assert np.array_equal(got_count, want_count), np.nonzero(got_count != want_count)[0][:10]
    assert torch.equal(face_of.cpu(), torch.from_numpy(want_face))
    assert torch.equal(pts.cpu(), torch.from_numpy(want_pts))
    only = ops.mesh_sample_surface(_dev(verts), _dev(np.asarray(faces, np.int32)), density)
    assert torch.equal(only, pts)
    return len(want_pts)


@pytest.mark.parametrize("density", sorted(NC.RIGHT_COUNTS))
def test_sample_right_triangle(density):
    assert _check_samples(*NC.RIGHT, density) == NC.RIGHT_COUNTS[density]


def test_sample_odd_faces():
    verts, faces = NC.odd_faces()
    n = _check_samples(verts, faces, 0.05)
    assert n > 0
    _, face_of = ops.mesh_sample_surface(_dev(verts), _dev(faces), 0.05, return_face=True)
    assert set(face_of.cpu().tolist()) == {2, 4}                      # no area, repeated vertex, too small: nothing
    assert _check_samples(verts, faces[[0, 1, 3]], 0.05) == 0


def test_sample_one_big_face_among_small_ones():
    verts, faces = NC.big_among_small()
    assert _check_samples(verts, faces, 0.01) > 40000


def test_sample_more_rows_than_one_wave_takes():
    assert _check_samples(*NC.RIGHT, 1.0 / 2500.5) > 3000000          # 2501 rows: three waves share the face


@functools.lru_cache(maxsize=None)
def _sphere_mesh():
    vol, spacing = NC.sphere_volume()
    verts, faces, normals = ops.marching_cubes(_dev(vol), 0.0, spacing)
    return verts, faces, normals


def test_sample_marching_cubes_sphere():
    verts, faces, _ = _sphere_mesh()
    n = _check_samples(verts.cpu().numpy(), faces.cpu().numpy(), 0.02)
    assert n > faces.shape[0]                                         # more than one sample per face on average


def test_sample_empty_faces():
    verts = _dev(NC.RIGHT[0])
    pts, face_of = ops.mesh_sample_surface(verts, torch.zeros((0, 3), dtype=torch.int32, device="cuda"), 0.1, True)
    assert pts.shape == (0, 3) and face_of.shape == (0,) and pts.dtype == torch.float32
    assert ops.mesh_sample_surface(verts, _dev(NC.RIGHT[1]), 0.6).shape == (0, 3)


# ---- G6: chamfer_distance and mesh_chamfer -----------------------------------------------------------------------
def _close(a, b):
    return abs(a - b) <= 1e-6 * abs(b)           # the bound of G3 carried through a mean


def test_chamfer_against_fp64_reference():
    verts, faces, normals = _sphere_mesh()
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    density, max_dist = 0.02, 0.03
    cloud = np.concatenate([v, NC.sample_ref(v, f, density)[0]])
    target = NC.perturbed_target(v, 20000, 0.02)
    ma, mb, overall, na, nb, d_ab, d_ba = NC.chamfer_ref(cloud, target, max_dist)
    for d in (d_ab, d_ba):
        assert np.abs(d / max_dist - 1).min() > 1e-6                  # no distance hinges on rounding at the cut-off
    assert 0 < na < len(cloud) and 0 < nb < len(target)               # some distances are excluded, both ways

    r = ops.chamfer_distance(_dev(cloud), _dev(target), max_dist)
    print("chamfer", r, "reference", (ma, mb, overall, na, nb))
    assert (r.n_a2b, r.n_b2a) == (na, nb)
    assert _close(r.mean_a2b, ma) and _close(r.mean_b2a, mb) and _close(r.overall, overall)
    assert r.overall == 0.5 * (r.mean_a2b + r.mean_b2a)
    assert tuple(ops.chamfer_distance(_dev(cloud), _dev(target), max_dist)) == tuple(r)

    m = mesh_chamfer((verts, faces, normals), _dev(target), density, max_dist)
    assert m.n_cloud == len(cloud) and tuple(m)[:5] == tuple(r)[:5]
    assert tuple(mesh_chamfer((verts, faces), _dev(target), density, max_dist)) == tuple(m)
    assert tuple(mesh_chamfer(TriMesh(v, f), _dev(target), density, max_dist)) == tuple(m)

    ma, mb, overall, na, nb, _, _ = NC.chamfer_ref(cloud, target, None)
    r = mesh_chamfer((verts, faces), _dev(target), density)
    assert (r.n_a2b, r.n_b2a, r.n_cloud) == (len(cloud), len(target), len(cloud)) == (na, nb, len(cloud))
    assert _close(r.mean_a2b, ma) and _close(r.mean_b2a, mb) and _close(r.overall, overall)

    none = ops.chamfer_distance(_dev(cloud), _dev(target + np.float32(50.0)), max_dist)
    assert (none.n_a2b, none.n_b2a) == (0, 0) and np.isnan(none.mean_a2b) and np.isnan(none.overall)
