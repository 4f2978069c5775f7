"""CPU-side checks of the point-to-mesh distance: the numpy restatement of the definition (tests/mesh_dist_cases.py,
the reference of csrc/hm_mesh_dist.hip) against itself in fp64 and against a dense sample, the claims the cases make,
and the argument checks of the new ops, which run before the library is touched."""
import numpy as np
import pytest
import torch

import mesh_dist_cases as MC
import nn_cases as NC


def _measured_queries(v, f, rng):
    return NC._f4(np.concatenate([MC.box_queries(v, 1000, rng), MC.centroid_queries(v, f, 300, rng)]))


@pytest.mark.parametrize("name", ["icosphere2", "icosphere3", "odd_faces", "big_among_small"])
def test_fp32_restatement_against_fp64(name):
    """|sqrt(d2_32) - sqrt(d2_64)| <= 8 * 2^-24 * max(M, d): the plane-projection interior is well conditioned.  The
    figure says nothing about the kernel, which is tested bit for bit against the fp32 restatement."""
    v, f = {"icosphere2": lambda: NC.icosphere(2), "icosphere3": lambda: NC.icosphere(3), "odd_faces": NC.odd_faces,
            "big_among_small": NC.big_among_small}[name]()
    q = _measured_queries(v, f, np.random.default_rng(3))
    d32 = MC.closest_ref(q, v, f)[0]
    d64 = MC.closest_ref(q, v, f, dtype=np.float64)[0]
    assert d32.dtype == np.float32 and d64.dtype == np.float64
    assert np.isfinite(d32).all() and np.isfinite(d64).all()
    err = np.abs(np.sqrt(d32.astype(np.float64)) - np.sqrt(d64)) / MC.unit(q, v, d64)
    print(f"{name}: max |sqrt(d2_32) - sqrt(d2_64)| = {err.max():.3f} units of 2^-24 max(M, d)")
    assert err.max() <= 8.0


def test_fp64_rule_against_a_dense_sample():
    """every face of icosphere(1) sampled on the barycentric lattice i/n, j/n, corners and edges included.  A sample
    is a point of the mesh, so it never beats the rule.  The lattice has a point within s = (longest edge)/n of the
    rule's closest point ON THE SAME FEATURE (interior, edge or the vertex itself), and from there the offset is
    perpendicular to q's offset, so the sample's d2 exceeds the rule's by at most s^2."""
    v, f = NC.icosphere(1)
    n = 16
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    keep = i + j <= n
    bu, bv = i[keep] / n, j[keep] / n
    tri = v.astype(np.float64)[f]
    pts = (tri[:, None, 0] * (1 - bu - bv)[None, :, None] + tri[:, None, 1] * bu[None, :, None]
           + tri[:, None, 2] * bv[None, :, None]).reshape(-1, 3)
    spacing = np.sqrt(((tri - np.roll(tri, 1, axis=1)) ** 2).sum(-1)).max() / n
    rng = np.random.default_rng(4)
    q = NC._f4(np.concatenate([MC.box_queries(v, 300, rng), MC.centroid_queries(v, f, 100, rng, off=0.02)]))
    rule = MC.closest_ref(q, v, f, dtype=np.float64)[0]
    sample = ((q.astype(np.float64)[:, None, :] - pts[None]) ** 2).sum(-1).min(1)
    print(f"sample - rule: min {(sample - rule).min():.3e}, max {(sample - rule).max():.3e}, s^2 = {spacing ** 2:.3e}")
    assert (sample >= rule - 1e-12).all()
    assert (sample - rule <= spacing ** 2 + 1e-12).all()


def test_planar_values_and_ties():
    v, f, q = MC.case("planar")
    d2, face, point, feature = MC.reference("planar")
    ties = MC.n_minimisers(q, v, f)
    assert d2.tolist() == [d for _, d, _ in MC.PLANAR_QUERIES]
    assert ties.tolist() == [k for _, _, k in MC.PLANAR_QUERIES]
    assert {1, 2, 6} <= set(ties.tolist())
    assert {1.0, 0.25, 4.0, 2.0, 0.0} == set(d2.tolist())
    assert (point[:, 2] == 0).all() and (feature >= 0).all()


@pytest.mark.parametrize("name", ["icosphere1", "icosphere2", "planar", "big_among_small"])
def test_lowest_face_wins(name):
    v, f, q = MC.case(name)
    d2, face, _, _ = MC.reference(name)
    tri = v[f]
    d = MC.face_values(q[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])[0]
    hit = d == d2[:, None]
    assert (face == hit.argmax(1)).all() and hit[np.arange(len(q)), face].all()
    if name.startswith("icosphere"):
        # shared edges and vertices: ordinary queries exercise the tie rule
        assert (hit.sum(1) > 1).mean() > 0.1


def test_odd_faces_are_total():
    v, f, q = MC.case("odd_faces")
    tri = v[f]
    d, p, k = MC.face_values(q[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
    assert np.isfinite(d).all() and np.isfinite(p).all() and (k >= 0).all()
    assert (k[:, 0] > 0).all() and (k[:, 1] > 0).all()          # the faces without area have no interior
    for dtype in (np.float32, np.float64):
        out = MC.closest_ref(q, v, f, dtype=dtype)
        assert np.isfinite(out[0]).all() and np.isfinite(out[2]).all()


def test_max_dist_cuts_some_queries_and_not_all():
    v, f, q = MC.case("clusters")
    md2 = float(np.float32(MC.CLUSTERS_MAX_DIST) ** 2)
    d2, face, point, feature = MC.reference("clusters", md2)
    full = MC.reference("clusters")[0]
    cut = face < 0
    assert 0 < cut.sum() < len(q)
    assert np.isinf(d2[cut]).all() and np.isnan(point[cut]).all() and (feature[cut] == -1).all()
    assert (full[cut] > md2).all() and np.array_equal(d2[~cut], full[~cut])


def test_near_reference_is_the_full_rule():
    """the pruned fp64 reference of the medium-size GPU test gives the brute force's values"""
    v, f = NC.icosphere(3)
    q = _measured_queries(v, f, np.random.default_rng(6))[::4]
    assert np.array_equal(MC.closest_ref_near(q, v, f), MC.closest_ref(q, v, f, dtype=np.float64)[0])


def test_argument_checks():
    """ValueError before the library is touched: there is no GPU here, and no call below reaches one"""
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd.evaluation import mesh_chamfer, mesh_to_mesh
    v, f, q = (torch.from_numpy(np.array(a)) for a in MC.case("single"))
    meta = dict(device="meta")
    vm, fm, qm = torch.zeros(3, 3, **meta), torch.zeros(1, 3, dtype=torch.int32, **meta), torch.zeros(5, 3, **meta)
    for bad in (v.double(), torch.zeros(3, 4), torch.zeros(3, 8).t(), torch.zeros(8), None):
        with pytest.raises(ValueError):
            ops.mesh_index(bad, f)
        with pytest.raises(ValueError):
            ops.mesh_closest_point(bad, v, f)
        with pytest.raises(ValueError):
            ops.mesh_closest_point(q, bad, f)
        with pytest.raises(ValueError):
            ops.point_mesh_distance(bad, (v, f))
    for bad in (f.long(), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32).t(), None):
        with pytest.raises(ValueError):
            ops.mesh_index(v, bad)
        with pytest.raises(ValueError):
            ops.mesh_closest_point(q, v, bad)
    # a CPU tensor of the right dtype and shape
    with pytest.raises(ValueError, match="GPU"):
        ops.mesh_index(v, f)
    with pytest.raises(ValueError, match="GPU"):
        ops.mesh_closest_point(q, v, f)
    with pytest.raises(ValueError, match="GPU"):
        ops.point_mesh_distance(q, (v, f))
    with pytest.raises(ValueError, match="at least one face"):
        ops.mesh_index(vm, torch.zeros(0, 3, dtype=torch.int32, **meta))
    for cell in (0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="cell"):
            ops.mesh_index(vm, fm, cell=cell)
        with pytest.raises(ValueError, match="cell"):
            ops.mesh_closest_point(qm, vm, fm, cell=cell)
    for big_face in (0, -1, 1.5, "1", None, True):
        with pytest.raises(ValueError, match="big_face"):
            ops.mesh_index(vm, fm, big_face=big_face)
        with pytest.raises(ValueError, match="big_face"):
            ops.mesh_closest_point(qm, vm, fm, big_face=big_face)
    for md in (-1.0, float("nan"), "1"):
        with pytest.raises(ValueError, match="max_dist"):
            ops.mesh_closest_point(qm, vm, fm, max_dist=md)
        with pytest.raises(ValueError, match="max_dist"):
            ops.point_mesh_distance(qm, (vm, fm), max_dist=md)
    for flag in (1, None, "yes"):
        with pytest.raises(ValueError, match="return_point"):
            ops.mesh_closest_point(qm, vm, fm, return_point=flag)
        with pytest.raises(ValueError, match="return_feature"):
            ops.mesh_closest_point(qm, vm, fm, return_feature=flag)
        with pytest.raises(ValueError, match="surface"):
            mesh_chamfer((vm, fm), qm, 0.1, surface=flag)
    with pytest.raises(ValueError, match="mesh"):
        ops.point_mesh_distance(qm, "mesh.ply")
    for density in (0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="density"):
            mesh_to_mesh((vm, fm), (vm, fm), density)
    with pytest.raises(ValueError, match="max_dist"):
        mesh_to_mesh((vm, fm), (vm, fm), 0.1, max_dist=-1.0)
