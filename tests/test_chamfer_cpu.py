"""The restatements and inputs of the Chamfer-evaluation tests have the properties the GPU tests rely on, and the new
ops check their arguments before they touch the library (runs anywhere)."""
import numpy as np
import pytest
import torch

import nn_cases as NC
from hashmodnffbanks_idr_amd import ops
from hashmodnffbanks_idr_amd.evaluation import mesh_chamfer


def _area(verts, faces):
    v = verts.astype(np.float64)[faces]
    return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)


def test_right_triangle_counts():
    for density, want in NC.RIGHT_COUNTS.items():
        pts, owner = NC.sample_ref(*NC.RIGHT, density)
        assert len(pts) == want == len(owner) and pts.dtype == np.float32
    pts, _ = NC.sample_ref(*NC.RIGHT, 0.3)
    # i outer, j inner: (u, v) = (1/6, 1/6), (1/6, 1/2), (1/2, 1/6)
    assert np.allclose(pts, [[1 / 6, 1 / 6, 0], [1 / 6, 1 / 2, 0], [1 / 2, 1 / 6, 0]], atol=1e-7)
    eq = np.array([[0, 0, 0], [1, 0, 0], [0.5, 3 ** 0.5 / 2, 0]], np.float32)
    assert len(NC.sample_ref(eq, [[0, 1, 2]], 0.05)[0]) == 153


def test_sample_density_on_a_sphere():
    verts, faces = NC.icosphere()
    v = verts.astype(np.float64)[faces]
    edges = np.concatenate([np.linalg.norm(v[:, i] - v[:, (i + 1) % 3], axis=1) for i in range(3)])
    density = 0.01
    assert edges.min() >= 10 * density
    _, owner = NC.sample_ref(verts, faces, density)
    count = np.bincount(owner, minlength=len(faces))
    want = _area(verts, faces) / density ** 2
    assert np.all(np.abs(count - want) <= 0.15 * want)
    assert abs(count.sum() - want.sum()) <= 0.15 * want.sum()


def test_odd_faces_and_big_face():
    verts, faces = NC.odd_faces()
    n1, n2, _ = NC.sample_counts(verts, faces, 0.05)
    assert n1[0] == 0 and n1[1] == 0 and n1[3] == 0 and n1[2] >= 1 and n1[4] >= 1
    verts, faces = NC.big_among_small()
    n1, _, _ = NC.sample_counts(verts, faces, 0.01)
    assert (n1 > 250).sum() == 1 and 250 < n1.max() < 400 and np.median(n1) < 10


def test_tie_case_has_ties():
    p, q = NC.cloud("lattice")
    k = NC.n_minimisers(q, p)
    assert np.all(k[:343] == 8) and np.all(k[343:443] >= 1) and np.all(k[443:] == 1)
    d2, idx = NC.reference("lattice")
    assert np.all(d2[443:] == 0) and np.array_equal(idx[443:], np.arange(512))
    assert np.all(d2[:343] == 0.75)
    # the lowest index of the 8 corners is the corner with the smallest coordinates
    assert np.array_equal(p[idx[:343]], np.floor(q[:343]))


def test_nn_ref_is_the_nearest_neighbour():
    from scipy.spatial import cKDTree
    p, q = NC.cloud("uniform_4097_1000")
    d2, idx = NC.reference("uniform_4097_1000")
    d, k = cKDTree(p.astype(np.float64)).query(q.astype(np.float64))
    # fp32 rounding of the expression: 5 * 2^-24 relative (difference, square, two sums)
    assert np.allclose(d2, d * d, rtol=1e-6, atol=0)
    exact = np.linalg.norm(p[idx].astype(np.float64) - q, axis=1)
    assert np.all(exact <= d * (1 + 1e-6))
    assert np.mean(idx == k) > 0.99
    d2c, idxc = NC.nn_ref(q, p, np.float32(1e-3))
    far = d2 > np.float32(1e-3)
    assert far.any() and not far.all()
    assert np.all(idxc[far] == -1) and np.all(np.isinf(d2c[far])) and np.array_equal(idxc[~far], idx[~far])


def test_clouds_are_what_they_claim():
    p, q = NC.cloud("clusters")
    assert p[:200, 0].max() < 1.0 and p[200:, 0].min() >= 100.0 and q[:, 0].min() < 0 and q[:, 0].max() > 101
    p, q = NC.cloud("identical")
    assert np.all(p == p[0])
    p, q = NC.cloud("plane")
    assert np.all(p[:, 2] == 0) and np.ptp(q[:, 2]) > 1
    p, q = NC.cloud("outside")
    assert np.abs(q).max() > 90 and all((q[:, a] < -1).any() and (q[:, a] > 2).any() for a in range(3))
    for name in NC.CLOUDS:
        p, _ = NC.cloud(name)
        assert len(NC.cells(p)) == 3


def test_grid_choice():
    h, g = ops._nn_grid([0, 0, 0], [7, 7, 7], 512, 1)
    assert h == 1.0 and g == [8, 8, 8]
    h, g = ops._nn_grid([0, 0, 0], [1, 1, 0], 1000, None)
    assert g[2] == 1 and g[0] == g[1] and 100 <= g[0] * g[1] <= 1000
    h, g = ops._nn_grid([0, 0, 0], [0, 0, 0], 5, None)
    assert g == [1, 1, 1]
    h, g = ops._nn_grid([-1, -1, -1], [1, 1, 1], 10 ** 9, None)
    assert g[0] * g[1] * g[2] <= ops.NN_MAX_CELLS <= 1 << 26
    with pytest.raises(ValueError, match="NN_MAX_CELLS"):
        ops._nn_grid([0, 0, 0], [1, 1, 1], 10, 1e-4)


def test_arguments_are_checked_before_the_library():
    p = torch.zeros(8, 3)
    f = torch.zeros(2, 3, dtype=torch.int32)
    meta = torch.zeros(8, 3, device="meta")
    bad_clouds = [p.double(), torch.zeros(8, 4), torch.zeros(3, 8).t(), torch.zeros(8), None]
    for bad in bad_clouds:
        with pytest.raises(ValueError):
            ops.nn_index(bad)
        with pytest.raises(ValueError):
            ops.nearest_neighbors(bad, p)
        with pytest.raises(ValueError):
            ops.nearest_neighbors(p, bad)
        with pytest.raises(ValueError):
            ops.chamfer_distance(bad, p)
        with pytest.raises(ValueError):
            ops.chamfer_distance(p, bad)
        if bad is not None:
            with pytest.raises(ValueError):
                ops.mesh_sample_surface(bad, f, 0.1)
    with pytest.raises(ValueError, match="devices"):
        ops.nearest_neighbors(p, meta)
    with pytest.raises(ValueError, match="devices"):
        ops.chamfer_distance(meta, p)
    with pytest.raises(ValueError, match="devices"):
        ops.mesh_sample_surface(meta, f, 0.1)
    with pytest.raises(ValueError, match="at least one"):
        ops.nn_index(torch.zeros(0, 3))
    with pytest.raises(ValueError, match="at least one"):
        ops.chamfer_distance(p, torch.zeros(0, 3))
    for cell in (0, -1.0, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="cell"):
            ops.nn_index(p, cell=cell)
    for md in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_dist"):
            ops.nearest_neighbors(p, p, max_dist=md)
        with pytest.raises(ValueError, match="max_dist"):
            ops.chamfer_distance(p, p, max_dist=md)
    for density in (0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="density"):
            ops.mesh_sample_surface(p, f, density)
        with pytest.raises(ValueError, match="density"):
            mesh_chamfer((p, f), p, density)
    for bad_faces in (f.long(), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32).t()):
        with pytest.raises(ValueError, match="int32"):
            ops.mesh_sample_surface(p, bad_faces, 0.1)
    with pytest.raises(ValueError, match="mesh"):
        mesh_chamfer("mesh.ply", p, 0.1)


def test_result_record():
    r = ops.ChamferResult(1.0, 3.0, 5, 7)
    assert r.overall == 2.0 and (r.mean_a2b, r.mean_b2a, r.n_a2b, r.n_b2a, r.n_cloud) == (1.0, 3.0, 5, 7, None)
    assert np.isnan(ops.ChamferResult(float("nan"), 3.0, 0, 7).overall)
