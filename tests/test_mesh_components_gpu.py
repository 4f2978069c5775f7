"""The mesh cleanup kernels (csrc/hm_mesh_cc.hip) against TriMesh.split and its numpy restatement
(tests/mesh_cc_cases.py): labels, per-component areas, the submesh of a component, the largest component, the surface
moments, and get_surface_high_res_mesh(largest_component=True)."""
import numpy as np
import pytest
import torch

import mc_ref as M
import mesh_cc_cases as CC
from hashmodnffbanks_idr_amd import ops
from hashmodnffbanks_idr_amd._lib import HashmodError
from hashmodnffbanks_idr_amd.utils.plots import TriMesh, _surface_moments, get_surface_high_res_mesh

pytestmark = pytest.mark.gpu

# sums of at most 2e5 positive fp64 terms in two orders: 2e5 * 2^-53 ~ 2e-11 at worst, times 5
SUM_RTOL = 1e-10


def _dev(name):
    m = CC.case(name)
    return (torch.tensor(m["verts"]).cuda(), torch.tensor(m["faces"].astype(np.int32)).cuda(),
            torch.tensor(m["normals"]).cuda())


def _ref_label(name):
    return torch.tensor(CC.reference(name)["label"].astype(np.int32)).cuda()


def _same_mesh(got, want):
    """device (verts, faces, normals) equal to the numpy ones after the dtype cast"""
    for g, w in zip(got, want):
        w = torch.tensor(np.asarray(w))
        assert g.is_cuda and g.shape == w.shape, (g.shape, w.shape)
        assert torch.equal(g.cpu().to(w.dtype), w)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].dtype == torch.float32


@pytest.mark.parametrize("name", CC.NAMES)
def test_labels(name):
    m, ref = CC.case(name), CC.reference(name)
    _, faces, _ = _dev(name)
    label = ops.mesh_components(faces, len(m["verts"]))
    assert label.dtype == torch.int32 and label.shape == (len(m["verts"]),) and label.is_cuda
    assert torch.equal(label.cpu().long(), torch.tensor(ref["label"]))
    free = np.setdiff1d(np.arange(len(m["verts"])), m["faces"])
    assert np.array_equal(label.cpu().numpy()[free], free)


@pytest.mark.parametrize("name", CC.NAMES)
def test_component_areas(name):
    ref = CC.reference(name)
    verts, faces, _ = _dev(name)
    ids, area, count = ops.mesh_component_areas(verts, faces, _ref_label(name))
    assert ids.dtype == torch.int32 and area.dtype == torch.float64 and count.dtype == torch.int64
    assert torch.equal(ids.cpu().long(), torch.tensor(ref["ids"]))
    assert torch.equal(count.cpu(), torch.tensor(ref["count"]))
    err = np.abs(area.cpu().numpy() - ref["area"])
    print(name, "largest relative area error", (err / np.maximum(ref["area"], 1e-300)).max() if len(err) else 0.0)
    assert np.all(err <= SUM_RTOL * ref["area"])


@pytest.mark.parametrize("name", ["three", "noise_many", "unused", "repeated"])
def test_select_equals_every_split_part(name):
    m, ref = CC.case(name), CC.reference(name)
    verts, faces, normals = _dev(name)
    label = ops.mesh_components(faces, len(m["verts"]))
    parts = TriMesh(m["verts"], m["faces"], m["normals"]).split(only_watertight=False)
    assert len(parts) == len(ref["ids"])
    for part, cid in zip(parts, ref["ids"]):
        got = ops.mesh_select(verts, faces, normals, label, int(cid))
        _same_mesh(got, (part.vertices, part.faces, part.vertex_normals))
    v, f, n = ops.mesh_select(verts, faces, None, label, int(ref["ids"][0]))
    assert n is None and torch.equal(f.cpu().long(), torch.tensor(parts[0].faces))
    # a label that owns no face: nothing is selected
    v, f, n = ops.mesh_select(verts, faces, normals, label, len(m["verts"]))
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)


@pytest.mark.parametrize("name", CC.NAMES)
def test_largest_component(name):
    got = ops.mesh_largest_component(*[_dev(name)[i] for i in (0, 1, 2)])
    want = CC.largest(name)
    _same_mesh(got, (want[0], want[1].astype(np.int64), want[2]))
    if name == CC.TIE:
        ref = CC.reference(name)
        assert ref["area"][0] == ref["area"][1]
        # the lower id: the first half of the vertices
        assert torch.equal(got[0].cpu(), torch.tensor(CC.case(name)["verts"][:len(want[0])]))


def test_largest_component_without_normals():
    verts, faces, _ = _dev("three")
    want = CC.largest("three")
    v, f, n = ops.mesh_largest_component(verts, faces)
    assert n is None and torch.equal(v.cpu(), torch.tensor(want[0])) and torch.equal(f.cpu().long(),
                                                                                        torch.tensor(want[1]))


@pytest.mark.parametrize("name", ["three", "noise"])
def test_surface_moments(name):
    m = CC.case(name)
    verts, faces, _ = _dev(name)
    area, mean, cov = ops.mesh_surface_moments(verts, faces)
    assert area.dtype == mean.dtype == cov.dtype == torch.float64 and mean.shape == (3,) and cov.shape == (3, 3)
    mesh = TriMesh(m["verts"], m["faces"])
    ref_mean, ref_cov = _surface_moments(mesh)
    a = mesh.area_faces
    # scale of the second moments: the area-weighted mean of |v|^2 over the triangles' corners
    scale = float((a * (mesh.vertices[mesh.faces] ** 2).sum(-1).mean(1)).sum() / a.sum())
    e_area = abs(area.item() - mesh.area) / mesh.area
    e_mean = np.abs(mean.cpu().numpy() - ref_mean).max() / np.abs(ref_mean).max()
    e_cov = np.abs(cov.cpu().numpy() - ref_cov).max() / scale
    print(name, "area", e_area, "mean", e_mean, "cov / scale", e_cov)
    assert e_area <= SUM_RTOL
    assert np.all(np.abs(mean.cpu().numpy() - ref_mean) <= SUM_RTOL * np.abs(ref_mean).max())
    assert np.all(np.abs(cov.cpu().numpy() - ref_cov) <= SUM_RTOL * scale)
    assert torch.equal(cov, cov.t())


def test_two_calls_give_the_same_bits():
    verts, faces, normals = _dev("noise")
    nv = verts.shape[0]

    def run():
        label = ops.mesh_components(faces, nv)
        ids, area, count = ops.mesh_component_areas(verts, faces, label)
        big = ops.mesh_largest_component(verts, faces, normals)
        sel = ops.mesh_select(verts, faces, normals, label, int(ids[3]))
        return (label, ids, area, count, *big, *sel, *ops.mesh_surface_moments(verts, faces))

    first, second = run(), run()
    for a, b in zip(first, second):
        assert a.dtype == b.dtype and torch.equal(a, b)


def test_bad_indices_and_arguments():
    verts, faces, normals = _dev("three")
    nv = verts.shape[0]
    label = _ref_label("three")
    for bad in (nv, -1):
        f = faces.clone()
        f[1234, 1] = bad
        with pytest.raises(HashmodError, match="outside"):
            ops.mesh_components(f, nv)
        with pytest.raises(HashmodError, match="outside"):
            ops.mesh_component_areas(verts, f, label)
        with pytest.raises(HashmodError, match="outside"):
            ops.mesh_select(verts, f, normals, label, 0)
        with pytest.raises(HashmodError, match="outside"):
            ops.mesh_surface_moments(verts, f)
        with pytest.raises(HashmodError, match="outside"):
            ops.mesh_largest_component(verts, f, normals)
    # the bad index was reported, not dereferenced: the process goes on and a correct call is right
    assert torch.equal(ops.mesh_components(faces, nv), label)
    _same_mesh(ops.mesh_largest_component(verts, faces, normals), CC.largest("three"))

    with pytest.raises(HashmodError, match="CPU"):
        ops.mesh_components(faces.cpu(), nv)
    with pytest.raises(HashmodError, match="CPU"):
        ops.mesh_component_areas(verts.cpu(), faces, label)
    with pytest.raises(HashmodError, match="CPU"):
        ops.mesh_select(verts, faces, normals, label.cpu(), 0)
    with pytest.raises(HashmodError, match="CPU"):
        ops.mesh_largest_component(verts, faces, normals.cpu())
    with pytest.raises(HashmodError, match="CPU"):
        ops.mesh_surface_moments(verts.cpu(), faces.cpu())
    with pytest.raises(ValueError, match="int32"):
        ops.mesh_components(faces.long(), nv)
    with pytest.raises(ValueError, match="int32"):
        ops.mesh_components(torch.zeros(8, 4, dtype=torch.int32, device="cuda"), nv)
    with pytest.raises(ValueError, match="int32"):
        ops.mesh_components(faces.t().contiguous().t(), nv)            # [F, 3] but not contiguous
    with pytest.raises(ValueError, match="fp32"):
        ops.mesh_largest_component(verts.double(), faces)
    with pytest.raises(ValueError, match="label"):
        ops.mesh_component_areas(verts, faces, label[:-1])
    with pytest.raises(ValueError, match="label"):
        ops.mesh_select(verts, faces, normals, label.long(), 0)


def test_no_faces():
    verts, faces, normals = _dev("empty")
    assert faces.shape == (0, 3)
    label = ops.mesh_components(faces, 5)
    assert torch.equal(label.cpu(), torch.arange(5, dtype=torch.int32))
    ids, area, count = ops.mesh_component_areas(verts, faces, label)
    assert ids.shape == area.shape == count.shape == (0,)
    assert ids.dtype == torch.int32 and area.dtype == torch.float64 and count.dtype == torch.int64
    v, f, n = ops.mesh_select(verts, faces, normals, label, 0)
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and n.dtype == torch.float32
    v, f, n = ops.mesh_largest_component(verts, faces, normals)
    assert v is verts and f is faces and n is normals
    area, mean, cov = ops.mesh_surface_moments(verts, faces)
    assert area.item() == 0.0 and area.dtype == torch.float64 and mean.shape == (3,) and cov.shape == (3, 3)
    assert ops.mesh_components(faces, 0).shape == (0,)


@pytest.mark.parametrize("sparse", [False, True])
def test_high_res_mesh_largest_component(sparse, tmp_path):
    c1, r1 = torch.tensor([-0.1, 0.0, 0.0], device="cuda"), 0.45
    c2, r2 = torch.tensor([0.55, 0.25, 0.1], device="cuda"), 0.12    # inside the aligned lattice's 0.2 margin

    def two_spheres(x):
        return torch.minimum((x - c1).norm(dim=1) - r1, (x - c2).norm(dim=1) - r2)

    whole = get_surface_high_res_mesh(two_spheres, 64, sparse=sparse)
    kept = get_surface_high_res_mesh(two_spheres, 64, sparse=sparse, largest_component=True)
    parts = whole.split(only_watertight=False)
    assert len(parts) == 2 and len(kept.split(only_watertight=False)) == 1
    best = parts[int(np.argmax([p.area for p in parts]))]
    assert len(best.faces) > len(whole.faces) // 2
    assert np.array_equal(kept.vertices, best.vertices) and np.array_equal(kept.faces, best.faces)
    assert np.array_equal(kept.vertex_normals, best.vertex_normals)
    assert kept.vertices.dtype == np.float64 and kept.faces.dtype == np.int64

    path = tmp_path / "kept.ply"
    kept.export(str(path))
    v, n, f = M.read_ply(str(path))
    assert np.array_equal(v, kept.vertices.astype(np.float32)) and np.array_equal(f, kept.faces)
    assert np.array_equal(n, kept.vertex_normals.astype(np.float32))
