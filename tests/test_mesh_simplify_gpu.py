"""The vertex-clustering kernels (csrc/hm_mesh_simplify.hip) behind ops.mesh_simplify against their numpy restatement
(tests/mesh_simplify_cases.py), and get_surface_high_res_mesh(simplify=k).

Tolerances.  Integer outputs are equal.  A position is one rounding to fp32 of an fp64 result; the kernel's and
numpy's fp64 results differ by reduction order and solve (about 21 k 2^-53 relative, nothing at this scale) and can
straddle a rounding boundary: one fp32 ulp at the largest coordinate, 2^-23 max|coord|, times two.  A normal has unit
length: 2^-22, on every cluster - tests/test_mesh_simplify_cpu.py shows that no compared cluster's unit normals cancel
below |sum n^| / k = 1e-3, which this file asserts again where it compares."""
import math

import numpy as np
import pytest
import torch

import mesh_simplify_cases as S
from hashmodnffbanks_idr_amd import ops
from hashmodnffbanks_idr_amd._lib import HashmodError
from hashmodnffbanks_idr_amd.utils.plots import get_surface_high_res_mesh

pytestmark = pytest.mark.gpu

ULP2 = 2.0 ** -22
MIN_NORMAL_RATIO = 1e-3


def _dev(name):
    m = S.case(name)
    return (torch.tensor(m["verts"]).cuda(), torch.tensor(m["faces"].astype(np.int32)).cuda(),
            torch.tensor(m["normals"]).cuda())


def _compare(got, ref, max_coord, what):
    """the op's four outputs (device) against the reference's"""
    verts, faces, normals, vmap = got
    assert verts.is_cuda and faces.is_cuda and vmap.is_cuda
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and vmap.dtype == torch.int32
    assert verts.shape == ref["verts"].shape and faces.shape == ref["faces"].shape, (verts.shape, faces.shape)
    assert torch.equal(faces.cpu().long(), torch.tensor(ref["faces"]))
    assert torch.equal(vmap.cpu().long(), torch.tensor(ref["vertex_map"]))
    err = np.abs(verts.cpu().numpy().astype(np.float64) - ref["verts"].astype(np.float64))
    print(what, "C", len(ref["verts"]), "G", len(ref["faces"]), "largest position error / max|coord|",
          err.max() / max_coord if err.size else 0.0)
    assert np.all(err <= ULP2 * max_coord)
    if ref["normals"] is None:
        assert normals is None
        return
    assert normals.is_cuda and normals.dtype == torch.float32 and normals.shape == ref["normals"].shape
    if len(ref["normals"]):
        assert ref["normal_ratio"].min() >= MIN_NORMAL_RATIO        # no cluster is left out
        nerr = np.abs(normals.cpu().numpy().astype(np.float64) - ref["normals"].astype(np.float64))
        print(what, "largest normal error", nerr.max())
        assert np.all(nerr <= ULP2)


@pytest.mark.parametrize("placement", S.PLACEMENTS)
@pytest.mark.parametrize("name", S.NAMES)
def test_against_reference(name, placement):
    m, ref = S.case(name), S.reference(name, placement)
    got = ops.mesh_simplify(*_dev(name), cell=m["cell"], placement=placement)
    _compare(got, ref, float(np.abs(m["verts"]).max()), f"{name} {placement}")


def test_two_calls_give_the_same_bits():
    for name in ("noise@1.7", "one_cell"):
        mesh, cell = _dev(name), S.case(name)["cell"]
        for placement in S.PLACEMENTS:
            first = ops.mesh_simplify(*mesh, cell=cell, placement=placement)
            second = ops.mesh_simplify(*mesh, cell=cell, placement=placement)
            for a, b in zip(first, second):
                assert a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("name", ["three@1.7", "noise@3.0", "strip_4097@0.8"])
def test_without_normals(name):
    m = S.case(name)
    verts, faces, normals = _dev(name)
    got = ops.mesh_simplify(verts, faces, None, cell=m["cell"], placement="mean")
    assert got[2] is None
    _compare(got, S.reference(name, "mean", with_normals=False), float(np.abs(m["verts"]).max()), name)
    with_normals = ops.mesh_simplify(verts, faces, normals, cell=m["cell"], placement="mean")
    assert torch.equal(got[0], with_normals[0]) and torch.equal(got[1], with_normals[1])
    assert torch.equal(got[3], with_normals[3])


def test_reg_reaches_the_kernel():
    m = S.case("noise@1.7")
    ref = S.simplify(m["verts"], m["faces"], m["normals"], m["cell"], "quadric", reg=0.5)
    got = ops.mesh_simplify(*_dev("noise@1.7"), cell=m["cell"], reg=0.5)
    assert not np.array_equal(ref["verts"], S.reference("noise@1.7")["verts"])
    _compare(got, ref, float(np.abs(m["verts"]).max()), "noise@1.7 reg=0.5")


def test_empty_inputs():
    verts, faces, normals = _dev("empty")
    v, f, n, vmap = ops.mesh_simplify(verts, faces, normals, cell=0.5)
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3) and v.is_cuda and f.is_cuda
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and n.dtype == torch.float32
    assert torch.equal(vmap.cpu(), torch.full((5,), -1, dtype=torch.int32))
    none = torch.zeros((0, 3), device="cuda")
    v, f, n, vmap = ops.mesh_simplify(none, faces, None, cell=0.5, placement="mean")
    assert v.shape == (0, 3) and f.shape == (0, 3) and n is None and vmap.shape == (0,) and vmap.dtype == torch.int32


def test_bad_arguments():
    verts, faces, normals = _dev("three@1.7")
    cell = S.case("three@1.7")["cell"]
    nv = verts.shape[0]
    with pytest.raises(ValueError, match="normals"):
        ops.mesh_simplify(verts, faces, None, cell=cell)
    with pytest.raises(ValueError, match="normals"):
        ops.mesh_simplify(verts, faces, None, cell=cell, placement="quadric")
    with pytest.raises(ValueError, match="placement"):
        ops.mesh_simplify(verts, faces, normals, cell=cell, placement="median")
    for bad in (None, 0, -1.0, math.nan, math.inf, 1e-60):
        with pytest.raises(ValueError, match="cell"):
            ops.mesh_simplify(verts, faces, normals, cell=bad)
    for bad in (None, 0, -0.05, math.nan, math.inf):
        with pytest.raises(ValueError, match="reg"):
            ops.mesh_simplify(verts, faces, normals, cell=cell, reg=bad)
    # the box is about 2 wide: 2e4 cells on an axis, 8e12 >= 2^31 in all
    with pytest.raises(ValueError, match=r"grid of \d+x\d+x\d+ cells.*2\^31"):
        ops.mesh_simplify(verts, faces, normals, cell=1e-4)
    v = verts.clone()
    v[77, 2] = math.nan
    with pytest.raises(HashmodError, match="non-finite"):
        ops.mesh_simplify(v, faces, normals, cell=cell)
    v[77, 2] = math.inf
    with pytest.raises(HashmodError, match="non-finite"):
        ops.mesh_simplify(v, faces, normals, cell=cell)
    for bad in (-1, nv):
        f = faces.clone()
        f[1234, 1] = bad
        with pytest.raises(HashmodError, match="outside"):
            ops.mesh_simplify(verts, f, normals, cell=cell)
    # the bad index was reported, not dereferenced: the process goes on and a correct call is right
    _compare(ops.mesh_simplify(verts, faces, normals, cell=cell), S.reference("three@1.7"),
             float(np.abs(S.case("three@1.7")["verts"]).max()), "after the bad calls")
    with pytest.raises(HashmodError, match="CPU"):
        ops.mesh_simplify(verts.cpu(), faces, normals, cell=cell)
    with pytest.raises(HashmodError, match="CPU"):
        ops.mesh_simplify(verts, faces.cpu(), normals, cell=cell)
    with pytest.raises(HashmodError, match="CPU"):
        ops.mesh_simplify(verts, faces, normals.cpu(), cell=cell)
    with pytest.raises(ValueError, match="int32"):
        ops.mesh_simplify(verts, faces.long(), normals, cell=cell)
    with pytest.raises(ValueError, match="int32"):
        ops.mesh_simplify(verts, torch.zeros(8, 4, dtype=torch.int32, device="cuda"), normals, cell=cell)
    with pytest.raises(ValueError, match="fp32"):
        ops.mesh_simplify(verts.double(), faces, normals, cell=cell)
    with pytest.raises(ValueError, match="fp32"):
        ops.mesh_simplify(verts.t().contiguous().t(), faces, normals, cell=cell)
    with pytest.raises(ValueError, match="normals"):
        ops.mesh_simplify(verts, faces, normals[:-1], cell=cell)
    with pytest.raises(ValueError, match="normals"):
        ops.mesh_simplify(verts, faces, normals.double(), cell=cell)


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("sparse", [False, True])
def test_high_res_mesh_simplify(sparse, largest, monkeypatch):
    c1, r1 = torch.tensor([-0.1, 0.0, 0.0], device="cuda"), 0.45
    c2, r2 = torch.tensor([0.55, 0.25, 0.1], device="cuda"), 0.12    # inside the aligned lattice's 0.2 margin

    def two_spheres(x):
        return torch.minimum((x - c1).norm(dim=1) - r1, (x - c2).norm(dim=1) - r2)

    cells = []
    op = ops.mesh_simplify

    def spy(*args, **kwargs):
        cells.append(kwargs["cell"])
        return op(*args, **kwargs)

    monkeypatch.setattr(ops, "mesh_simplify", spy)
    today = get_surface_high_res_mesh(two_spheres, 64, sparse=sparse, largest_component=largest)
    plain = get_surface_high_res_mesh(two_spheres, 64, sparse=sparse, largest_component=largest, simplify=None)
    assert not cells
    for a, b in ((today.vertices, plain.vertices), (today.faces, plain.faces),
                 (today.vertex_normals, plain.vertex_normals)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    small = get_surface_high_res_mesh(two_spheres, 64, sparse=sparse, largest_component=largest, simplify=2)
    assert len(cells) == 1
    # the cell is twice the fine lattice spacing d: every marching-cubes triangle lies inside one lattice cube, so its
    # edges are at most sqrt(3) d long, and a sphere's mesh has edges longer than d (the diagonals of cut cube faces)
    edge = plain.vertices[plain.faces] - plain.vertices[np.roll(plain.faces, 1, axis=1)]
    longest = float(np.linalg.norm(edge, axis=2).max())
    assert longest / math.sqrt(3.0) * (1.0 - 1e-5) <= cells[0] / 2.0 <= longest
    verts = plain.vertices.astype(np.float32)
    assert np.array_equal(verts.astype(np.float64), plain.vertices)
    ref = S.simplify(verts, plain.faces, plain.vertex_normals.astype(np.float32), cells[0])
    assert 0 < len(ref["faces"]) < len(plain.faces) // 2
    assert small.vertices.dtype == np.float64 and small.faces.dtype == np.int64
    assert np.array_equal(small.faces, ref["faces"])
    assert small.vertices.shape == ref["verts"].shape
    assert np.all(np.abs(small.vertices - ref["verts"]) <= ULP2 * float(np.abs(verts).max()))
    assert ref["normal_ratio"].min() >= MIN_NORMAL_RATIO
    assert np.all(np.abs(small.vertex_normals - ref["normals"]) <= ULP2)
    if largest:
        assert len(small.split(only_watertight=False)) == 1
