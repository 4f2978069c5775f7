"""ops.marching_cubes_sparse (csrc/hm_mesh_sparse.hip): the brick-sparse extraction gives ops.marching_cubes of the
fully evaluated lattice bit for bit while it evaluates only the bricks near the surface.

"Equal to dense": the volume is sdf(lattice_points of every index), through the same sdf and the same point generator;
verts, faces and normals of ops.marching_cubes on it are torch.equal to the sparse outputs."""
import functools

import numpy as np
import pytest
import torch

import mc_ref as M
from hashmodnffbanks_idr_amd import ops
from hashmodnffbanks_idr_amd._lib import HashmodError
from hashmodnffbanks_idr_amd.utils.plots import TriMesh, get_surface_high_res_mesh, lattice_points
from helpers import make_implicit

pytestmark = pytest.mark.gpu


def _axes(shape, lo=-1.0, hi=1.0):
    return [np.linspace(lo, hi, n) for n in shape]


def _spacing(axes):
    return tuple(float(a[1] - a[0]) for a in axes)


def _dist(x, c):
    # elementwise only: a point's value cannot depend on the batch it is evaluated in
    return torch.sqrt((x[:, 0] - c[0]) ** 2 + (x[:, 1] - c[1]) ** 2 + (x[:, 2] - c[2]) ** 2)


def _sphere(r, c=(0.0, 0.0, 0.0)):
    return lambda x: _dist(x, c) - r


def _torus(x):      # tests/test_mesh_gpu.py::_torus
    return torch.sqrt((torch.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2) - 0.55) ** 2 + x[:, 2] ** 2) - 0.25


def _dense(sdf, axes, level=0.0, rot=None, shift=None):
    shape = tuple(len(a) for a in axes)
    q = torch.arange(shape[0] * shape[1] * shape[2], dtype=torch.int64, device="cuda")
    volume = sdf(lattice_points(axes, q, rot, shift)).view(shape)
    return ops.marching_cubes(volume, level, _spacing(axes))


def _assert_equal(sparse, dense):
    assert dense[1].shape[0] > 0
    for name, s, d in zip(("verts", "faces", "normals"), sparse, dense):
        assert s.dtype == d.dtype and s.shape == d.shape, name
        assert torch.equal(s, d), name


def _check_equal_to_dense(sdf, shape, seeds, level=0.0, **kw):
    axes = _axes(shape)
    out = ops.marching_cubes_sparse(sdf, axes, _spacing(axes), seeds, level, return_stats=True, **kw)
    _assert_equal(out[:3], _dense(sdf, axes, level))
    return out


# ---- 1. shapes: no dimension is a multiple of the brick size, one seed on the surface ---------------------
SHAPES = {
    "sphere_61x77x45": (_sphere(0.6), (61, 77, 45), [[0.6, 0.0, 0.0]], 0.0),
    "torus_72x80x56": (_torus, (72, 80, 56), [[0.8, 0.0, 0.0]], 0.0),
    "sphere_level_0.15": (_sphere(0.6), (61, 77, 45), [[0.75, 0.0, 0.0]], 0.15),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_equal_dense_and_closed(name):
    sdf, shape, seeds, level = SHAPES[name]
    verts, faces, normals, stats = _check_equal_to_dense(sdf, shape, seeds, level)
    assert M.edge_check(faces.cpu().numpy()) == (True, True)


# ---- 2. the surface lies between two bricks: every brick's own points have one sign ------------------------
def test_surface_between_bricks():
    shape = (40, 48, 56)
    x = torch.as_tensor(_axes(shape)[0], dtype=torch.float32)
    mid = float((x[7] + x[8]) / 2)
    _check_equal_to_dense(lambda p: p[:, 0] - mid, shape, [[mid, 0.0, 0.0]])


# ---- 3. cut by the lattice border ---------------------------------------------------------------------
def test_cut_by_the_lattice_border():
    verts, faces, _, _ = _check_equal_to_dense(_sphere(0.9, (0.8, -0.5, 0.3)), (48, 40, 56), [[-0.1, -0.5, 0.3]])
    assert M.edge_check(faces.cpu().numpy())[0] is False      # open at the border, as the dense mesh


# ---- 4. exact zeros on lattice points -------------------------------------------------------------------
def test_exact_zeros_on_lattice_points():
    sdf = lambda p: p[:, 0].abs() + p[:, 1].abs() + p[:, 2].abs() - 0.5     # coordinates are multiples of 1/16
    axes = _axes((33, 33, 33))
    q = torch.arange(33 ** 3, device="cuda")
    assert int((sdf(lattice_points(axes, q)) == 0).sum()) > 100
    _check_equal_to_dense(sdf, (33, 33, 33), [[0.5, 0.0, 0.0]])


# ---- 5. two components ------------------------------------------------------------------------------------
# the second sphere starts less than a brick (8 * 2/63) beyond the first one, so it crosses bricks that are evaluated
# as the halo of the first one's surface bricks
CA, RA, CB, RB = (-0.45, 0.0, 0.0), 0.35, (0.36, 0.1, 0.0), 0.3
TWO_SHAPE = (64, 56, 48)


def _two_spheres(x):
    return torch.minimum(_dist(x, CA) - RA, _dist(x, CB) - RB)


@functools.lru_cache(maxsize=None)
def _two_dense():
    return _dense(_two_spheres, _axes(TWO_SHAPE))


def test_two_components_seeds_on_both():
    axes = _axes(TWO_SHAPE)
    seeds = [[CA[0] - RA, CA[1], CA[2]], [CB[0] + RB, CB[1], CB[2]]]
    _assert_equal(ops.marching_cubes_sparse(_two_spheres, axes, _spacing(axes), seeds), _two_dense())


def test_two_components_seed_on_one_gives_that_one_whole():
    axes = _axes(TWO_SHAPE)
    h = _spacing(axes)
    verts, faces, normals = ops.marching_cubes_sparse(_two_spheres, axes, h, [[CA[0] - RA, CA[1], CA[2]]])
    f = faces.cpu().numpy()
    assert M.edge_check(f) == (True, True)
    mesh = TriMesh(verts.cpu().numpy() - 1.0, f)
    assert len(mesh.split()) == 1
    on_a = np.abs(np.linalg.norm(mesh.vertices - np.array(CA), axis=1) - RA)
    assert on_a.max() <= 0.5 * np.sqrt(3.0) * max(h)
    dv, df, _ = _two_dense()
    parts = TriMesh(dv.cpu().numpy() - 1.0, df.cpu().numpy()).split()
    assert len(parts) == 2
    part_a = [p for p in parts if np.abs(np.linalg.norm(p.vertices - np.array(CA), axis=1) - RA).max() < 0.1]
    assert len(part_a) == 1 and len(f) == len(part_a[0].faces) and len(mesh.vertices) == len(part_a[0].vertices)


# ---- 6. rotation and shift, network SDF -------------------------------------------------------------------
def test_rotated_lattice_of_a_network_sdf():
    net = make_implicit("tiny", (64,) * 8, 16, 3, 0.1, 0.05, bias=0.6)
    sdf = lambda x: net.sdf(x, tile_points=64)       # at tile 64 a point's value does not depend on its batch
    g = torch.Generator().manual_seed(5)
    rot = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))[0].float().cuda()
    assert (rot.abs() > 0.05).all()
    shift = torch.tensor([0.04, -0.03, 0.05], device="cuda")
    axes = [np.linspace(-0.9, 0.9, n) for n in (48, 56, 40)]
    # the geometric initialisation is close to a sphere of radius 0.6 around the world origin
    world = 0.6 * torch.cat([torch.eye(3), -torch.eye(3)]).cuda()
    seeds = (world - shift) @ rot.T
    out = ops.marching_cubes_sparse(sdf, axes, _spacing(axes), seeds, 0.0, rot, shift, return_stats=True)
    _assert_equal(out[:3], _dense(sdf, axes, 0.0, rot, shift))
    assert out[0].shape[0] > 1000


# ---- 7. work done -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap", [(128, 0.35), (256, 0.18)])
def test_share_of_the_lattice_that_is_evaluated(n, cap):
    sdf = _sphere(0.6)
    axes = _axes((n, n, n))
    verts, faces, normals, stats = ops.marching_cubes_sparse(sdf, axes, _spacing(axes), [[0.6, 0.0, 0.0]],
                                                              return_stats=True)
    share = stats["points"] / n ** 3
    print(f"{n}^3: share {share:.4f}, {stats}")
    assert stats["lattice_points"] == n ** 3
    assert share <= cap
    assert stats["points"] == stats["bricks_evaluated"] * 512
    assert 0 < stats["surface_bricks"] < stats["bricks_evaluated"] and stats["rounds"] > 1
    dense = _dense(sdf, axes)
    if n == 128:
        _assert_equal((verts, faces, normals), dense)
    else:
        assert verts.shape == dense[0].shape and faces.shape == dense[1].shape and faces.shape[0] > 0


def test_batches_of_at_most_chunk_points():
    sizes = []

    def sdf(x):
        sizes.append(x.shape[0])
        return _sphere(0.6)(x)

    axes = _axes((61, 77, 45))
    out = ops.marching_cubes_sparse(sdf, axes, _spacing(axes), [[0.6, 0.0, 0.0]], chunk=4096, return_stats=True)
    assert max(sizes) <= 4096 and sum(sizes) == out[3]["points"] and len(sizes) == out[3]["sdf_calls"]
    _assert_equal(out[:3], _dense(_sphere(0.6), axes))


def test_lattice_of_more_than_2_31_points():
    """1400^3 = 2.74e9 lattice points; the sphere lies where every linear index is above 2^31 (i >= 1297), so a key or
    an index narrowed to 32 bits scrambles the order.  The reference is the dense call on the brick-aligned corner
    [1120:, 1120:, 1120:] of the same lattice: the same values, so faces and normals are equal bit for bit (cropping keeps
    the order of points and cells), and the vertices differ by the crop's offset up to rounding."""
    n, lo = 1400, 1120
    axes = _axes((n, n, n))
    h = _spacing(axes)
    sdf = _sphere(0.045, (0.9, 0.9, 0.9))
    verts, faces, normals, stats = ops.marching_cubes_sparse(sdf, axes, h, [[0.945, 0.9, 0.9]], return_stats=True)
    assert stats["lattice_points"] == n ** 3 > 1 << 31 and stats["points"] < 2e6
    crop = [a[lo:] for a in axes]
    dv, df, dn = _dense(sdf, crop)
    assert df.shape[0] > 10000 and M.edge_check(df.cpu().numpy()) == (True, True)
    assert torch.equal(faces, df) and torch.equal(normals, dn)
    assert float(verts.min()) > 1297 * h[0]
    # (fp32(i) + t) * h: half an ulp of 1400 times h = 8.7e-8, then half an ulp of 2 = 1.2e-7, on both sides
    err = (verts.double() - (dv.double() + lo * torch.tensor(h, dtype=torch.float64, device="cuda"))).abs().max()
    assert float(err) <= 2 * (8.7e-8 + 1.2e-7)


# ---- 8. edge cases ----------------------------------------------------------------------------------------
def test_empty_nan_and_repeatability():
    axes = _axes((40, 40, 40))
    h = _spacing(axes)
    far = [[0.95, 0.95, 0.95], [3.0, 0.0, 0.0], [float("nan"), 0.0, 0.0]]      # the last two: outside the lattice
    v, f, n, stats = ops.marching_cubes_sparse(_sphere(0.3), axes, h, far, return_stats=True)
    e = ops.marching_cubes(torch.ones(9, 7, 5, device="cuda"))
    for a, b in zip((v, f, n), e):
        assert a.shape == b.shape == (0, 3) and a.dtype == b.dtype and a.is_cuda
    assert stats["surface_bricks"] == 0 and stats["bricks_evaluated"] <= 64
    v, f, n = ops.marching_cubes_sparse(_sphere(0.3), axes, h, torch.zeros(0, 3))
    assert v.shape == f.shape == n.shape == (0, 3)

    def with_nan(x):
        s = _sphere(0.6)(x)
        return torch.where((x[:, 0] < -0.5) & (x[:, 1].abs() < 0.03) & (x[:, 2].abs() < 0.03), float("nan"), s)

    with pytest.raises(HashmodError, match="NaN"):
        ops.marching_cubes_sparse(with_nan, axes, h, [[0.6, 0.0, 0.0]])

    a = ops.marching_cubes_sparse(_torus, axes, h, [[0.8, 0.0, 0.0]])
    b = ops.marching_cubes_sparse(_torus, axes, h, [[0.8, 0.0, 0.0]])
    assert a[1].shape[0] > 1000
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_lattice_points_is_the_indexed_lattice():
    axes = [np.linspace(-1.0, 1.0, 9), np.linspace(0.0, 3.0, 7), np.linspace(-2.0, 0.5, 5)]
    q = torch.tensor([0, 1, 5, 7 * 5, 9 * 7 * 5 - 1, 123], device="cuda")
    p = lattice_points(axes, q)
    i, j, k = q // 35, q // 5 % 7, q % 5
    ref = torch.stack([torch.as_tensor(a, dtype=torch.float32).cuda()[t] for a, t in zip(axes, (i, j, k))], dim=1)
    assert torch.equal(p, ref)
    rot = torch.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], device="cuda")   # a permutation: exact
    shift = torch.tensor([0.5, -1.0, 2.0], device="cuda")
    assert torch.equal(lattice_points(axes, q, rot, shift), ref[:, [2, 0, 1]] + shift)
    assert torch.isnan(lattice_points(axes, torch.tensor([-1, 9 * 7 * 5], device="cuda"))).all()


# ---- 9. get_surface_high_res_mesh(sparse=True) ------------------------------------------------------------
def test_high_res_mesh_sparse_keeps_the_larger_sphere():
    c1, r1 = torch.tensor([-0.35, 0.1, 0.0], device="cuda"), 0.45
    c2, r2 = torch.tensor([0.75, -0.7, 0.7], device="cuda"), 0.15

    def two_spheres(x):     # tests/test_mesh_gpu.py::test_high_res_mesh_keeps_the_larger_sphere_and_exports
        return torch.minimum((x - c1).norm(dim=1) - r1, (x - c2).norm(dim=1) - r2)

    mesh = get_surface_high_res_mesh(two_spheres, 80, sparse=True)
    assert mesh is not None
    assert len(mesh.split()) == 1 and mesh.is_watertight
    dist = np.linalg.norm(mesh.vertices - c1.cpu().numpy(), axis=1)
    assert np.abs(dist - r1).max() < 0.01
    radial = (mesh.vertices - c1.cpu().numpy()) / dist[:, None]
    assert np.einsum("ij,ij->i", mesh.vertex_normals, radial).min() > 0.99
    dense = get_surface_high_res_mesh(two_spheres, 80)
    assert mesh.area == pytest.approx(dense.area, rel=1e-4)
    assert get_surface_high_res_mesh(lambda x: x.norm(dim=1) + 1.0, 32, sparse=True) is None
