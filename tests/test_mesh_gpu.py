"""ops.marching_cubes (csrc/hm_mesh.hip) against the numpy reference tests/mc_ref.py, and the reference's mesh
procedure utils/plots.get_surface_high_res_mesh on top of it."""
import numpy as np
import pytest
import torch

import mc_ref as M
from hashmodnffbanks_idr_amd import ops
from helpers import make_implicit

pytestmark = pytest.mark.gpu


def _lattice(shape, lo=-1.0, hi=1.0):
    axes = [np.linspace(lo, hi, n) for n in shape]
    return np.meshgrid(*axes, indexing="ij"), [a[1] - a[0] for a in axes]


def _sphere(shape=(64, 64, 64), r=0.6, c=(0.0, 0.0, 0.0)):
    (X, Y, Z), h = _lattice(shape)
    return (np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r).astype(np.float32), h


def _torus(shape=(64, 64, 64)):
    (X, Y, Z), h = _lattice(shape)
    return (np.sqrt((np.sqrt(X ** 2 + Y ** 2) - 0.55) ** 2 + Z ** 2) - 0.25).astype(np.float32), h


def _noise(shape, seed):
    v = np.ones(shape, np.float32)
    v[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed).standard_normal([s - 2 for s in shape]).astype(np.float32)
    return v, (1.0, 1.0, 1.0)


def _one_corner():
    v = np.ones((2, 2, 2), np.float32)
    v[0, 0, 0] = -1.0
    return v, (1.0, 1.0, 1.0)


CASES = {
    "sphere": lambda: (*_sphere(), 0.0),
    "torus": lambda: (*_torus(), 0.0),
    "noise": lambda: (*_noise((40, 40, 40), 1), 0.0),
    "noncubic_17x33x9": lambda: (*_noise((17, 33, 9), 2), 0.0),
    "sphere_noncubic_17x33x9": lambda: (*_sphere((17, 33, 9), 0.7), 0.0),
    "level_0.15": lambda: (*_sphere(), 0.15),
    "noise_level_-0.3": lambda: (*_noise((24, 20, 28), 3), -0.3),
    "cut_by_border": lambda: (*_sphere((48, 40, 56), 0.9, (0.8, -0.5, 0.3)), 0.0),
    # the edges of a workgroup block (16 rounds of 256 points): exactly one block; a second block that breaks off after
    # two rounds, the second one partial (4352 points); the smallest legal volume, one cell and one triangle
    "one_block_16x16x16": lambda: (*_noise((16, 16, 16), 4), 0.0),
    "block_and_partial_round_17x16x16": lambda: (*_noise((17, 16, 16), 5), 0.0),
    "one_cell_2x2x2": lambda: (*_one_corner(), 0.0),
}
OPEN = ("cut_by_border", "one_cell_2x2x2")   # surfaces that end at the volume's border


def _check_against_ref(vol, spacing, level):
    rv, rf, rn = M.marching_cubes(vol, level, spacing)
    v, f, n = ops.marching_cubes(torch.from_numpy(vol).cuda(), level, spacing)
    assert v.shape == rv.shape and n.shape == rn.shape and f.shape == rf.shape
    assert f.dtype == torch.int32
    assert torch.equal(f.cpu(), torch.from_numpy(rf.astype(np.int32)))
    assert np.abs(v.cpu().numpy() - rv).max() <= 1e-5
    assert np.abs(n.cpu().numpy() - rn).max() <= 1e-5
    return rv, rf


@pytest.mark.parametrize("name", list(CASES))
def test_marching_cubes_matches_reference(name):
    vol, spacing, level = CASES[name]()
    rv, rf = _check_against_ref(vol, spacing, level)
    assert len(rf) > 0
    if name not in OPEN:
        assert M.edge_check(rf) == (True, True)


def test_strided_volume_equals_contiguous_copy():
    from hashmodnffbanks_idr_amd.utils.plots import get_grid_uniform
    grid = get_grid_uniform(50, "cuda")
    p = grid["grid_points"]
    z = (p.norm(dim=1) - 0.55 + 0.05 * torch.sin(7 * p[:, 0]) * torch.cos(5 * p[:, 1])).contiguous()
    view = z.view(50, 50, 50).permute(1, 0, 2)                    # sdf_volume's transpose, no copy
    assert not view.is_contiguous()
    d = float(grid["xyz"][0][1] - grid["xyz"][0][0])
    a = ops.marching_cubes(view, 0.0, (d, d, d))
    b = ops.marching_cubes(view.contiguous(), 0.0, (d, d, d))
    assert a[0].shape[0] > 1000
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # reproducible: a second call gives the same bits
    c = ops.marching_cubes(view, 0.0, (d, d, d))
    for x, y in zip(a, c):
        assert torch.equal(x, y)
    _check_against_ref(view.cpu().numpy(), (d, d, d), 0.0)


def test_empty_nan_and_cpu_volumes():
    from hashmodnffbanks_idr_amd._lib import HashmodError
    v, f, n = ops.marching_cubes(torch.ones(9, 7, 5, device="cuda"))
    assert v.shape == (0, 3) and n.shape == (0, 3) and f.shape == (0, 3) and v.is_cuda and f.dtype == torch.int32
    vol = torch.from_numpy(_sphere((16, 16, 16))[0]).cuda()
    vol[3, 4, 5] = float("nan")
    with pytest.raises(HashmodError, match="NaN"):
        ops.marching_cubes(vol)
    with pytest.raises(HashmodError):
        ops.marching_cubes(torch.zeros(4, 4, 4))
    with pytest.raises(ValueError, match=">= 2"):
        ops.marching_cubes(torch.zeros(1, 4, 4, device="cuda"))


def test_high_res_mesh_of_a_geometric_init_network():
    from hashmodnffbanks_idr_amd.utils.plots import get_surface_high_res_mesh
    net = make_implicit("tiny", (64,) * 8, 16, 3, 0.1, 0.05, bias=0.6)
    res = 64
    mesh = get_surface_high_res_mesh(lambda x: net.sdf(x), res)
    assert mesh is not None and len(mesh.faces) > 1000
    assert np.abs(mesh.vertices).max() < 1.0
    assert M.edge_check(mesh.faces) == (True, True) and mesh.is_watertight
    assert len(mesh.split(only_watertight=False)) == 1
    assert M.signed_volume(mesh.vertices, mesh.faces) > 0
    # cell size of the aligned grid: (shortest extent + 2 * 0.2) / (res - 1) <= (largest extent + 0.4) / (res - 1)
    h = (np.ptp(mesh.vertices, axis=0).max() + 0.4) / (res - 1)
    s = net.sdf(torch.from_numpy(mesh.vertices).float().cuda()).cpu().numpy()
    assert np.abs(s).max() <= 0.5 * np.sqrt(3.0) * h


def test_high_res_mesh_keeps_the_larger_sphere_and_exports(tmp_path):
    from hashmodnffbanks_idr_amd.utils.plots import get_surface_high_res_mesh
    c1, r1 = torch.tensor([-0.35, 0.1, 0.0], device="cuda"), 0.45
    c2, r2 = torch.tensor([0.75, -0.7, 0.7], device="cuda"), 0.15   # outside the aligned grid around the larger one

    def two_spheres(x):
        return torch.minimum((x - c1).norm(dim=1) - r1, (x - c2).norm(dim=1) - r2)

    mesh = get_surface_high_res_mesh(two_spheres, 80)
    assert mesh is not None
    assert len(mesh.split()) == 1 and mesh.is_watertight
    dist = np.linalg.norm(mesh.vertices - c1.cpu().numpy(), axis=1)
    assert np.abs(dist - r1).max() < 0.01
    assert mesh.area == pytest.approx(4 * np.pi * r1 ** 2, rel=0.01)
    # normals point outward of the kept sphere
    radial = (mesh.vertices - c1.cpu().numpy()) / dist[:, None]
    assert np.einsum("ij,ij->i", mesh.vertex_normals, radial).min() > 0.99
    assert get_surface_high_res_mesh(lambda x: x.norm(dim=1) + 1.0, 32) is None

    path = tmp_path / "mesh.ply"
    mesh.export(str(path))
    v, n, f = M.read_ply(str(path))
    assert np.array_equal(v, mesh.vertices.astype(np.float32))
    assert np.array_equal(n, mesh.vertex_normals.astype(np.float32))
    assert np.array_equal(f, mesh.faces.astype(np.int32))
