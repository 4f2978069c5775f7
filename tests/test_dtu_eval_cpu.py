"""The restatements and inputs of the DTU-evaluation tests have the properties the GPU tests rely on, the new entry
points check their arguments before they touch the library, and the library exports what _lib.py declares (runs
anywhere)."""
import ctypes as C

import numpy as np
import pytest
import torch

import dtu_cases as DC
import nn_cases as NC
from hashmodnffbanks_idr_amd import _lib, ops
from hashmodnffbanks_idr_amd.evaluation import dtu_chamfer, load_dtu_scan


def _sklearn_loop(points, radius):
    """the reference's code, literally (evaluation/dtu_eval), in index order"""
    from sklearn.neighbors import NearestNeighbors
    p = np.asarray(points, np.float64)
    nn = NearestNeighbors(n_neighbors=1, radius=radius, algorithm="kd_tree", n_jobs=1)
    nn.fit(p)
    dist, nb = nn.radius_neighbors(p, radius=radius, return_distance=True)
    mask = np.ones(len(p), dtype=np.bool_)
    for curr, idxs in enumerate(nb):
        if mask[curr]:
            mask[idxs] = 0
            mask[curr] = 1
    return mask, np.concatenate(dist)


@pytest.mark.parametrize("name,radius", [("uniform_4097_1000", 0.0835), ("clusters", 0.228), ("sphere_shuffled", 0.05),
                                         ("sphere_swept", 0.05)])
def test_downsample_ref_is_the_sklearn_loop(name, radius):
    p = DC.sphere(name.split("_", 1)[1]) if name.startswith("sphere_") else NC.cloud(name)[0]
    mask, dist = _sklearn_loop(p, radius)
    # no pair so close to the radius that fp32 rounding of d2 could decide differently from sklearn's fp64
    assert np.abs(dist / radius - 1.0).min() > 1e-6
    want = DC.reference(name, radius)
    assert np.array_equal(want, mask)
    assert 0 < want.sum() < len(p)


def test_downsample_ref_small_cases():
    assert DC.downsample_ref(np.zeros((1, 3)), 1.0).tolist() == [True]
    assert DC.downsample_ref(np.zeros((5, 3)), 1.0).tolist() == [True, False, False, False, False]
    pair = np.array([[0, 0, 0], [3, 4, 0]], np.float32)
    assert DC.downsample_ref(pair, 5.0).tolist() == [True, False]                 # d2 == radius2: a neighbour
    assert DC.downsample_ref(pair, float(np.nextafter(np.float32(5), np.float32(0)))).tolist() == [True, True]
    keep = DC.reference("lattice", 1.0)
    p = NC.lattice()
    assert np.array_equal(keep, p.sum(1) % 2 == 0)                                # the checkerboard
    assert DC.reference("lattice", float(np.nextafter(np.float32(1), np.float32(0)))).all()
    for name in ("line", "line_reversed"):
        keep = DC.reference(name, 1.0)
        assert keep.sum() == 513 and np.array_equal(keep, np.arange(1025) % 2 == 0)


def test_sphere_orders_are_the_same_points():
    a, b = DC.sphere("shuffled"), DC.sphere("swept")
    assert a.shape == (20000, 3) and np.array_equal(np.sort(a, 0), np.sort(b, 0)) and not np.array_equal(a, b)
    assert np.all(np.diff(np.floor((b[:, 2].astype(np.float64) + 1.0) / 0.02)) >= 0)


@pytest.mark.parametrize("name", sorted(DC.FLAG_CASES))
def test_flags_ref_at_the_boundaries(name):
    shape, bb, res, patch, plane = DC.FLAG_CASES[name]
    mask = DC.flag_volume(name)
    assert mask.shape == shape and 0 < mask.sum() < mask.size
    pts = DC.flag_boundary_points(name)
    f = DC.flags_ref(pts, np.ones_like(mask), bb, res, patch, plane)
    per_axis = 15
    for a in range(3):
        lo_in, lo_out, hi_out, hi_in, h0, h1, h2, m0, m1, m2, top_half, top, last, far, nfar = f[a * per_axis:
                                                                                                 (a + 1) * per_axis]
        assert lo_in & 1 and not lo_out & 1 and not hi_out & 1 and hi_in & 1
        assert h0 & 2 and h1 & 2 and h2 & 2 and m0 & 2 and not m1 & 2 and not m2 & 2
        assert bool(top_half & 2) == ((shape[a] - 1) % 2 == 0) and not top & 2 and last & 2
        assert far & 3 == 0 and nfar & 3 == 0
    zero, above, below = f[3 * per_axis:3 * per_axis + 3]
    assert not zero & 4 and above & 4 and not below & 4
    assert np.all(f[-3:] == 0)
    # the voxel the half-way points round to: half to even
    only = np.zeros(shape, np.uint8)
    only[2, :, :] = 1
    g = DC.flags_ref(pts[:per_axis], only, bb, res, patch, plane)
    assert not g[4] & 2 and g[5] & 2 and g[6] & 2                                  # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    for n in (1, 255, 256, 257):
        assert DC.flag_points(name, n).shape == (n, 3)
    assert len(set(DC.flags_ref(DC.flag_points(name, 257), mask, bb, res, patch, plane).tolist())) >= 6


def test_arguments_are_checked_before_the_library():
    p = torch.zeros(8, 3)
    f = torch.zeros(2, 3, dtype=torch.int32)
    mask = torch.ones((2, 2, 2), dtype=torch.uint8)
    scan = dict(obs_mask=mask, bb=[[0, 0, 0], [1, 1, 1]], res=1.0, plane=[0, 0, 1, 0])
    for bad in (p.double(), torch.zeros(8, 4), torch.zeros(3, 8).t(), torch.zeros(8), None):
        with pytest.raises(ValueError):
            ops.radius_downsample(bad, 1.0)
        with pytest.raises(ValueError):
            ops.dtu_point_flags(bad, mask, scan["bb"], 1.0, 1.0, scan["plane"])
        with pytest.raises(ValueError):
            ops.one_sided_distance(bad, p)
        with pytest.raises(ValueError):
            ops.one_sided_distance(p, bad)
        with pytest.raises(ValueError):
            dtu_chamfer((p, f), bad, **scan)
    for radius in (0, -1.0, float("nan"), float("inf"), 1e-60, "1"):
        with pytest.raises(ValueError, match="radius"):
            ops.radius_downsample(p, radius)
    for cell in (0, float("nan")):
        with pytest.raises(ValueError, match="cell"):
            ops.radius_downsample(p, 1.0, cell=cell)
    assert ops.radius_downsample(torch.zeros(0, 3), 1.0).shape == (0,)
    assert ops.radius_downsample(torch.zeros(0, 3), 1.0).dtype == torch.bool
    for bad_mask in (mask.float(), torch.ones((2, 2), dtype=torch.uint8), torch.ones((2, 2, 4), dtype=torch.uint8)[..., ::2],
                     torch.ones((0, 2, 2), dtype=torch.uint8), None):
        with pytest.raises(ValueError, match="obs_mask"):
            ops.dtu_point_flags(p, bad_mask, scan["bb"], 1.0, 1.0, scan["plane"])
        with pytest.raises(ValueError, match="obs_mask"):
            dtu_chamfer((p, f), p, **dict(scan, obs_mask=bad_mask))
    for bb in ([[0, 0, 0]], [[0, 0, 0], [1, 1, float("nan")]], "bb"):
        with pytest.raises(ValueError, match="bb"):
            ops.dtu_point_flags(p, mask, bb, 1.0, 1.0, scan["plane"])
    for res in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError, match="res"):
            ops.dtu_point_flags(p, mask, scan["bb"], res, 1.0, scan["plane"])
    with pytest.raises(ValueError, match="plane"):
        ops.dtu_point_flags(p, mask, scan["bb"], 1.0, 1.0, [0, 0, 1])
    with pytest.raises(ValueError, match="devices"):
        ops.dtu_point_flags(p, mask.to("meta"), scan["bb"], 1.0, 1.0, scan["plane"])
    with pytest.raises(ValueError, match="devices"):
        ops.one_sided_distance(p, torch.zeros(8, 3, device="meta"))
    for md in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_dist"):
            ops.one_sided_distance(p, p, max_dist=md)
        with pytest.raises(ValueError, match="max_dist"):
            dtu_chamfer((p, f), p, max_dist=md, **scan)
    for density in (0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="density"):
            dtu_chamfer((p, f), p, density=density, **scan)
    with pytest.raises(ValueError, match="mesh"):
        dtu_chamfer("mesh.ply", p, **scan)
    assert ops.one_sided_distance(torch.zeros(0, 3), p)[1] == 0 and np.isnan(ops.one_sided_distance(p, p[:0])[0])


def test_library_exports_the_new_symbols():
    L = _lib.lib()
    want = {
        "hm_nn_radius_workspace_bytes": (C.c_int64, 1),
        "hm_nn_radius_begin": (C.c_int, 5),
        "hm_nn_radius_rounds": (C.c_int, 15),
        "hm_nn_radius_finish": (C.c_int, 6),
        "hm_dtu_point_flags": (C.c_int, 7),
    }
    for name, (res, n_args) in want.items():
        assert name in _lib.SIGNATURES
        fn = getattr(L, name)
        assert fn.restype is res and len(fn.argtypes) == n_args == len(_lib.SIGNATURES[name][1])
    # host-side checks answer without a GPU
    assert L.hm_nn_radius_workspace_bytes(0) == 0
    n = 1000
    assert L.hm_nn_radius_workspace_bytes(n) >= n + 8 * n + 4 * 4
    assert L.hm_nn_radius_workspace_bytes(-1) < 0 and L.hm_nn_radius_workspace_bytes(1 << 31) < 0
    assert L.hm_nn_radius_begin(0, None, 0, None, None) == -1
    assert L.hm_dtu_point_flags(None, 0, None, (C.c_int64 * 3)(2, 2, 2), (C.c_double * 14)(*([0.0] * 14)), None,
                                None) == -1                                        # res == 0
    with open(_lib.LIB_PATH.replace("libhashmod.so", "../include/hashmod.h")) as fh:
        header = fh.read()
    for name in want:
        assert f"HM_API int{'64_t' if want[name][0] is C.c_int64 else ''} {name}(" in header


def test_load_dtu_scan_round_trip(tmp_path):
    from scipy.io import savemat
    rng = np.random.default_rng(0)
    mask = rng.random((4, 5, 6)) < 0.5
    bb = np.array([[-1.0, -2.0, -3.0], [4.0, 5.0, 6.0]])
    plane = np.array([[0.1, -0.2, 0.97, 3.5]])
    (tmp_path / "ObsMask").mkdir()
    savemat(tmp_path / "ObsMask" / "ObsMask24_10.mat", {"ObsMask": mask, "BB": bb, "Res": np.array([[0.5]])})
    savemat(tmp_path / "ObsMask" / "Plane24.mat", {"P": plane})
    for folder in (tmp_path, tmp_path / "ObsMask"):
        scan = load_dtu_scan(str(folder), 24)
        assert scan["obs_mask"].dtype == np.uint8 and scan["obs_mask"].flags.c_contiguous
        assert np.array_equal(scan["obs_mask"], mask.astype(np.uint8))
        assert np.array_equal(scan["bb"], bb) and scan["res"] == 0.5 and np.array_equal(scan["plane"], plane[0])
    with pytest.raises(FileNotFoundError, match="ObsMask25_10.mat"):
        load_dtu_scan(str(tmp_path), 25)
    # what load_dtu_scan returns is what dtu_point_flags takes
    ops._dtu_params("test", torch.from_numpy(scan["obs_mask"]), scan["bb"], scan["res"], 60, scan["plane"])


def test_dtu_case_uses_every_stage():
    c, r = DC.dtu_case(), DC.dtu_case_reference()
    print({k: v for k, v in r.items() if k not in ("d2s", "s2d")})
    assert 25000 < r["n_cloud"] < 35000 and len(c["stl"]) == 20000
    assert 0 < r["n_down"] < r["n_cloud"] and 0 < r["n_in"] < r["n_down"] and 0 < r["n_in_obs"] < r["n_in"]
    assert 0 < r["n_stl_above"] < len(c["stl"])
    assert 0 < r["n_d2s"] < r["n_in_obs"] and 0 < r["n_s2d"] < r["n_stl_above"]
    for d in (r["d2s"], r["s2d"]):
        assert np.abs(d / c["max_dist"] - 1).min() > 1e-6
