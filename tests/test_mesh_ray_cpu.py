"""CPU-side checks of the mesh ray cast: the numpy restatement of the definition (tests/mesh_ray_cases.py, the
reference of csrc/hm_mesh_ray.hip) against the slab walk the kernel performs and against itself in fp64, the claims
the cases make, and the argument checks of the new ops, which run before the library is touched."""
import math

import numpy as np
import pytest
import torch

import mesh_ray_cases as RC
import nn_cases as NC

CELL_IDS = ["default", "one_cell", "fine"]
PAD_IDS = ["pad0", "default_pad", "eighth"]


# ---- the walk against the brute force -----------------------------------------------------------------------
@pytest.mark.parametrize("which_pad", range(3), ids=PAD_IDS)
@pytest.mark.parametrize("name", RC.CASES)
def test_walk_equals_brute_force(name, which_pad):
    v, f, o, d, t_min, t_max = RC.case(name)
    t, face, _, _ = RC.reference(name, which_pad)
    pad = RC.pads(v)[which_pad]
    early = 0
    for cell in RC.cells(v):
        stats = {}
        wt, wf = RC.walk_ref(o, d, RC.GridIndex(v, f, cell, pad), t_min, t_max, stats)
        assert np.array_equal(wt.view(np.int32), t.view(np.int32)), f"t bits differ (cell {cell}, pad {pad})"
        assert np.array_equal(wf, face), f"face differs (cell {cell}, pad {pad})"
        early += stats["early_stops"]
    if name in ("icosphere2", "rays_1000"):
        assert early > 0                      # the stopping rule is exercised, not only the end of the range


def test_the_cases_cover_what_they_claim():
    for name in ("icosphere2", "soup_257", "planar", "big_among_small"):
        v, f, o, d, t_min, t_max = RC.case(name)
        assert len(o) == 344 + (6 if name == "planar" else 0)
        t, face, uv, point = RC.reference(name, 1)
        hit = face >= 0
        assert 0.3 < hit.mean() < 1.0
        assert np.isinf(t[~hit]).all() and np.isnan(uv[~hit]).all() and np.isnan(point[~hit]).all()
        assert (np.abs(d).max(1) == 0).sum() == 4 and not hit[np.abs(d).max(1) == 0].any()
        assert (t_max == 1).sum() == 64 and (t_min > 0).sum() == 20
        length = np.linalg.norm(d.astype(np.float64), axis=1)
        assert ((length > 0) & (length < 2e-3)).sum() >= 20 and (length > 5e2).sum() >= 20
        axis_parallel = (d != 0).sum(1) == 1
        assert axis_parallel.sum() >= 36
        if name == "icosphere2":
            # a closed mesh: the segments end near the surface, so some reach it and some do not; t_min past the first
            # hit finds the far side where the aim was at the near one; rays start on the mesh
            seg = t_max == 1
            assert 0 < hit[seg].sum() < seg.sum()
            late = (t_min > 0) & hit
            first = RC.ray_ref(o[late], d[late], v, f, RC.pads(v)[1])[0]
            assert late.sum() >= 3 and (t[late] >= t_min[late]).all() and (first < t_min[late]).all()
            assert (t[hit] == 0).any() or (np.abs(t[hit]) < 1e-6).any()
            assert hit[axis_parallel].sum() >= 30


# ---- fp32 against fp64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [2, 3])
def test_fp32_restatement_against_fp64(level):
    """|t32 - t64| <= 8 * 2^-24 * max(M, t) / |cos incidence| for outside origins and unit directions, and the same
    hit masks.  The figure says nothing about the kernel, which is tested bit for bit against the fp32 restatement."""
    v, f = NC.icosphere(level)
    rng = np.random.default_rng(17 + level)
    m = 3000
    o = NC._f4(3.0 * RC._unit(rng, m))
    w = RC._unit(rng, m) * rng.random((m, 1)) ** (1 / 3) * 0.95 - o
    d = NC._f4(w / np.linalg.norm(w, axis=1, keepdims=True))
    pad = RC.default_pad(v)
    t32, f32, _, _ = RC.ray_ref(o, d, v, f, pad)
    t64, f64, _, _ = RC.ray_ref(o, d, v, f, pad, dtype=np.float64)
    assert t32.dtype == np.float32 and t64.dtype == np.float64
    assert np.array_equal(f32 >= 0, f64 >= 0) and (f64 >= 0).mean() > 0.9
    hit = f64 >= 0
    tri = v.astype(np.float64)[f[f64[hit]]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    d64 = d.astype(np.float64)[hit]
    cos = np.abs((n * d64).sum(1)) / (np.linalg.norm(n, axis=1) * np.linalg.norm(d64, axis=1))
    M = max(float(np.abs(v).max()), float(np.abs(o).max()))
    unit = 2.0 ** -24 * np.maximum(M, t64[hit]) / cos
    err = np.abs(t32[hit].astype(np.float64) - t64[hit]) / unit
    print(f"icosphere({level}): max |t32 - t64| = {err.max():.3f} units of 2^-24 max(M, t) / |cos|")
    assert err.max() <= 8.0


# ---- planar values and ties ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which_pad", [0, 1], ids=PAD_IDS[:2])
def test_planar_values_and_ties(which_pad):
    v, f, o, d, t_min, t_max = RC.case("planar")
    k = len(RC.PLANAR_RAYS)
    t, face, uv, point = (x[:k] for x in RC.reference("planar", which_pad))
    hitters = RC.n_hitters(o[:k], d[:k], v, f, RC.pads(v)[which_pad])
    assert t.tolist() == [r[2] for r in RC.PLANAR_RAYS]
    assert hitters.tolist() == [r[3] for r in RC.PLANAR_RAYS]
    assert [a for a, r in zip(face.tolist(), RC.PLANAR_RAYS) if r[4] is not None] == [12, 23, 25, 0, -1]
    assert (point[face >= 0, 2] == 0).all()


@pytest.mark.parametrize("name", ["icosphere1", "icosphere2", "planar", "big_among_small"])
def test_lowest_face_wins(name):
    v, f, o, d, t_min, t_max = RC.case(name)
    pad = RC.pads(v)[1]
    t, face, _, _ = RC.reference(name, 1)
    tri = v[f]
    tt = RC.face_values(o[:, None, :], d[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], pad,
                        t_min[:, None], t_max[:, None])[0]
    hit = face >= 0
    at = tt[hit] == t[hit, None]
    assert (face[hit] == at.argmax(1)).all() and at[np.arange(hit.sum()), face[hit]].all()
    ties = RC.n_hitters(o, d, v, f, pad, t_min, t_max)
    assert np.array_equal(ties > 0, hit)
    if name != "big_among_small":
        assert (ties > 1).any()               # rays at vertices and edge midpoints exercise the tie rule


# ---- closed meshes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [2, 3])
def test_closed_mesh_leaks(level):
    """rays from outside through a random interior point of a closed icosphere: the share of misses is at most 1e-3
    (no watertightness is claimed; 0 were seen)"""
    v, f = NC.icosphere(level)
    rng = np.random.default_rng(23 + level)
    m = 20000
    r_in = RC.inner_radius(v, f)
    o = 3.0 * RC._unit(rng, m)
    through = RC._unit(rng, m) * rng.random((m, 1)) ** (1 / 3) * (0.98 * r_in)
    w = through - o
    t, face, _, _ = RC.ray_ref(NC._f4(o), NC._f4(w / np.linalg.norm(w, axis=1, keepdims=True)), v, f, RC.default_pad(v))
    misses = int((face < 0).sum())
    print(f"icosphere({level}): {misses} misses of {m}")
    assert misses <= 1e-3 * m


# ---- the argument checks ------------------------------------------------------------------------------------
def test_argument_checks():
    """ValueError before the library is touched: there is no GPU here, and no call below reaches one"""
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd.evaluation import cast_camera_rays, depth_agreement
    v, f = (torch.from_numpy(np.array(a)) for a in RC.case("single")[:2])
    o, d = torch.zeros(5, 3), torch.ones(5, 3)
    meta = dict(device="meta")
    vm, fm = torch.zeros(3, 3, **meta), torch.zeros(1, 3, dtype=torch.int32, **meta)
    om, dm = torch.zeros(5, 3, **meta), torch.zeros(5, 3, **meta)
    for bad in (o.double(), torch.zeros(5, 4), torch.zeros(3, 8).t(), torch.zeros(8), None):
        with pytest.raises(ValueError):
            ops.mesh_ray_cast(bad, d, v, f)
        with pytest.raises(ValueError):
            ops.mesh_ray_cast(o, bad, v, f)
        with pytest.raises(ValueError):
            ops.mesh_ray_cast(om, dm, bad, fm, pad=0.0)
        with pytest.raises(ValueError):
            ops.mesh_ray_pad(bad)
    with pytest.raises(ValueError, match="same number"):
        ops.mesh_ray_cast(om, torch.zeros(4, 3, **meta), vm, fm)
    with pytest.raises(ValueError, match="GPU"):
        ops.mesh_ray_cast(o, d, v, f)
    with pytest.raises(ValueError, match="GPU"):
        ops.mesh_ray_cast(o, d, v, f, pad=0.01)
    with pytest.raises(ValueError, match="GPU"):
        ops.mesh_index(v, f, pad=0.01)
    for pad in (-1.0, float("nan"), float("inf"), "1", True, 1e39):
        with pytest.raises(ValueError, match="pad"):
            ops.mesh_index(vm, fm, pad=pad)
        with pytest.raises(ValueError, match="pad"):
            ops.mesh_ray_cast(om, dm, vm, fm, pad=pad)
    with pytest.raises(ValueError, match="pad"):
        ops.mesh_index(vm, fm, pad=None)
    for name in ("t_min", "t_max"):
        for bad in (float("nan"), "1", None, True, torch.zeros(4, **meta), torch.zeros(5, 1, **meta),
                    torch.zeros(5, dtype=torch.float64, **meta), torch.zeros(10, **meta)[::2]):
            with pytest.raises(ValueError, match=name):
                ops.mesh_ray_cast(om, dm, vm, fm, **{name: bad})
    with pytest.raises(ValueError, match="t_min"):
        ops.mesh_ray_cast(om, dm, vm, fm, t_min=-math.inf)
    for flag in (1, None, "yes"):
        with pytest.raises(ValueError, match="return_uv"):
            ops.mesh_ray_cast(om, dm, vm, fm, return_uv=flag)
        with pytest.raises(ValueError, match="return_point"):
            ops.mesh_ray_cast(om, dm, vm, fm, return_point=flag)
    for cell in (0, -1.0, float("nan"), "1", True):
        with pytest.raises(ValueError, match="cell"):
            ops.mesh_ray_cast(om, dm, vm, fm, cell=cell)
    for big_face in (0, 1.5, None, True):
        with pytest.raises(ValueError, match="big_face"):
            ops.mesh_ray_cast(om, dm, vm, fm, big_face=big_face)
    # the default pad is fp32(2^-12 * the largest extent) and needs no GPU
    assert ops.mesh_ray_pad(v) == float(RC.default_pad(v.numpy())) > 0
    # the evaluation entry points
    uv, pose, K = torch.zeros(1, 4, 2), torch.eye(4)[None], torch.eye(4)[None]
    with pytest.raises(ValueError, match="mesh"):
        cast_camera_rays("mesh.ply", uv, pose, K)
    for radius in (0, -1.0, float("nan"), "1"):
        with pytest.raises(ValueError, match="radius"):
            cast_camera_rays((vm, fm), uv, pose, K, radius=radius)
    with pytest.raises(ValueError, match="uv"):
        cast_camera_rays((vm, fm), torch.zeros(4, 2), pose, K)
    with pytest.raises(ValueError, match="pose"):
        cast_camera_rays((vm, fm), uv, torch.eye(4), K)
    t, hit = torch.zeros(2, 3, **meta), torch.zeros(2, 3, dtype=torch.bool, **meta)
    with pytest.raises(ValueError, match="shape"):
        depth_agreement(t, hit, torch.zeros(2, 4, **meta), hit)
    with pytest.raises(ValueError, match="bool"):
        depth_agreement(t, hit.float(), t, hit)
    with pytest.raises(ValueError, match="GPU"):
        depth_agreement(torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.bool), torch.zeros(2, 3),
                        torch.zeros(2, 3, dtype=torch.bool))
