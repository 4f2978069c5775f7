"""The device mesh ray cast (csrc/hm_mesh_ray.hip) against its numpy restatement (tests/mesh_ray_cases.ray_ref): bit
for bit over every grid, big-face setting and pad, independent of batching and order, the range ends, the padded
index, the errors, and against the rasteriser and analytic spheres through the evaluation entry points."""
import functools
import math

import numpy as np
import pytest
import torch

import mesh_cull_cases as CC
import mesh_dist_cases as MC
import mesh_ray_cases as RC
import nn_cases as NC
from hashmodnffbanks_idr_amd import ops
from hashmodnffbanks_idr_amd._lib import HashmodError
from hashmodnffbanks_idr_amd.evaluation import cast_camera_rays, depth_agreement

pytestmark = pytest.mark.gpu

CELL_IDS = ["default", "one_cell", "fine"]
PAD_IDS = ["pad0", "default_pad", "eighth"]


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # a copy: the shared inputs are read-only


def _big(big_face):
    return ops.MESH_DIST_BIG_FACE if big_face is None else big_face


def _check(got, want, what=""):
    """t, face, uv, point torch.equal to the reference (the NaNs of a missed ray compared as NaN)"""
    t, face, uv, point = got
    assert t.dtype == torch.float32 and face.dtype == torch.int32
    assert uv.dtype == torch.float32 and point.dtype == torch.float32
    assert torch.equal(face.cpu(), torch.from_numpy(want[1].copy())), f"face differs from the brute force {what}"
    assert torch.equal(t.cpu(), torch.from_numpy(want[0].copy())), f"t differs from the brute force {what}"
    miss = want[1] < 0
    got_uv, got_p = uv.cpu().numpy(), point.cpu().numpy()
    assert np.isinf(want[0][miss]).all() and np.isnan(got_uv[miss]).all() and np.isnan(got_p[miss]).all(), what
    assert torch.equal(torch.from_numpy(got_uv[~miss]), torch.from_numpy(want[2][~miss])), f"uv differs {what}"
    assert torch.equal(torch.from_numpy(got_p[~miss]), torch.from_numpy(want[3][~miss])), f"point differs {what}"


def _cast(o, d, v, f, t_min=0.0, t_max=math.inf, **kw):
    t_min = _dev(t_min) if isinstance(t_min, np.ndarray) else t_min
    t_max = _dev(t_max) if isinstance(t_max, np.ndarray) else t_max
    return ops.mesh_ray_cast(_dev(o), _dev(d), _dev(v), _dev(f), t_min, t_max, return_point=True, **kw)


# ---- G1: bit for bit against ray_ref ------------------------------------------------------------------------
@pytest.mark.parametrize("which_pad", range(3), ids=PAD_IDS)
@pytest.mark.parametrize("which", range(3), ids=CELL_IDS)
@pytest.mark.parametrize("name", RC.CASES)
def test_ray_cast_equals_brute_force(name, which, which_pad):
    v, f, o, d, t_min, t_max = RC.case(name)
    cell, pad = RC.cells(v)[which], RC.pads(v)[which_pad]
    want = RC.reference(name, which_pad)
    for big_face in MC.BIG_FACES:
        _check(_cast(o, d, v, f, t_min, t_max, cell=cell, big_face=_big(big_face), pad=pad), want,
               f"(cell {cell}, big_face {big_face}, pad {pad})")


def test_default_pad_is_mesh_ray_pad():
    v, f, o, d, t_min, t_max = RC.case("icosphere2")
    assert ops.mesh_ray_pad(_dev(v)) == RC.pads(v)[1]
    index = ops.mesh_ray_index(_dev(v), _dev(f))
    assert index.pad == RC.pads(v)[1] and ops.mesh_ray_index(_dev(v), _dev(f), pad=0.25).pad == 0.25
    _check(index.ray_cast(_dev(o), _dev(d), _dev(t_min), _dev(t_max), return_point=True), RC.reference("icosphere2", 1))
    _check(_cast(o, d, v, f, t_min, t_max), RC.reference("icosphere2", 1))


# ---- G2: independence ---------------------------------------------------------------------------------------
def test_result_does_not_depend_on_batching_or_order():
    v, f, o, d, _, _ = RC.case("rays_1000")
    want = RC.reference("rays_1000", 1)
    index = ops.mesh_index(_dev(v), _dev(f), pad=RC.pads(v)[1])
    od, dd = _dev(o), _dev(d)
    first = index.ray_cast(od, dd, return_point=True)
    _check(first, want)
    again = index.ray_cast(od, dd, return_point=True)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, again))
    for k in (1, 63, 65):
        part = index.ray_cast(od[:k].contiguous(), dd[:k].contiguous(), return_point=True)
        assert all(torch.equal(a.view(torch.int32), b[:k].view(torch.int32)) for a, b in zip(part, first)), k
    perm = torch.from_numpy(np.random.default_rng(8).permutation(len(o))).cuda()
    shuffled = index.ray_cast(od[perm].contiguous(), dd[perm].contiguous(), return_point=True)
    assert all(torch.equal(a.view(torch.int32), b[perm].view(torch.int32)) for a, b in zip(shuffled, first))


def test_scalar_and_tensor_bounds_agree():
    v, f, o, d, _, _ = RC.case("rays_1000")
    index = ops.mesh_index(_dev(v), _dev(f), pad=RC.pads(v)[1])
    od, dd = _dev(o), _dev(d)
    m = len(o)
    for t_min, t_max in ((0.0, math.inf), (2.5, math.inf), (0.0, 2.5), (2.2, 3.5), (-1.0, 2.5)):
        scalar = index.ray_cast(od, dd, t_min, t_max, return_point=True)
        tensor = index.ray_cast(od, dd, torch.full((m,), t_min, device="cuda"), torch.full((m,), t_max, device="cuda"),
                                return_point=True)
        _check(scalar, RC.ray_ref(o, d, v, f, RC.pads(v)[1], t_min, t_max), f"(range {t_min} .. {t_max})")
        _check(tensor, RC.ray_ref(o, d, v, f, RC.pads(v)[1], t_min, t_max), f"(tensor range {t_min} .. {t_max})")


@pytest.mark.parametrize("name", ["icosphere2", "big_among_small", "planar"])
def test_permuting_the_faces_maps_the_winner(name):
    v, f, o, d, t_min, t_max = RC.case(name)
    pad = RC.pads(v)[1]
    t, face, _, _ = RC.reference(name, 1)
    perm = np.random.default_rng(12).permutation(len(f))              # new face i is old face perm[i]
    got = _cast(o, d, v, f[perm], t_min, t_max, pad=pad)
    assert torch.equal(got[0].cpu(), torch.from_numpy(t.copy()))
    unique = RC.n_hitters(o, d, v, f, pad, t_min, t_max) == 1
    assert unique.any()
    assert np.array_equal(perm[got[1].cpu().numpy()[unique]], face[unique])
    # and in general the winner is the lowest NEW index among the hitters: the brute force over the permuted mesh
    _check(got, RC.ray_ref(o, d, v, f[perm], pad, t_min, t_max))


# ---- G3: the range ends on the planar grid ------------------------------------------------------------------
def test_range_ends_are_inclusive():
    v, f = MC.planar()
    o, d = NC._f4([[2.25, 2.5, 1.0]]), NC._f4([[0.0, 0.0, -1.0]])          # t = 1 exactly, on face 25
    below = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    above = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    for cell in MC.cells(v):
        for big_face in MC.BIG_FACES:
            for pad in RC.pads(v)[:2]:
                kw = dict(cell=cell, big_face=_big(big_face), pad=pad)
                for t_min, t_max, hit in ((0.0, 1.0, True), (0.0, below, False), (1.0, math.inf, True),
                                          (above, math.inf, False), (1.0, 1.0, True)):
                    t, face, uv, point = _cast(o, d, v, f, t_min, t_max, **kw)
                    if hit:
                        assert t.tolist() == [1.0] and face.tolist() == [25] and point.tolist() == [[2.25, 2.5, 0.0]]
                    else:
                        assert t.tolist() == [math.inf] and face.tolist() == [-1]
                        assert torch.isnan(uv).all() and torch.isnan(point).all()


def test_t_min_past_the_first_of_two_stacked_faces():
    v = NC._f4([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, -2], [4, 0, -2], [0, 4, -2]])
    f = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    o, d = NC._f4([[1, 1, 1]]), NC._f4([[0, 0, -1]])
    for cell in (None, 0.5, 100.0):
        for t_min, want_t, want_f in ((0.0, 1.0, 0), (1.0, 1.0, 0), (1.5, 3.0, 1), (3.0, 3.0, 1), (3.5, math.inf, -1)):
            t, face, _ = ops.mesh_ray_cast(_dev(o), _dev(d), _dev(v), _dev(f), t_min=t_min, cell=cell)
            assert (t.tolist(), face.tolist()) == ([want_t], [want_f]), (cell, t_min)


# ---- G4: the padded index -----------------------------------------------------------------------------------
def _cell_np(p, lo, h, g):
    """nn_cell in numpy: clamp(floor((p - lo) / h), 0, g - 1) per axis, fp32, every operation rounded once"""
    t = np.floor((p.astype(np.float32) - np.asarray(lo, np.float32)) / np.float32(h))
    return np.minimum(np.clip(t, 0, 2.0 ** 30).astype(np.int64), np.asarray(g, np.int64) - 1)


@pytest.mark.parametrize("big_face", [None, 1, 8, 1 << 40])
@pytest.mark.parametrize("name,cell,pad", [("big_among_small", None, 0.01), ("big_among_small", 0.25, 0.3),
                                          ("icosphere2", 0.3, 0.05), ("planar", 1.0, 0.5), ("soup_257", None, 1e-3)])
def test_padded_index_layout(name, cell, pad, big_face):
    v, f, _ = MC.case(name)
    big_face = _big(big_face)
    index = ops.mesh_index(_dev(v), _dev(f), cell=cell, big_face=big_face, pad=pad)
    assert index.pad == float(np.float32(pad))
    g = index.g
    cs = index.cell_start.cpu().numpy()
    rec = index.records.cpu().numpy()
    n_pairs, n_big = index.n_pairs, index.n_big
    assert rec.shape == (n_pairs + n_big, 12) and len(cs) == g[0] * g[1] * g[2] + 1
    assert cs[0] == 0 and cs[-1] == n_pairs and np.all(np.diff(cs) >= 0)
    face_of = rec[:, 9].view(np.int32)
    assert np.array_equal(rec[:, :9], v[f[face_of]].reshape(-1, 9)) and (rec[:, 10:] == 0).all()
    # what the layout must be: every face in exactly the cells of its PADDED box, or in the big list
    tri = v[f]
    c0 = _cell_np(tri.min(1) - np.float32(pad), index.lo, index.h, g)
    c1 = _cell_np(tri.max(1) + np.float32(pad), index.lo, index.h, g)
    n_cells = np.prod(c1 - c0 + 1, axis=1)
    plain = np.prod(_cell_np(tri.max(1), index.lo, index.h, g) - _cell_np(tri.min(1), index.lo, index.h, g) + 1, axis=1)
    assert (n_cells >= plain).all() and n_cells.sum() > plain.sum()                  # the pad lists more
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


@pytest.mark.parametrize("name", ["icosphere2", "big_among_small", "planar", "outside"])
def test_closest_point_on_a_padded_index_is_exact(name):
    v, f, q = MC.case(name)
    want = MC.reference(name)
    for cell in MC.cells(v):
        for pad in RC.pads(v)[1:]:
            got = ops.mesh_index(_dev(v), _dev(f), cell=cell, pad=pad).query(_dev(q), return_feature=True)
            for a, b in zip(got, want):
                assert np.array_equal(a.cpu().numpy(), b, equal_nan=True), (cell, pad)


def test_pad_zero_is_the_index_without_a_pad():
    v, f, _ = MC.case("big_among_small")
    for cell in (None, 0.25):
        a, b = ops.mesh_index(_dev(v), _dev(f), cell=cell), ops.mesh_index(_dev(v), _dev(f), cell=cell, pad=0.0)
        assert a.pad == b.pad == 0.0 and (a.h, a.g, a.lo, a.n_pairs, a.n_big) == (b.h, b.g, b.lo, b.n_pairs, b.n_big)
        assert torch.equal(a.cell_start, b.cell_start)
        assert torch.equal(a.records.view(torch.int32), b.records.view(torch.int32))


# ---- G5: errors ---------------------------------------------------------------------------------------------
def test_bad_rays_raise_and_leave_the_library_usable():
    v, f, o, d, t_min, t_max = RC.case("icosphere1")
    want = RC.reference("icosphere1", 1)
    index = ops.mesh_index(_dev(v), _dev(f), pad=RC.pads(v)[1])
    args = dict(o=o, d=d, t_min=t_min, t_max=t_max)
    for name, bad in (("o", np.nan), ("o", np.inf), ("d", np.nan), ("d", -np.inf), ("t_min", np.nan),
                      ("t_min", np.inf), ("t_min", -np.inf), ("t_max", np.nan)):
        mod = {k: np.array(a) for k, a in args.items()}
        if mod[name].ndim == 2:
            mod[name][5, 1] = bad
        else:
            mod[name][5] = bad
        with pytest.raises(HashmodError, match="non-finite"):
            index.ray_cast(_dev(mod["o"]), _dev(mod["d"]), _dev(mod["t_min"]), _dev(mod["t_max"]))
        with pytest.raises(HashmodError, match="non-finite"):
            _cast(mod["o"], mod["d"], v, f, mod["t_min"], mod["t_max"])
    _check(index.ray_cast(_dev(o), _dev(d), _dev(t_min), _dev(t_max), return_point=True), want)
    _check(_cast(o, d, v, f, t_min, t_max), want)


def test_outputs_are_optional_and_no_rays_give_empty_outputs():
    v, f, o, d, t_min, t_max = RC.case("icosphere1")
    want = RC.reference("icosphere1", 1)
    index = ops.mesh_index(_dev(v), _dev(f), pad=RC.pads(v)[1])
    a = (_dev(o), _dev(d), _dev(t_min), _dev(t_max))
    out = index.ray_cast(*a, return_uv=False)
    assert len(out) == 2 and torch.equal(out[0].cpu(), torch.from_numpy(want[0].copy()))
    out = index.ray_cast(*a, return_uv=False, return_point=True)
    assert len(out) == 3 and np.array_equal(out[2].cpu().numpy(), want[3], equal_nan=True)
    stats = {}
    out = index.ray_cast(*a, stats=stats)
    assert len(out) == 3 and np.array_equal(out[2].cpu().numpy(), want[2], equal_nan=True)
    assert stats["face_tests"] >= int((want[1] >= 0).sum())
    none = torch.zeros((0, 3), device="cuda")
    t, face, uv, point = index.ray_cast(none, none, return_point=True)
    assert t.shape == (0,) and face.shape == (0,) and uv.shape == (0, 2) and point.shape == (0, 3)
    t, face, uv = ops.mesh_ray_cast(none, none, _dev(v), _dev(f))
    assert t.shape == (0,) and face.dtype == torch.int32 and uv.shape == (0, 2)


# ---- G6: against the rasteriser -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,views", [("sphere", (0, 1, 2, 3)), ("nested", (1,))])
def test_pixel_centre_rays_see_the_rendered_faces(name, views):
    """the rays through the pixel centres, d = R ((col - cx) / fx, (row - cy) / fy, 1): where the rasteriser's hit is
    not near an edge of its face (all three weights >= 0.02) the ray cast reports the rendered face, every one.
    Those pixels are at least 80 % of the covered ones; by the CPU reference of the rasteriser alone
    (mesh_render_cases.scene_render) they are 89.7 % for the sphere's four views and 88.1 % for view 1 of "nested"
    (85.6 % over its four views; view 0 looks straight along a lattice axis, sees many marching-cubes faces edge-on
    and has 75.1 %, so it is not the view taken here)."""
    m = CC.scene(name)
    v, f = m["verts"], m["faces"]
    vw = CC.VIEWS_A
    H, W = vw["H"], vw["W"]
    proj = np.ascontiguousarray(vw["proj"][list(views)])
    ren = ops.mesh_render(_dev(v), _dev(f), proj, H, W, return_weights=True)
    row, col = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    O, D = [], []
    for k in views:
        K, pose = vw["intrinsics"][k].astype(np.float64), vw["pose"][k].astype(np.float64)
        cam = np.stack([(col - K[0, 2]) / K[0, 0], (row - K[1, 2]) / K[1, 1], np.ones_like(col)], -1).reshape(-1, 3)
        D.append(cam @ pose[:3, :3].T)
        O.append(np.broadcast_to(pose[:3, 3], D[-1].shape))
    o, d = NC._f4(np.concatenate(O)), NC._f4(np.concatenate(D))
    pad = float(RC.default_pad(v))
    got = _cast(o, d, v, f)
    _check(got, RC.ray_ref(o, d, v, f, pad))
    face_id = ren.face_id.cpu().numpy().reshape(-1)
    weights = ren.weights.cpu().numpy().reshape(-1, 3)
    covered = face_id >= 0
    safe = covered & (weights.min(1) >= 0.02)
    cast_face = got[1].cpu().numpy()
    print(f"{name}: {safe.sum()} of {covered.sum()} covered pixels are safe; "
          f"{(cast_face[safe] == face_id[safe]).sum()} agree")
    assert safe.sum() >= 0.8 * covered.sum() > 0
    assert np.array_equal(cast_face[safe], face_id[safe])


# ---- G7: analytic shells ------------------------------------------------------------------------------------
def _shell_check(o, d, t, face, v, f):
    """a convex mesh inscribed in the unit sphere contains the sphere of radius r_in: a ray whose line passes within
    r_in of the centre hits, between its entries into the two spheres (widened by 16 * 2^-24 * max(4, t)); a ray
    that passes outside radius 1 misses.  Returns (inner, outer, t_1, t_in)."""
    r_in = RC.inner_radius(v, f)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    d64 = d64 / np.linalg.norm(d64, axis=-1, keepdims=True)
    closest = np.linalg.norm(np.cross(o64, d64), axis=-1)
    t_1, _ = RC.sphere_entry(o64, d64, 1.0)
    t_in, _ = RC.sphere_entry(o64, d64, r_in)
    inner, outer = closest < r_in, closest > 1.0
    assert inner.sum() > 0 and outer.sum() > 0
    assert (face[inner] >= 0).all() and (face[outer] < 0).all() and np.isinf(t[outer]).all()
    t64 = t.astype(np.float64)
    wide = 16 * 2.0 ** -24 * np.maximum(4.0, t64[inner])
    assert (t64[inner] >= t_1[inner] - wide).all() and (t64[inner] <= t_in[inner] + wide).all()
    return inner, outer, t_1, t_in


def test_analytic_shell_through_cast_camera_rays():
    v, f = NC.icosphere(4)
    H, W = 48, 64
    eyes = [(3.0, 0.0, 0.0), (-1.5, 2.4, 1.0), (0.3, -2.0, 2.2), (-1.0, -1.0, -2.6)]
    eyes = [tuple(3.0 * np.asarray(e) / np.linalg.norm(e)) for e in eyes]
    pose = np.stack([CC.look_at(e) for e in eyes])
    K = np.stack([CC.intrinsics(80.0, H, W)] * len(eyes))
    row, col = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    uv = np.broadcast_to(np.stack([col, row], -1).reshape(1, -1, 2), (len(eyes), H * W, 2))
    uvd, posed, Kd = _dev(uv), _dev(pose), _dev(K)
    index = ops.mesh_index(_dev(v), _dev(f), pad=ops.mesh_ray_pad(_dev(v)))
    t, face, hit = cast_camera_rays(index, uvd, posed, Kd)
    assert t.shape == face.shape == hit.shape == (len(eyes), H * W) and hit.dtype == torch.bool
    assert torch.equal(hit, face >= 0) and torch.equal(hit, torch.isfinite(t))
    dirs, cam, _, _ = ops.camera_rays(uvd, posed, Kd, 1.0)
    d = dirs.cpu().numpy().reshape(-1, 3)
    o = np.repeat(cam.cpu().numpy(), H * W, axis=0)
    tn, fn = t.cpu().numpy().reshape(-1), face.cpu().numpy().reshape(-1)
    inner, outer, t_1, t_in = _shell_check(o, d, tn, fn, v, f)
    # the same through a (verts, faces) pair, and inside the tracer's bounding sphere: the range of every ray that
    # meets the mesh contains its first hit
    for mesh, radius in (((_dev(v), _dev(f)), None), (index, 1.5)):
        other = cast_camera_rays(mesh, uvd, posed, Kd, radius=radius)
        assert all(torch.equal(a, b) for a, b in zip(other, (t, face, hit)))
    t_small, _, hit_small = cast_camera_rays(index, uvd, posed, Kd, radius=0.5)       # inside the mesh: nothing to hit
    assert not hit_small.any() and torch.isinf(t_small).all()
    # against the analytic unit sphere on the rays that are clearly inside or outside
    clear = inner | outer
    want_t = np.where(inner, t_1, np.inf).astype(np.float32)
    r = depth_agreement(_dev(tn[clear]), _dev(fn[clear] >= 0), _dev(want_t[clear]), _dev(inner[clear]))
    print(r, f"bound {np.max(t_in[inner] - t_1[inner]):.3e}")
    assert r.n == int(clear.sum()) and r.n_both == int(inner.sum()) and r.iou == 1.0
    # want_t is t_1 rounded to fp32: half an ulp of a value in [2, 4) on top of the bound
    assert 0.0 <= r.median <= r.max and 0.0 <= r.mean <= r.max <= np.max(t_in[inner] - t_1[inner]) + 2.0 ** -23
    diff = np.abs(tn[inner].astype(np.float64) - want_t[inner].astype(np.float64))
    assert r.max == diff.max() and r.mean == pytest.approx(diff.mean(), rel=1e-12)
    assert r.median == np.sort(diff)[(len(diff) - 1) // 2]
    empty = depth_agreement(_dev(tn[:4]), _dev(np.zeros(4, bool)), _dev(tn[:4]), _dev(np.zeros(4, bool)))
    assert empty.n == 4 and empty.n_both == 0 and all(math.isnan(x) for x in empty[2:])


# ---- G8: medium size ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _medium_rays():
    target = NC.sphere_clouds()[0]
    o = 3.0 * RC._unit(np.random.default_rng(41), len(target))
    w = target.astype(np.float64) - o
    return NC._f4(o), NC._f4(w / np.linalg.norm(w, axis=1, keepdims=True))


def test_medium_size():
    v, f = NC.icosphere(5)
    o, d = _medium_rays()
    assert len(f) == 20480 and len(o) == 200000
    index = ops.mesh_index(_dev(v), _dev(f), pad=ops.mesh_ray_pad(_dev(v)))
    od, dd = _dev(o), _dev(d)
    stats = {}
    t, face, uv, point = index.ray_cast(od, dd, return_point=True, stats=stats)
    print(f"{stats['face_tests'] / len(o):.1f} face tests per ray")
    _shell_check(o, d, t.cpu().numpy(), face.cpu().numpy(), v, f)
    some = slice(0, None, 100)
    _check((t[some], face[some], uv[some], point[some]), RC.ray_ref(o[some], d[some], v, f, index.pad))
    again = index.ray_cast(od, dd, return_point=True)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((t, face, uv, point), again))
