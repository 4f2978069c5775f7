"""The texture kernels (csrc/hm_mesh_texture.hip), the bake (evaluation.texture.texture_mesh) and the textured views
(evaluation.mesh_views) against the numpy restatement (tests/mesh_texture_cases.py), bit for bit: fp32 as int32 words,
fp64 as int64 words."""
import functools

import numpy as np
import pytest
import torch

import mesh_color_cases as CC
import mesh_cull_cases as MC
import mesh_render_cases as MR
import mesh_texture_cases as TC
from hashmodnffbanks_idr_amd import _lib, ops
from hashmodnffbanks_idr_amd.evaluation import (TextureStats, color_mesh, evaluate_mesh_views, render_mesh, texture_mesh,
                                                texture_mesh_for_dataset)

pytestmark = pytest.mark.gpu


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()   # a copy: the cases are read-only


def _bits32(x):
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    assert x.dtype == np.float32
    return np.ascontiguousarray(x).view(np.int32)


def _bits64(x):
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    assert x.dtype == np.float64
    return np.ascontiguousarray(x).view(np.int64)


def _same_points(got, want, what=""):
    for g, w in zip(got[:2], want[:2]):
        assert (g is None) == (w is None), what
        if w is not None:
            assert g.is_cuda and g.dtype == torch.float32 and np.array_equal(_bits32(g), _bits32(w)), what
    assert got[2].dtype == torch.int32 and np.array_equal(got[2].cpu().numpy(), want[2]), what


# ---------------------------------------------------------------------------------------------------------------------
# points, normals and the face map
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [1, 2, 5])
@pytest.mark.parametrize("n_faces", [1, 2, 5, 37])
def test_texel_points_of_small_meshes(n_faces, res):
    verts, faces, normals = TC.fan_mesh(n_faces)
    Hb, Wb = TC.block_shape(res)
    for nrm in (normals, None):
        want = TC.texel_points_ref(verts, faces, res, nrm)
        got = ops.mesh_texture_points(_t(verts), _t(faces), res, _t(nrm))
        assert tuple(got[0].shape) == ((n_faces + 1) // 2 * Hb * Wb, 3)
        _same_points(got, want, (n_faces, res, nrm is not None))
    assert (want[2] < 0).sum() == (Hb * Wb // 2 if n_faces % 2 else 0)
    if (n_faces, res) == (37, 5):
        assert len(want[2]) == 1064                       # more than one workgroup, not a multiple of 256


def test_texel_points_of_the_sphere():
    m = MC.scene("sphere")
    for res in (1, 4):
        want = TC.texel_points_ref(m["verts"], m["faces"], res, m["normals"])
        _same_points(ops.mesh_texture_points(_t(m["verts"]), _t(m["faces"]), res, _t(m["normals"])), want, res)
    assert len(want[2]) > 20000


def test_texel_points_of_odd_meshes():
    """a NaN and an infinite vertex, a degenerate face (a repeated vertex, and three equal ones), a face index equal to
    V and a negative one"""
    verts, faces, normals = TC.fan_mesh(7)
    verts, faces, normals = verts.copy(), faces.copy(), normals.copy()
    assert (faces == 2).sum() == 1 and faces[0, 1] == 2 and (faces == 5).sum() == 1 and not (faces == 1).any()
    verts[2] = (np.nan, 0.5, -0.5)                         # a corner of face 0 only
    verts[5, 1] = np.inf                                   # a corner of face 6 only
    normals[faces[2, 0]] = (0.0, np.nan, 1.0)
    faces[4] = (faces[4, 0], faces[4, 0], faces[4, 1])
    faces[5] = (1, 1, 1)
    want = TC.texel_points_ref(verts, faces, 3, normals)
    _same_points(ops.mesh_texture_points(_t(verts), _t(faces), 3, _t(normals)), want)
    assert np.isnan(want[0][want[2] == 0]).any() and np.isfinite(want[0][want[2] == 1]).all()
    assert (want[0][want[2] == 5] == verts[1]).all() and np.isinf(want[0][want[2] == 6]).any()
    for bad in (len(verts), -1, 1 << 30):
        broken = faces.copy()
        broken[6, 1] = bad
        for nrm in (normals, None):
            with pytest.raises(_lib.HashmodError, match="face index"):
                ops.mesh_texture_points(_t(verts), _t(broken), 3, _t(nrm))
    empty = ops.mesh_texture_points(_t(verts), _t(faces[:0]), 3, _t(normals))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[2].shape == (0,)


# ---------------------------------------------------------------------------------------------------------------------
# the bake
# ---------------------------------------------------------------------------------------------------------------------
BAKE_RES = 2


@functools.lru_cache(maxsize=None)
def _bake_inputs(name, which):
    m, vw = MC.scene(name), MC.views(which)
    pts, nrm, face = TC.texel_points_ref(m["verts"], m["faces"], BAKE_RES, -m["normals"])
    return m, vw, pts, nrm, face, np.isfinite(MC.scene_depth(name, which)[0])


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("name", ["sphere", "nested"])
def test_bake_is_the_vertex_colours_of_the_texel_points(name, which):
    m, vw, pts, nrm, face, silhouette = _bake_inputs(name, which)
    images, centers = CC.noise_images(which), CC.view_centers(vw)
    ref_depth = MC.scene_depth(name, which)
    mesh = (_t(m["verts"]), _t(m["faces"]), _t(-m["normals"]))
    K, pose, d_images = _t(vw["intrinsics"]), _t(vw["pose"]), _t(images)
    d_pts, d_nrm, d_face = ops.mesh_texture_points(mesh[0], mesh[1], BAKE_RES, mesh[2])
    _same_points((d_pts, d_nrm, d_face), (pts, nrm, face))
    depth, _ = ops.mesh_depth_maps(mesh[0], mesh[1], vw["proj"], vw["H"], vw["W"])
    assert np.array_equal(_bits32(depth), _bits32(ref_depth[0]))
    Hb, Wb = TC.block_shape(BAKE_RES)
    n = len(vw["proj"])
    for mode in CC.MODES:
        for masks in (None, silhouette):
            kw = dict(erode=1, min_cos=0.1, power=2, mode=mode)
            fill = (0.25, -0.5, 0.75)
            texels, used, stats, (acc, n_used) = TC.bake_ref(m["verts"], m["faces"], -m["normals"], vw, images, BAKE_RES,
                                                             masks, fill=fill, depth=ref_depth, **kw)
            what = (name, which, mode, masks is not None)
            assert 500 < stats["n_colored"] < stats["n_texels"] == (face >= 0).sum(), what
            dev = ops.mesh_vertex_colors(d_pts, d_nrm, vw["proj"], centers, d_images, depth, masks=_t(masks), **kw)
            assert np.array_equal(_bits64(dev[0]), _bits64(acc)) and np.array_equal(dev[1].cpu().numpy(), n_used), what
            # the views split into [0, k) + [k, n)
            for k in (1, n - 1):
                out = ops.mesh_vertex_colors(d_pts, d_nrm, vw["proj"][:k], centers[:k], d_images[:k], depth[:k],
                                             masks=_t(None if masks is None else masks[:k]), **kw)
                ops.mesh_vertex_colors(d_pts, d_nrm, vw["proj"][k:], centers[k:], d_images[k:], depth[k:],
                                       masks=_t(None if masks is None else masks[k:]), out=out, **kw)
                assert torch.equal(out[0].view(torch.int64), dev[0].view(torch.int64)) and torch.equal(out[1], dev[1])
            fin = ops.mesh_colors_finish(*dev, mode, fill).reshape(-1, Hb, Wb, 3)
            for view_bytes in (1 << 28, 1, 3 * 17 * vw["H"] * vw["W"]):
                atlas, got_stats = texture_mesh(mesh, K, pose, d_images, (vw["H"], vw["W"]), res=BAKE_RES,
                                                masks=_t(masks), fill=fill, view_bytes=view_bytes, **kw)
                assert isinstance(atlas, ops.TextureAtlas) and isinstance(got_stats, TextureStats)
                assert (atlas.res, atlas.n_faces, atlas.block_shape, atlas.fill) == (BAKE_RES, len(m["faces"]), (Hb, Wb),
                                                                                     fill)
                assert atlas.texels.is_cuda and torch.equal(atlas.texels.view(torch.int32), fin.view(torch.int32)), what
                assert np.array_equal(_bits32(atlas.texels), _bits32(texels)), what
                assert np.array_equal(atlas.used.cpu().numpy(), used) and got_stats._asdict() == stats, what


def test_texture_mesh_for_dataset_and_host_inputs():
    m, vw = MC.scene("sphere"), MC.views("A")
    images, masks = CC.sphere_images("A")
    want = TC.bake_ref(m["verts"], m["faces"], -m["normals"], vw, images, 3, masks, depth=MC.scene_depth("sphere", "A"))
    data = TC.Dataset(vw, images, masks)
    mesh = (_t(m["verts"]), _t(m["faces"]), _t(-m["normals"]))
    for kw in ({}, {"view_bytes": 1}):
        atlas, stats = texture_mesh_for_dataset(mesh, data, res=3, **kw)
        assert np.array_equal(_bits32(atlas.texels), _bits32(want[0])) and stats._asdict() == want[2]
    plain, stats = texture_mesh_for_dataset(mesh, data, res=3, masks=None)
    ref = TC.bake_ref(m["verts"], m["faces"], -m["normals"], vw, images, 3, None, depth=MC.scene_depth("sphere", "A"))
    assert np.array_equal(_bits32(plain.texels), _bits32(ref[0])) and stats._asdict() == ref[2]
    # the image of the export is the restatement's
    assert np.array_equal(_bits32(atlas.image()), _bits32(TC.atlas_image_ref(want[0], 3)))


# ---------------------------------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------------------------------
def _noise_texels(n_faces, res, seed=0):
    Hb, Wb = TC.block_shape(res)
    return np.random.default_rng(seed).uniform(-1, 1, ((n_faces + 1) // 2, Hb, Wb, 3)).astype(np.float32)


@pytest.mark.parametrize("res", [1, 2, 5])
def test_sampler_on_the_renders_own_faces_and_weights(res):
    m, vw = MC.scene("sphere"), MC.views("A")
    n_faces = len(m["faces"])
    texels = _noise_texels(n_faces, res, res)
    ren = ops.mesh_render(_t(m["verts"]), _t(m["faces"]), vw["proj"], vw["H"], vw["W"], return_weights=True)
    ref = MR.scene_render("sphere", "A")
    assert np.array_equal(ren.face_id.cpu().numpy(), ref["face_id"])
    assert np.array_equal(_bits32(ren.weights), _bits32(ref["weights"]))
    bg = (0.5, -2.0, 7.0)
    want = TC.texture_sample_ref(texels, res, n_faces, ref["face_id"], ref["weights"], bg)
    got = ops.mesh_texture_sample(_t(texels), res, n_faces, ren.face_id, ren.weights, bg)
    assert got.is_cuda and tuple(got.shape) == ref["face_id"].shape + (3,)
    assert np.array_equal(_bits32(got), _bits32(want))
    again = ops.mesh_texture_sample(_t(texels), res, n_faces, ren.face_id, ren.weights, bg)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    drawn = ref["face_id"] >= 0
    assert 3000 < drawn.sum() < drawn.size and (want[~drawn] == np.asarray(bg, np.float32)).all()
    assert (ref["face_id"][drawn] % 2 == 1).sum() > 1000 and (ref["face_id"][drawn] % 2 == 0).sum() > 1000


@pytest.mark.parametrize("res", [1, 2, 5])
def test_sampler_at_corners_edges_and_beyond(res):
    n_faces = 37                                           # the last face is alone in its block
    Hb, Wb = TC.block_shape(res)
    texels = _noise_texels(n_faces, res, 40 + res)
    texels[3] = (0.125, -0.75, 0.5)                        # faces 6 and 7 have one colour
    d_tex = _t(texels)
    corners = np.eye(3, dtype=np.float32)
    face = np.repeat(np.arange(n_faces, dtype=np.int32), 3)
    got = ops.mesh_texture_sample(d_tex, res, n_faces, _t(face), _t(np.tile(corners, (n_faces, 1))))
    n = res
    for f in range(n_faces):
        blk = texels[f // 2]
        want = [blk[0, 0], blk[0, n], blk[n, 0]] if f % 2 == 0 else [blk[n + 1, n + 2], blk[n + 1, 2], blk[1, n + 2]]
        assert np.array_equal(_bits32(got[3 * f:3 * f + 3]), _bits32(np.stack(want))), f
    # random points of every face, the edge midpoints, and weights far outside the face: the clamp holds them
    rng = np.random.default_rng(res)
    w = rng.dirichlet((1.0, 1.0, 1.0), 600).astype(np.float32)
    odd = np.asarray([[0.5, 0.5, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0, 1, 1], [-1, 2, 0], [3, -1, -1], [0, 1e30, -1e30],
                      [0, -3e38, 3e38], [1, 3e38, 3e38], [1, 0, np.nan], [np.nan, 0, 0], [0, np.inf, 0],
                      [0, 0, -np.inf], [np.inf, 0.5, 0.5]], np.float32)
    w = np.concatenate([w, np.tile(odd, (4, 1))])
    f = np.concatenate([rng.integers(0, n_faces, 600), np.repeat([0, 1, 36, 7], len(odd))]).astype(np.int32)
    f[:40] = -1
    f[40:60] = -(1 << 31)
    f[60:120] = 36
    f[120:180] = 7
    f, w = f.reshape(2, -1), w.reshape(2, -1, 3)
    bg = 0.375
    want = TC.texture_sample_ref(texels, res, n_faces, f, w, bg)
    got = ops.mesh_texture_sample(d_tex, res, n_faces, _t(f), _t(w), bg)
    assert tuple(got.shape) == f.shape + (3,) and np.array_equal(_bits32(got), _bits32(want))
    flat_f, flat_w, flat = f.reshape(-1), w.reshape(-1, 3), want.reshape(-1, 3)
    assert (flat[flat_f < 0] == np.float32(bg)).all() and (flat[~np.isfinite(flat_w).all(1)] == np.float32(bg)).all()
    inside = (flat_f == 7) & (flat_w.min(1) >= 0) & (flat_w.max(1) <= 1.0)
    inside[inside] = flat_w[inside].sum(1) <= 1.0
    assert inside.sum() > 50 and np.array_equal(flat[inside], np.tile(texels[3, 0, 0], (inside.sum(), 1)))
    for bad in (n_faces, n_faces + 1, (1 << 31) - 1):
        broken = f.copy()
        broken[1, 5] = bad
        with pytest.raises(_lib.HashmodError, match="face_id"):
            ops.mesh_texture_sample(d_tex, res, n_faces, _t(broken), _t(w), bg)
    none = ops.mesh_texture_sample(d_tex, res, n_faces, _t(f[:, :0]), _t(w[:, :0]))
    assert tuple(none.shape) == (2, 0, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the textured views
# ---------------------------------------------------------------------------------------------------------------------
def test_render_mesh_with_a_texture_is_the_sampler_composed_by_hand():
    m, vw = MC.scene("sphere"), MC.views("B")
    n_faces, res = len(m["faces"]), 3
    texels = 1.2 * _noise_texels(n_faces, res, 8)           # some beyond [-1, 1]: the clamp shows
    mesh = (_t(m["verts"]), _t(m["faces"]))
    atlas = ops.TextureAtlas(res, n_faces, _t(texels))
    K, pose = _t(vw["intrinsics"]), _t(vw["pose"])
    bg = (1.0, 0.5, 0.25)
    ren = ops.mesh_render(mesh[0], mesh[1], vw["proj"], vw["H"], vw["W"], return_weights=True)
    unit = ((atlas.texels + 1.0) / 2.0).clamp(0.0, 1.0).contiguous()
    hand = ops.mesh_texture_sample(unit, res, n_faces, ren.face_id, ren.weights, bg).clamp(0.0, 1.0)
    want = TC.texture_views_ref(m["verts"], m["faces"], vw, res, texels, bg, render=MR.scene_render("sphere", "B"))
    for view_bytes in (1 << 28, 1):
        got = render_mesh(mesh, K, pose, (vw["H"], vw["W"]), texture=atlas, background=bg, view_bytes=view_bytes)
        assert torch.equal(got.rgb.view(torch.int32), hand.view(torch.int32))
        assert np.array_equal(_bits32(got.rgb), _bits32(want))
        assert torch.equal(got.face_id, ren.face_id) and torch.equal(got.coverage, ren.face_id >= 0)
        assert torch.equal(got.depth.view(torch.int32), ren.depth.view(torch.int32))
    assert (np.abs(texels) > 1.0).sum() > 1000 and want.min() >= 0.0 and want.max() <= 1.0


def test_color_mesh_keeps_its_bits():
    """the refactor of color_mesh's loop: the sphere against color_mesh_ref"""
    m, vw = MC.scene("sphere"), MC.views("A")
    images, masks = CC.noise_images("A"), np.isfinite(MC.scene_depth("sphere", "A")[0])
    mesh = (_t(m["verts"]), _t(m["faces"]), _t(-m["normals"]))
    K, pose = _t(vw["intrinsics"]), _t(vw["pose"])
    for mode in CC.MODES:
        for msk in (None, masks):
            kw = dict(erode=1, min_cos=0.1, power=2, mode=mode, fill=(0.5, -0.25, 2.0))
            want, want_stats = CC.color_mesh_ref(m["verts"], m["faces"], -m["normals"], vw, images, msk,
                                                 depth=MC.scene_depth("sphere", "A"), **kw)
            for view_bytes in (1 << 28, 1):
                colors, stats = color_mesh(mesh, K, pose, _t(images), (vw["H"], vw["W"]), masks=_t(msk),
                                           view_bytes=view_bytes, **kw)
                assert np.array_equal(_bits32(colors), _bits32(want)) and stats._asdict() == want_stats


def test_a_texture_scores_higher_than_vertex_colours_on_a_coarse_mesh():
    """The sphere scene simplified by ops.mesh_simplify at a cell of 0.3 (108 faces of about 20 pixels each), the
    photographs of views A with an analytic pattern of about three periods across the sphere.  On the CPU, with
    mesh_simplify_cases.simplify and the restatements (mean PSNR over the masks of the four views, data range 1):
    vertex colours 15.25 dB, texture at res 2 17.95 dB, at res 4 18.84 dB - both are held down by the coarse
    silhouette, which the masks count.  The assertion is the order, not a number."""
    m, vw = MC.scene("sphere"), MC.views("A")
    images, masks = TC.pattern_images("A")
    verts, faces, normals, _ = ops.mesh_simplify(_t(m["verts"]), _t(m["faces"]), _t(-m["normals"]), cell=TC.COARSE_CELL)
    ref = TC.coarse_sphere_ref()
    assert abs(len(faces) - len(ref[1])) <= 4 and len(faces) < len(m["faces"]) // 10
    data = TC.Dataset(vw, images, masks)
    mesh = (verts, faces, normals)
    K, pose = _t(vw["intrinsics"]), _t(vw["pose"])
    colors, _ = color_mesh(mesh, K, pose, _t(images), (vw["H"], vw["W"]), masks=_t(masks))
    atlas, stats = texture_mesh(mesh, K, pose, _t(images), (vw["H"], vw["W"]), res=4, masks=_t(masks))
    assert stats.n_colored > stats.n_texels // 2
    plain = evaluate_mesh_views(mesh, data, colors=colors)
    textured = evaluate_mesh_views(mesh, data, texture=atlas)
    print("mean PSNR: vertex colours", plain.psnr_mean, "texture", textured.psnr_mean, "| SSIM", plain.ssim_mean,
          textured.ssim_mean)
    assert textured.psnr_mean > plain.psnr_mean
