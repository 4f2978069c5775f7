"""The numpy restatement of the texture atlas (tests/mesh_texture_cases.py) against independent truths, so that the
GPU tests, which compare csrc/hm_mesh_texture.hip with it bit for bit, cannot pass vacuously; the new entry points' ABI
and argument checks; ops.TextureAtlas' image and coordinates; TriMesh.export_obj (runs anywhere)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import mesh_cull_cases as MC
import mesh_render_cases as MR
import mesh_texture_cases as TC
from hashmodnffbanks_idr_amd import _lib, ops
from hashmodnffbanks_idr_amd.evaluation import (TextureStats, evaluate_mesh_views, render_mesh,  # noqa: F401
                                                texture_mesh, texture_mesh_for_dataset)
from hashmodnffbanks_idr_amd.utils.plots import TriMesh, colors_to_uint8

NEW_SYMBOLS = {"hm_mesh_texture_points": (C.c_int, 11), "hm_mesh_texture_sample": (C.c_int, 10)}
RES = (1, 2, 3, 5, 8)


# ---------------------------------------------------------------------------------------------------------------------
# the layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", RES)
def test_every_texel_of_a_block_has_one_owner(n):
    Hb, Wb = TC.block_shape(n)
    assert (Hb, Wb) == (n + 2, n + 3) == ops.texture_block_shape(n)
    upper, S, T = TC.layout_ref(n)
    j, i = np.meshgrid(np.arange(Hb), np.arange(Wb), indexing="ij")
    lower_set = {(a, b) for a, b in zip(i.ravel(), j.ravel()) if a + b <= n + 1}
    upper_set = {(n + 2 - a, n + 1 - b) for a, b in lower_set}                  # the lower rule, point-mirrored
    assert lower_set.isdisjoint(upper_set) and len(lower_set) + len(upper_set) == Hb * Wb
    assert lower_set | upper_set == set(zip(i.ravel(), j.ravel()))
    assert {(a, b) for a, b in zip(i[upper], j[upper])} == upper_set
    # the numerators are mirror images too, and every texel is a point of its face: S, T >= 0, S + T <= 2n
    assert np.array_equal(S[::-1, ::-1], S) and np.array_equal(T[::-1, ::-1], T)
    assert S.min() == 0 and T.min() == 0 and (S + T).max() == 2 * n
    # the corners sit at (0, 0), (n, 0), (0, n), and the gutter lies on the hypotenuse
    assert (S[0, 0], T[0, 0]) == (0, 0) and (S[0, n], T[0, n]) == (2 * n, 0) and (S[n, 0], T[n, 0]) == (0, 2 * n)
    gutter = (~upper) & (i + j == n + 1)
    assert gutter.sum() == n + 2 and ((S + T)[gutter] == 2 * n).all()
    interior = (~upper) & (i + j <= n)
    assert interior.sum() == (n + 1) * (n + 2) // 2
    assert np.array_equal(S[interior], 2 * i[interior]) and np.array_equal(T[interior], 2 * j[interior])
    print("res", n, "interior texels", 2 * int(interior.sum()), "of", Hb * Wb)
    assert {5: (42, 56), 8: (90, 110)}.get(n, (2 * interior.sum(), Hb * Wb)) == (2 * interior.sum(), Hb * Wb)


def _barycentrics(n_random, seed):
    """fp32 [K,3]: random points of a triangle, then the three corners and the three edge midpoints exactly"""
    rng = np.random.default_rng(seed)
    a, b = rng.random(n_random), rng.random(n_random)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    w = np.stack([1 - a - b, a, b], 1)
    exact = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0], [0, 0.5, 0.5], [0.5, 0, 0.5]]
    return np.concatenate([w, np.asarray(exact)]).astype(np.float32)


@pytest.mark.parametrize("n", RES)
def test_no_tap_of_a_point_inside_a_face_reads_the_other_face(n):
    """The only way to the other face's set is the fp32 rounding of the weights (w1 + w2 above 1 by an ulp): such a
    tap's weight is of that size.  The cap is 1e-6; the largest weight found is printed."""
    owner = TC.layout_ref(n)[0]
    for upper in (False, True):
        w = _barycentrics(100000, 10 * n + upper)
        x, y, wt = TC.sample_taps_ref(n, upper, w)
        foreign = owner[y, x] != upper
        worst = float(wt[foreign].max()) if foreign.any() else 0.0
        print("res", n, "upper" if upper else "lower", "taps in the other set:", int((foreign & (wt > 0)).sum()),
              "largest weight", worst)
        assert worst <= 1e-6
        assert np.allclose(wt.sum(1), 1.0, atol=1e-12) and wt.min() >= 0.0
        # the corners' taps: all the weight on the corner texel
        corner = {False: [(0, 0), (n, 0), (0, n)], True: [(n + 2, n + 1), (2, n + 1), (n + 2, 1)]}[upper]
        for m, (cx, cy) in enumerate(corner):
            k = 100000 + m
            on = (x[k] == cx) & (y[k] == cy)
            assert wt[k][on].sum() == 1.0, (n, upper, m)


def test_texel_points_are_points_of_their_faces():
    """independent of the association: every texel's point is, to fp32 rounding, the barycentric mix of its face, lies
    in the face's plane and inside the face; the corner texels are the corners, bit for bit"""
    verts, faces, normals = TC.fan_mesh(5)
    for n in (1, 2, 5):
        Hb, Wb = TC.block_shape(n)
        pts, nrm, face = TC.texel_points_ref(verts, faces, n, normals)
        assert pts.shape == (3 * Hb * Wb, 3) == nrm.shape and face.shape == (3 * Hb * Wb,)
        blocks = face.reshape(3, Hb, Wb)
        assert (blocks[2][TC.layout_ref(n)[0]] == -1).all() and np.isnan(pts[face < 0]).all()
        assert np.isnan(nrm[face < 0]).all() and (face < 0).sum() == Hb * Wb // 2
        assert sorted(set(face.tolist())) == [-1, 0, 1, 2, 3, 4] and np.isfinite(pts[face >= 0]).all()
        p = pts.reshape(3, Hb, Wb, 3)
        for f in range(5):
            A, B, Cc = (verts[faces[f, m]] for m in range(3))
            blk = p[f // 2]
            got = [blk[0, 0], blk[0, n], blk[n, 0]] if f % 2 == 0 else [blk[n + 1, n + 2], blk[n + 1, 2], blk[1, n + 2]]
            assert all(np.array_equal(g, w) for g, w in zip(got, (A, B, Cc))), (n, f)
            mine = pts[face == f].astype(np.float64)
            M = np.stack([B - A, Cc - A], 1).astype(np.float64)
            st, res, _, _ = np.linalg.lstsq(M, (mine - A.astype(np.float64)).T, rcond=None)
            assert np.abs(M @ st + A.astype(np.float64)[:, None] - mine.T).max() < 1e-6
            assert st.min() > -1e-6 and st.sum(0).max() < 1 + 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# the 2-D image and its coordinates
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_faces", [1, 2, 5, 37])
@pytest.mark.parametrize("n", RES)
def test_face_uvs_recover_the_corner_texels(n, n_faces):
    Hb, Wb = TC.block_shape(n)
    n_blocks = (n_faces + 1) // 2
    rng = np.random.default_rng(n * 100 + n_faces)
    texels = rng.uniform(-1, 1, (n_blocks, Hb, Wb, 3)).astype(np.float32)
    atlas = ops.TextureAtlas(n, n_faces, torch.from_numpy(texels), fill=(0.25, -0.5, 0.75))
    for bw in (None, 1, 3, n_blocks + 2):
        _, Ha, Wa = TC.atlas_shape_ref(n, n_blocks, bw)
        assert atlas.atlas_shape(bw)[1:] == (Ha, Wa)
        uv = atlas.face_uvs(bw)
        assert uv.shape == (n_faces, 3, 2) and np.array_equal(uv, TC.face_uvs_ref(n, n_faces, bw))
        assert uv.min() > 0.0 and uv.max() < 1.0
        image = atlas.image(bw).numpy()
        assert image.shape == (Ha, Wa, 3) and np.array_equal(image, TC.atlas_image_ref(texels, n, bw, atlas.fill))
        x, y = uv[..., 0] * Wa - 0.5, (1.0 - uv[..., 1]) * Ha - 0.5
        xi, yi = np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)
        assert np.abs(x - xi).max() < 1e-9 and np.abs(y - yi).max() < 1e-9
        assert np.array_equal(np.stack([xi, yi], -1), TC.face_corner_texels_ref(n, n_faces, bw))
        # the pixel under a corner's coordinates is the texel the sampler returns for weights at that corner
        corners = np.eye(3, dtype=np.float32)
        for f in range(n_faces):
            want = TC.texture_sample_ref(texels, n, n_faces, np.full(3, f, np.int32), corners)
            assert np.array_equal(image[yi[f], xi[f]], want), (n, n_faces, bw, f)
    if n_blocks >= 4:                                       # the default is about a square
        _, Ha, Wa = atlas.atlas_shape()
        assert abs(Ha - Wa) <= max(Hb, Wb) + Hb


def test_export_obj_round_trip(tmp_path):
    verts, faces, normals = TC.fan_mesh(5)
    n = 3
    Hb, Wb = TC.block_shape(n)
    texels = np.random.default_rng(3).uniform(-1, 1, (3, Hb, Wb, 3)).astype(np.float32)
    atlas = ops.TextureAtlas(n, 5, torch.from_numpy(texels))
    image = colors_to_uint8(atlas.image()).reshape(tuple(atlas.atlas_shape()[1:]) + (3,))
    mesh = TriMesh(verts, faces, normals, texture=image, face_uvs=atlas.face_uvs())
    plain = TriMesh(verts, faces, normals)
    assert mesh.export() == plain.export()                                   # the .ply does not change
    paths = mesh.export_obj(str(tmp_path / "ball"))
    assert [p.rsplit(".", 1)[1] for p in paths] == ["obj", "mtl", "png"]
    assert mesh.export_obj(str(tmp_path / "ball.obj")) == paths
    v, vn, vt, fs = [], [], [], []
    lines = open(paths[0]).read().split("\n")
    assert lines[0] == "mtllib ball.mtl" and lines[1] == "usemtl ball"
    for ln in lines[2:]:
        tok = ln.split()
        if tok:
            {"v": v, "vn": vn, "vt": vt, "f": fs}[tok[0]].append(tok[1:])
    assert np.array_equal(np.asarray(v, np.float64).astype(np.float32), verts)
    assert np.array_equal(np.asarray(vn, np.float64).astype(np.float32), normals)
    corner = np.asarray([[[int(x) for x in c.split("/")] for c in f] for f in fs])          # [F, 3, (v, vt, vn)]
    assert np.array_equal(corner[..., 0] - 1, faces) and np.array_equal(corner[..., 2] - 1, faces)
    assert np.array_equal(np.asarray(vt, np.float64)[corner[..., 1] - 1], atlas.face_uvs())
    mtl = open(paths[1]).read()
    assert "newmtl ball\n" in mtl and "map_Kd ball.png\n" in mtl
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(paths[2])), image)
    with pytest.raises(ValueError, match="texture"):
        plain.export_obj(str(tmp_path / "none"))
    for bad in (dict(texture=image), dict(face_uvs=atlas.face_uvs()), dict(texture=image.astype(np.float32),
                face_uvs=atlas.face_uvs()), dict(texture=image, face_uvs=atlas.face_uvs()[:4])):
        with pytest.raises(ValueError, match="texture|face_uvs"):
            TriMesh(verts, faces, normals, **bad)
    # split gathers the faces' coordinates
    two = TriMesh(np.concatenate([verts, verts + 10]), np.concatenate([faces, faces + len(verts)]), None,
                  texture=image, face_uvs=np.concatenate([atlas.face_uvs(), atlas.face_uvs() * 0.5]))
    parts = two.split()
    assert sum(len(p.faces) for p in parts) == 10 and all(p.texture is image for p in parts)
    assert all(p.face_uvs.shape == (len(p.faces), 3, 2) for p in parts)


# ---------------------------------------------------------------------------------------------------------------------
# ABI and argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_symbols():
    L = _lib.lib()
    with open(_lib.LIB_PATH.replace("libhashmod.so", "../include/hashmod.h")) as fh:
        header = fh.read()
    for name, (res, n_args) in NEW_SYMBOLS.items():
        assert name in _lib.SIGNATURES
        fn = getattr(L, name)
        assert fn.restype is res and len(fn.argtypes) == n_args == len(_lib.SIGNATURES[name][1])
        decl = re.search(r"HM_API int(64_t)? %s\(([^;]*)\);" % name, header)
        assert decl and (decl.group(1) is not None) == (res is C.c_int64)
        assert len(decl.group(2).split(",")) == n_args


def _points(L, p, **k):
    a = dict(n_verts=8, n_faces=4, res=3, normals=True)
    a.update(k)
    return L.hm_mesh_texture_points(p, p if a["normals"] else None, a["n_verts"], p, a["n_faces"], a["res"], p,
                                    p if a["normals"] else None, p, p, None)


def _sample(L, p, **k):
    a = dict(res=3, n_faces=4, n_samples=16)
    a.update(k)
    return L.hm_mesh_texture_sample(p, a["res"], a["n_faces"], p, p, a["n_samples"], None, p, p, None)


def test_exports_refuse_bad_arguments_on_the_host():
    """-1 (HM_ERR_INVALID) from the host-side checks, before any pointer is used or any launch is made"""
    L = _lib.lib()
    host = np.zeros(4096, np.float64)
    hp = host.ctypes.data_as(C.c_void_p)
    for p in (None, hp):
        for k in (dict(n_verts=-1), dict(n_verts=1 << 31), dict(n_faces=-1), dict(n_faces=1 << 31), dict(res=0),
                  dict(res=-3), dict(res=4097), dict(res=4096, n_faces=1 << 18)):
            assert _points(L, p, **k) == -1, k
            assert b"hm_mesh_texture_points" in L.hm_last_error()
        for k in (dict(res=0), dict(res=4097), dict(n_faces=-1), dict(n_faces=1 << 31), dict(n_samples=-1),
                  dict(n_samples=1 << 40), dict(res=4096, n_faces=1 << 18)):
            assert _sample(L, p, **k) == -1, k
            assert b"hm_mesh_texture_sample" in L.hm_last_error()
    assert _points(L, None) == -1 and b"hm_mesh_texture_points: NULL" in L.hm_last_error()
    assert _sample(L, None) == -1 and b"hm_mesh_texture_sample: NULL pointer" in L.hm_last_error()
    assert L.hm_mesh_texture_points(hp, hp, 8, hp, 4, 3, hp, None, hp, hp, None) == -1        # normals without a result
    assert b"go together" in L.hm_last_error()
    assert L.hm_mesh_texture_points(hp, None, 8, hp, 4, 3, hp, hp, hp, hp, None) == -1
    # nothing to do is not an error - after the checks
    assert _points(L, None, n_faces=0) == 0 and _sample(L, None, n_samples=0) == 0
    assert _points(L, None, n_faces=0, res=0) == -1 and _sample(L, None, n_samples=0, res=0) == -1


def test_ops_check_their_arguments():
    verts, faces, normals = (torch.from_numpy(a.copy()) for a in TC.fan_mesh(5))
    with pytest.raises(_lib.HashmodError, match="no CPU fallback"):
        ops.mesh_texture_points(verts, faces, 3, normals)
    with pytest.raises(_lib.HashmodError, match="no CPU fallback"):
        ops.mesh_texture_points(verts, faces, 3)
    for res in (0, -1, 4097, 2.0, None, True):
        with pytest.raises(ValueError, match="res"):
            ops.mesh_texture_points(verts, faces, res)
    for bad in (verts.double(), verts[:, :2], torch.zeros(3, 7).t()):
        with pytest.raises(ValueError, match="verts"):
            ops.mesh_texture_points(bad, faces, 3)
    for bad in (faces.long(), faces[:, :2], torch.zeros((3, 5), dtype=torch.int32).t()):
        with pytest.raises(ValueError, match="faces"):
            ops.mesh_texture_points(verts, bad, 3)
    for bad in (normals.double(), normals[:-1]):
        with pytest.raises(ValueError, match="normals"):
            ops.mesh_texture_points(verts, faces, 3, bad)
    with pytest.raises(ValueError, match="devices"):
        ops.mesh_texture_points(verts, faces, 3, normals.to("meta"))
    Hb, Wb = ops.texture_block_shape(3)
    texels = torch.zeros((3, Hb, Wb, 3))
    face_id, weights = torch.zeros((4, 6), dtype=torch.int32), torch.zeros((4, 6, 3))
    with pytest.raises(_lib.HashmodError, match="no CPU fallback"):
        ops.mesh_texture_sample(texels, 3, 5, face_id, weights)
    bad = {"texels": (texels.double(), texels[:2], texels[..., :2], texels[:, :, ::2], None),
           "res": (0, 4097, 3.0, None),
           "n_faces": (-1, 1 << 31, 5.0, None),
           "face_id": (face_id.long(), face_id[:, ::2], None),
           "weights": (weights.double(), weights[:3], weights[..., :2], weights[:, ::2], None),
           "background": (None, (1.0, 2.0), "white", (1.0, 2.0, 3.0, 4.0))}
    for name, values in bad.items():
        for value in values:
            a = dict(texels=texels, res=3, n_faces=5, face_id=face_id, weights=weights, background=0.0)
            a[name] = value
            if name in ("res", "n_faces") and isinstance(value, int):
                a["texels"] = torch.zeros((1, 1, 1, 3))              # whatever the shape: the number is refused first
            with pytest.raises(ValueError, match=name):
                ops.mesh_texture_sample(**a)
    with pytest.raises(ValueError, match="texels"):
        ops.mesh_texture_sample(texels, 3, 7, face_id, weights)      # 7 faces are 4 blocks
    with pytest.raises(ValueError, match="devices"):
        ops.mesh_texture_sample(texels, 3, 5, face_id.to("meta"), weights.to("meta"))
    for k in (dict(texels=texels.double()), dict(texels=texels[:2]), dict(used=torch.ones((3, Hb, Wb))),
              dict(used=torch.ones((2, Hb, Wb), dtype=torch.bool)), dict(fill=(1.0, 2.0)), dict(fill=None), dict(res=0)):
        a = dict(res=3, n_faces=5, texels=texels, used=None, fill=(0.0, 0.0, 0.0))
        a.update(k)
        with pytest.raises(ValueError, match="TextureAtlas"):
            ops.TextureAtlas(**a)
    atlas = ops.TextureAtlas(3, 5, texels)
    assert atlas.block_shape == (Hb, Wb) and atlas.n_blocks == 3 and bool(atlas.used.all())
    for bw in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="blocks_per_row"):
            atlas.image(bw)
    # the front ends
    vw = MC.VIEWS_A
    K, pose = torch.from_numpy(vw["intrinsics"].copy()), torch.from_numpy(vw["pose"].copy())
    images = torch.zeros((4, 48, 64, 3))
    mesh = (verts, faces, normals)
    for res in (0, 2.0, None):
        with pytest.raises(ValueError, match="res"):
            texture_mesh(mesh, K, pose, images, (48, 64), res=res)
    with pytest.raises(ValueError, match="texture_mesh: view_bytes"):
        texture_mesh(mesh, K, pose, images, (48, 64), view_bytes=0)
    with pytest.raises(ValueError, match="texture_mesh: mode"):
        texture_mesh(mesh, K, pose, images, (48, 64), mode="mean")
    with pytest.raises(ValueError, match="texture_mesh: one image"):
        texture_mesh(mesh, K, pose, images[:3], (48, 64))
    with pytest.raises(_lib.HashmodError, match="no CPU fallback"):
        texture_mesh(mesh, K, pose, images, (48, 64), device="cpu")
    with pytest.raises(ValueError, match="texture"):
        render_mesh(mesh, K, pose, (48, 64), texture=atlas, shade="normal", device="cpu")
    with pytest.raises(ValueError, match="texture"):
        render_mesh(mesh, K, pose, (48, 64), texture=atlas, colors=torch.zeros((7, 3)), device="cpu")
    with pytest.raises(ValueError, match="texture"):
        render_mesh(mesh, K, pose, (48, 64), texture=ops.TextureAtlas(3, 6, texels), device="cpu")
    with pytest.raises(ValueError, match="texture"):
        render_mesh(mesh, K, pose, (48, 64), texture=texels, device="cpu")
    with pytest.raises(TypeError, match="unexpected"):
        evaluate_mesh_views(mesh, None, textures=atlas)


# ---------------------------------------------------------------------------------------------------------------------
# the plane property
# ---------------------------------------------------------------------------------------------------------------------
# the restatement's largest error on the interior pixels of plane_scene per res, measured on the CPU (it falls as 1 / res)
MEASURED = {1: 0.0625, 4: 0.014706, 8: 0.007353}


@pytest.mark.parametrize("n", [1, 4, 8])
def test_a_plane_with_an_affine_photograph_is_reproduced(n):
    """One fronto-parallel quad of two faces, one view, a photograph affine in the pixel coordinates: baked and drawn
    again through the restatement it shows the photograph on the interior pixels.  Not to rounding: the texel points
    are affine in the lattice and so is the photograph, so every lattice texel holds the photograph's value exactly (up
    to rounding); but a gutter texel holds the value at the nearest point of the hypotenuse, not the affine
    continuation half a cell beyond it, and a sample in a cell on the hypotenuse gives that tap the weight fx fy <= 1/4.
    The error is therefore at most a quarter of the photograph's change over half a cell diagonal and shrinks as 1/n.
    Measured on this scene with the restatement, in units of the [0, 1] image: see MEASURED; the test allows four
    times that.  The device is held to the restatement's bits (test_mesh_texture_gpu.py), so this bound never tests
    the device."""
    verts, faces, normals, vw, images = TC.plane_scene()
    texels, used, stats, _ = TC.bake_ref(verts, faces, normals, vw, images, n, erode=0)
    assert used.reshape(-1)[TC.texel_points_ref(verts, faces, n)[2] >= 0].all() and stats["n_skipped"] == (0,)
    ren = MR.renders_ref(verts, faces, vw["proj"], vw["H"], vw["W"])
    got = TC.texture_views_ref(verts, faces, vw, n, texels, render=ren)[0]
    want = TC.to_unit(images[0])
    interior = np.zeros((vw["H"], vw["W"]), bool)
    interior[6:37, 7:40] = True                          # the quad covers columns [6, 40] and rows [5, 37]
    assert (ren["face_id"][0][interior] >= 0).all() and set(ren["face_id"][0][interior].tolist()) == {0, 1}
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64))[interior].max())
    print("res", n, "largest error on the interior pixels", err)
    assert err <= 4 * MEASURED[n]

