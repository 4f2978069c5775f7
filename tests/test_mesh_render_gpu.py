"""The mesh renderer (csrc/hm_mesh_render.hip, ops.mesh_render) against its numpy restatement
(tests/mesh_render_cases.py) bit for bit, and evaluation.mesh_views on top of it.  Images of 48 x 64, 45 x 67, 1 x 5."""
import math
import os

import numpy as np
import pytest
import torch

import mesh_cull_cases as MC
import mesh_render_cases as MR
from hashmodnffbanks_idr_amd import ops
from hashmodnffbanks_idr_amd._lib import HashmodError
from hashmodnffbanks_idr_amd.evaluation import MeshViews, evaluate_mesh_views, render_mesh
from hashmodnffbanks_idr_amd.utils.plots import TriMesh

pytestmark = pytest.mark.gpu

BG = (-1.0, 0.5, 2.0)               # scene_render's background


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()        # a copy: the cases' arrays are read-only


def _mesh(name):
    m = MC.scene(name)
    return _t(m["verts"]), _t(m["faces"])


def _bits(x):
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.int32) if x.dtype == np.float32 else np.ascontiguousarray(x)


def _same(got, want, what=""):
    """every output of a MeshRender equal to the restatement's, floats by their bits (a NaN equals itself)"""
    assert got.face_id.dtype == torch.int32 and got.depth.dtype == torch.float32 and got.n_skipped.dtype == torch.int32
    for k in ("face_id", "depth", "weights", "image", "n_skipped"):
        g, w = getattr(got, k), want[k]
        if w is None:
            assert g is None, (what, k)
            continue
        assert g.is_cuda and tuple(g.shape) == w.shape, (what, k, g.shape, w.shape)
        assert np.array_equal(_bits(g), _bits(w)), (what, k)


def _same_render(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("name", ["sphere", "nested"])
def test_render_of_the_scenes(name, which):
    vw = MC.views(which)
    H, W = vw["H"], vw["W"]
    want = MR.scene_render(name, which)
    verts, faces = _mesh(name)
    got = ops.mesh_render(verts, faces, vw["proj"], H, W, attrs=verts, background=BG, return_weights=True)
    _same(got, want, (name, which))
    assert (want["face_id"] >= 0).any() and (want["face_id"] < 0).any()
    depth, skipped = ops.mesh_depth_maps(verts, faces, vw["proj"], H, W)
    assert torch.equal(got.depth.view(torch.int32), depth.view(torch.int32)) and torch.equal(got.n_skipped, skipped)
    # twice (a device projection this time); every face on the wave path; every face on the lane path
    again = ops.mesh_render(verts, faces, _t(vw["proj"]), H, W, attrs=verts, background=BG, return_weights=True)
    _same_render(again, got)
    for big_face in (1, 1 << 40):
        other = ops.mesh_render(verts, faces, vw["proj"], H, W, attrs=verts, background=BG, big_face=big_face,
                                return_weights=True)
        _same_render(other, got)
    # without weights, without attributes
    bare = ops.mesh_render(verts, faces, vw["proj"], H, W)
    assert bare.weights is None and bare.image is None
    assert torch.equal(bare.face_id, got.face_id)
    assert torch.equal(bare.depth.view(torch.int32), got.depth.view(torch.int32))


def test_render_does_not_depend_on_the_order_of_the_faces():
    vw, m = MC.views("A"), MC.scene("sphere")
    H, W = vw["H"], vw["W"]
    perm = np.random.default_rng(5).permutation(len(m["faces"]))
    faces = np.ascontiguousarray(m["faces"][perm])
    want = MR.renders_ref(m["verts"], faces, vw["proj"], H, W, m["verts"], BG)
    got = ops.mesh_render(_t(m["verts"]), _t(faces), vw["proj"], H, W, attrs=_t(m["verts"]), background=BG,
                          return_weights=True)
    _same(got, want, "permuted")
    base = MR.scene_render("sphere", "A")
    assert np.array_equal(_bits(want["depth"]), _bits(base["depth"]))
    on = base["face_id"] >= 0
    ties = perm[want["face_id"][on]] != base["face_id"][on]            # another face of the same depth took the pixel
    print("pixels whose winner changed with the order (equal depths):", int(ties.sum()), "of", int(on.sum()))


# ---------------------------------------------------------------------------------------------------------------------
# hand-made faces
# ---------------------------------------------------------------------------------------------------------------------
def _single_faces():
    """name -> (verts fp32 [., 3], faces int32 [., 3]) in MC.axis_view(): uv positions at the depths 1, 2, 4"""
    vw = MC.axis_view()

    def tri(uv, z=(1.0, 2.0, 4.0), order=(0, 1, 2)):
        return (np.asarray([MC.at_uv(vw, u, v, d) for (u, v), d in zip(uv, z)], np.float32),
                np.asarray([order], np.int32))

    cases = {
        "whole_image": tri([(-100.0, -100.0), (300.0, -100.0), (-100.0, 300.0)]),
        "straddles_border": tri([(-10.0, 5.0), (20.0, 10.0), (5.0, 60.0)]),
        "between_centres": tri([(10.25, 10.25), (10.75, 10.25), (10.5, 10.75)]),
        "edges_through_centres": tri([(4.0, 4.0), (20.0, 4.0), (4.0, 20.0)]),
        "zero_area": tri([(4.0, 4.0), (8.0, 8.0), (12.0, 12.0)]),
        "box_of_64": tri([(10.0, 10.0), (17.5, 10.25), (10.25, 17.5)]),                     # the last lane-path size
        "box_of_72": tri([(10.0, 10.0), (18.5, 10.25), (10.25, 17.5)]),                     # the first wave-path size
        "behind_camera": tri([(4.0, 4.0), (20.0, 4.0), (4.0, 20.0)], z=(1.0, 2.0, -1.0)),
        "nan_vertex": (np.asarray([[np.nan, 0, 1], [0, 0, 1], [1, 0, 1]], np.float32),
                       np.asarray([[0, 1, 2]], np.int32)),
    }
    for name, (verts, faces, _) in MR.tie_cases()[1].items():
        cases[name] = (verts, faces)
    verts = np.concatenate([v for v, _ in cases.values()])
    offsets = np.cumsum([0] + [len(v) for v, _ in cases.values()])
    faces = np.concatenate([f + o for (_, f), o in zip(cases.values(), offsets)]).astype(np.int32)
    cases["all_together"] = (verts, faces)
    return vw, cases


def test_render_of_single_faces():
    vw, cases = _single_faces()
    H, W = vw["H"], vw["W"]
    expect_skipped = {"behind_camera": 1, "nan_vertex": 1, "all_together": 2}
    for name, (verts, faces) in cases.items():
        attrs = np.stack([verts[:, 2], np.arange(len(verts), dtype=np.float32)], 1)
        want = MR.renders_ref(verts, faces, vw["proj"], H, W, attrs, (3.0, -3.0))
        for big_face in (64, 1, 1 << 40):
            got = ops.mesh_render(_t(verts), _t(faces), vw["proj"], H, W, attrs=_t(attrs), background=(3.0, -3.0),
                                  big_face=big_face, return_weights=True)
            _same(got, want, (name, big_face))
        assert got.n_skipped.tolist() == [expect_skipped.get(name, 0)], name
        n = int((want["face_id"] >= 0).sum())
        print(name, "pixels drawn", n)
        if name == "whole_image":
            assert n == H * W
        if name in ("between_centres", "zero_area", "behind_camera", "nan_vertex"):
            assert n == 0
        if name == "edges_through_centres":
            assert n == 17 * 18 // 2
        if name == "straddles_border":
            assert (want["face_id"][0, :, 0] >= 0).any()
        if name.startswith("coincident"):
            assert set(np.unique(want["face_id"])) == {-1, 0}
        if name.startswith("shared_edge"):
            assert (want["face_id"][0][MR.tie_cases()[1][name][2]] == 0).all()


@pytest.mark.parametrize("H,W", [(45, 67), (1, 5)])
def test_render_of_odd_images(H, W):
    """rows of 67 pixels are not a multiple of the wave; an image of one row"""
    vw = MC.axis_view(H, W)
    verts = np.asarray([MC.at_uv(vw, -3.0, -2.0, 1.0), MC.at_uv(vw, 80.0, -1.0, 2.0), MC.at_uv(vw, 2.0, 70.0, 4.0),
                        MC.at_uv(vw, 1.0, 0.0, 1.0), MC.at_uv(vw, 4.0, 0.0, 1.0), MC.at_uv(vw, 2.0, 0.5, 1.0)],
                       np.float32)
    faces = np.asarray([[0, 1, 2], [3, 4, 5]], np.int32)
    want = MR.renders_ref(verts, faces, vw["proj"], H, W, verts, 0.25)
    assert set(np.unique(want["face_id"])) >= {0, 1}
    for big_face in (64, 1, 1 << 40):
        got = ops.mesh_render(_t(verts), _t(faces), vw["proj"], H, W, attrs=_t(verts), background=0.25,
                              big_face=big_face, return_weights=True)
        _same(got, want, (H, W, big_face))


@pytest.mark.parametrize("C", [0, 1, 3, 16])
def test_render_attribute_counts(C):
    vw, m = MC.views("B"), MC.scene("sphere")
    H, W = vw["H"], vw["W"]
    rng = np.random.default_rng(C)
    attrs = rng.standard_normal((len(m["verts"]), C)).astype(np.float32)
    bg = rng.standard_normal(C).astype(np.float32)
    if C == 3:
        attrs[m["faces"][MR.scene_render("sphere", "B")["face_id"][0, H // 2, W // 2]][0], 1] = np.nan
    want = MR.renders_ref(m["verts"], m["faces"], vw["proj"][:2], H, W, attrs, bg)
    got = ops.mesh_render(*_mesh("sphere"), vw["proj"][:2], H, W, attrs=_t(attrs), background=bg.tolist(),
                          return_weights=True)
    assert got.image.shape == (2, H, W, C)
    _same(got, want, C)
    if C == 3:
        assert np.isnan(want["image"][0, H // 2, W // 2, 1]) and not np.isnan(want["image"][..., [0, 2]]).any()
        off = want["face_id"] < 0
        assert np.array_equal(want["image"][off], np.broadcast_to(bg, (int(off.sum()), 3)))


def test_render_of_nothing_and_a_bad_index():
    verts, faces = _mesh("sphere")
    vw = MC.views("A")
    H, W = vw["H"], vw["W"]
    for bad in (-1, len(verts)):
        f = faces.clone()
        f[5, 1] = bad
        with pytest.raises(HashmodError, match="face index"):
            ops.mesh_render(verts, f, vw["proj"], H, W, attrs=verts)
    none = ops.mesh_render(verts, faces, vw["proj"][:0], H, W, attrs=verts, return_weights=True)
    assert none.face_id.shape == (0, H, W) and none.depth.shape == (0, H, W) and none.weights.shape == (0, H, W, 3)
    assert none.image.shape == (0, H, W, 3) and none.n_skipped.shape == (0,)
    empty = ops.mesh_render(verts, faces[:0], vw["proj"], H, W, attrs=verts, background=BG, return_weights=True)
    assert (empty.face_id == -1).all() and torch.isinf(empty.depth).all() and not empty.weights.any()
    assert torch.equal(empty.image, torch.tensor(BG, device="cuda").expand(len(vw["proj"]), H, W, 3))
    assert not empty.n_skipped.any()
    empty = ops.mesh_render(verts[:0], faces[:0], vw["proj"], H, W)
    assert (empty.face_id == -1).all() and empty.image is None


# ---------------------------------------------------------------------------------------------------------------------
# evaluation.mesh_views
# ---------------------------------------------------------------------------------------------------------------------
def _cameras(vw):
    return _t(vw["intrinsics"]), _t(vw["pose"])


def test_render_mesh_shades():
    vw, m = MC.views("A"), MC.scene("sphere")
    H, W = vw["H"], vw["W"]
    K, pose = _cameras(vw)
    mesh = (_t(m["verts"]), _t(m["faces"]), _t(m["normals"]))
    attrs = (m["normals"] + np.float32(1.0)) / np.float32(2.0)
    want = MR.renders_ref(m["verts"], m["faces"], vw["proj"], H, W, attrs, (1.0, 0.0, 0.5))
    got = render_mesh(mesh, K, pose, (H, W), shade="normal", background=(1.0, 0.0, 0.5))
    assert isinstance(got, MeshViews) and got.rgb.dtype == torch.float32 and got.coverage.dtype == torch.bool
    assert np.array_equal(_bits(got.rgb), _bits(np.clip(want["image"], 0.0, 1.0)))
    assert np.array_equal(got.coverage.cpu().numpy(), want["face_id"] >= 0)
    assert np.array_equal(got.face_id.cpu().numpy(), want["face_id"]) and got.n_skipped.tolist() == [0] * 4
    assert np.array_equal(_bits(got.depth), _bits(want["depth"]))
    one = render_mesh(mesh, K, pose, (H, W), shade="normal", background=(1.0, 0.0, 0.5), view_bytes=1)
    assert all(torch.equal(a, b) for a, b in zip(one, got))
    # the colours: fp32 in [-1, 1], and a TriMesh's bytes
    colors = _t(np.clip(m["verts"] / 0.6, -1.0, 1.0).astype(np.float32))
    col = render_mesh(mesh[:2], K, pose, (H, W), colors=colors)
    want = MR.renders_ref(m["verts"], m["faces"], vw["proj"], H, W, ((colors + 1.0) / 2.0).cpu().numpy(), 1.0)
    assert np.array_equal(_bits(col.rgb), _bits(np.clip(want["image"], 0.0, 1.0)))
    one = render_mesh(mesh[:2], K, pose, (H, W), colors=colors, view_bytes=1)
    assert all(torch.equal(a, b) for a, b in zip(one, col))
    bytes_ = np.rint((colors.cpu().numpy() + 1.0) * 127.5).astype(np.uint8)
    tm = render_mesh(TriMesh(m["verts"], m["faces"], vertex_colors=bytes_), K, pose, (H, W))
    assert torch.equal(tm.face_id, col.face_id) and (tm.rgb - col.rgb).abs().max() <= 0.5 / 255 + 1e-6
    # the depth: in (0, 1] on the mesh, 1 at the farthest covered pixel of every view, the background elsewhere
    dep = render_mesh(mesh, K, pose, (H, W), shade="depth", background=0.0)
    on = dep.coverage
    assert torch.equal(dep.depth.view(torch.int32), got.depth.view(torch.int32)) and torch.equal(on, got.coverage)
    far = torch.where(on, dep.depth, torch.zeros_like(dep.depth)).amax(dim=(1, 2), keepdim=True)
    assert torch.equal(dep.rgb[..., 0][on], (dep.depth / far)[on]) and not dep.rgb[~on].any()
    assert (dep.rgb.amax(dim=(1, 2, 3)) == 1.0).all() and torch.equal(dep.rgb[..., 0], dep.rgb[..., 2])
    assert all(torch.equal(a, b) for a, b in zip(render_mesh(mesh, K, pose, (H, W), shade="depth", background=0.0,
                                                             view_bytes=1), dep))
    for bad in (dict(shade="phong"), dict(view_bytes=0), dict(background=(1.0, 2.0))):
        with pytest.raises(ValueError):
            render_mesh(mesh, K, pose, (H, W), **{"shade": "normal", **bad})
    with pytest.raises(ValueError, match="normals"):
        render_mesh(mesh[:2], K, pose, (H, W), shade="normal")
    with pytest.raises(ValueError, match="colors"):
        render_mesh(mesh, K, pose, (H, W))


class _StubDataset:
    """what evaluate_mesh_views reads of a SceneDataset: per-view lists on the host"""

    def __init__(self, vw, images, masks):
        self.img_res = (vw["H"], vw["W"])
        self.intrinsics_all = [torch.from_numpy(k.copy()) for k in vw["intrinsics"]]
        self.pose_all = [torch.from_numpy(p.copy()) for p in vw["pose"]]
        self.rgb_images = [im.reshape(-1, 3).cpu() for im in images]
        self.object_masks = [mk.reshape(-1).cpu() for mk in masks]


def test_evaluate_mesh_views_scores_a_known_shift(tmp_path):
    """The photographs are the mesh's own render in [-1, 1] plus delta = 0.1 inside the mask, so every view's squared
    error in [0, 1] units is (delta / 2)^2 on every pixel and channel of the mask: PSNR = 20 log10(2 / delta).  The fp32
    roundings: 2 rgb - 1, + delta, and view_metrics' (v + 1) / 2 of both images each move a value of size <= 2 by at
    most 2^-24, so the difference of 0.05 is off by at most 4 * 2^-24 = 2.4e-7, 5e-6 of itself, and the PSNR by
    20 log10(1 + 5e-6) = 4e-5 dB at worst (about 2e-5 dB when the errors do not all line up); the bound is 1e-3 dB."""
    vw, m = MC.views("A"), MC.scene("sphere")
    H, W = vw["H"], vw["W"]
    K, pose = _cameras(vw)
    mesh = (_t(m["verts"]), _t(m["faces"]))
    colors = _t(np.clip(m["verts"] / 0.7, -0.85, 0.85).astype(np.float32))      # rgb in [0.075, 0.925]: nothing clamps
    own = render_mesh(mesh, K, pose, (H, W), colors=colors)
    delta = 0.1
    masks = torch.zeros((4, H, W), dtype=torch.bool, device="cuda")
    masks[:, 6:40, 10:50] = True                                                 # covered and uncovered (white) pixels
    assert (masks & own.coverage).any() and (masks & ~own.coverage).any()
    images = own.rgb * 2.0 - 1.0 + delta * masks[..., None]
    data = _StubDataset(vw, images, masks)
    indices = [2, 0, 3]
    scores = evaluate_mesh_views(mesh, data, indices=indices, out_dir=str(tmp_path), save_png=True, colors=colors)
    print(scores)
    want = 20.0 * math.log10(2.0 / delta)
    assert scores.indices == indices and len(scores.psnrs) == len(scores.ssims) == 3
    assert all(abs(p - want) <= 1e-3 for p in scores.psnrs) and abs(scores.psnr_mean - want) <= 1e-3
    assert all(0.5 < s < 1.0 for s in scores.ssims)
    for name, values, mean in (("mesh_psnrs.csv", scores.psnrs, scores.psnr_mean),
                               ("mesh_ssims.csv", scores.ssims, scores.ssim_mean)):
        lines = (tmp_path / name).read_text().splitlines()
        assert lines[0] == ",0" and len(lines) == len(indices) + 2
        assert lines[1:] == [f"{k},{v!r}" for k, v in enumerate(values + [mean])]
    assert sorted(os.listdir(tmp_path)) == ["mesh_0.png", "mesh_2.png", "mesh_3.png", "mesh_psnrs.csv",
                                            "mesh_ssims.csv"]
    from PIL import Image
    png = np.asarray(Image.open(tmp_path / "mesh_2.png"))
    assert png.shape == (H, W, 3) and np.array_equal(png, (own.rgb[2] * 255.0).round().to(torch.uint8).cpu().numpy())
    # all views, through chunks of one view: the same scores
    every = evaluate_mesh_views(mesh, data, colors=colors, view_bytes=1)
    assert every.indices == [0, 1, 2, 3] and [every.psnrs[i] for i in indices] == scores.psnrs
    assert [every.ssims[i] for i in indices] == scores.ssims
    with pytest.raises(ValueError, match="no view"):
        evaluate_mesh_views(mesh, data, indices=[], colors=colors)
    with pytest.raises(TypeError, match="shade"):
        evaluate_mesh_views(mesh, data, colors=colors, shade="normal")
