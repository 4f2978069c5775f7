"""The mesh-culling kernels (csrc/hm_mesh_cull.hip) and evaluation.cull.cull_mesh against the numpy restatement
(tests/mesh_cull_cases.py), bit for bit: mask votes, depth maps, visibility votes, compaction, the whole."""
import numpy as np
import pytest
import torch

import mesh_cull_cases as MC
from hashmodnffbanks_idr_amd import ops
from hashmodnffbanks_idr_amd._lib import HashmodError
from hashmodnffbanks_idr_amd.evaluation import CullStats, cull_mesh
from hashmodnffbanks_idr_amd.utils.plots import TriMesh

pytestmark = pytest.mark.gpu


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()        # a copy: the cases' arrays are read-only


def _mesh(name):
    m = MC.scene(name)
    return _t(m["verts"]), _t(m["faces"]), _t(m["normals"])


def _bits(x):
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _same_mesh(got, want):
    for g, w in zip(got, want):
        if w is None:
            assert g is None
            continue
        w = np.asarray(w)
        assert g.is_cuda and tuple(g.shape) == w.shape, (g.shape, w.shape)
        assert np.array_equal(g.cpu().numpy().view(np.int32), np.ascontiguousarray(w).view(np.int32))
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32


def _vote_verts(vw):
    """the special vertices first (so that every V has them), then the nested scene's"""
    return np.concatenate([MC.special_vertices(vw), MC.scene("nested")["verts"]])


def _masks(which, kind):
    vw = MC.views(which)
    n, H, W = len(vw["proj"]), vw["H"], vw["W"]
    if kind == "zero":
        return np.zeros((n, H, W), bool)
    if kind == "one":
        return np.ones((n, H, W), bool)
    if kind == "sparse":
        return np.random.default_rng(7).random((n, H, W)) < 0.01
    return MC.shell_masks(which)


# ---------------------------------------------------------------------------------------------------------------------
# mask votes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("kind", ["zero", "one", "sparse", "shell"])
def test_mask_votes(which, kind):
    vw = MC.views(which)
    verts, masks = _vote_verts(vw), _masks(which, kind)
    for r in (0, 1, 3, 100):
        want = MC.mask_votes_ref(verts, vw["proj"], masks, r)
        got = ops.mesh_mask_votes(_t(verts), vw["proj"], _t(masks), r)
        for g, w in zip(got, want):
            assert g.dtype == torch.int32 and g.is_cuda and np.array_equal(g.cpu().numpy(), w)
    if kind == "one":
        assert np.array_equal(want[0], want[1]) and 0 < want[0].min() + 1 and want[0].max() == len(vw["proj"])
    if kind == "zero":
        assert not want[1].any() and want[0].any()


@pytest.mark.parametrize("n_verts", [0, 63, 64, 65])
def test_mask_votes_sizes_and_chunks(n_verts):
    vw = MC.views("B")
    verts, masks = _vote_verts(vw)[:n_verts], _masks("B", "sparse")
    want = MC.mask_votes_ref(verts, vw["proj"], masks, 2)
    proj = _t(vw["proj"])                                                # a device tensor is taken as it is
    for m in (_t(masks), _t(masks.astype(np.uint8) * 3)):
        for table_bytes in (1 << 28, 1):                                 # all views at once; one view per table
            got = ops.mesh_mask_votes(_t(verts.reshape(-1, 3)), proj, m, 2, table_bytes=table_bytes)
            assert got[0].shape == (n_verts,)
            assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    if n_verts == 65:
        assert want[0].max() >= 1 and 0 < want[1].sum() < want[0].sum()
        got = ops.mesh_mask_votes(_t(verts), proj[:0], _t(masks[:0]), 2)
        assert not got[0].any() and not got[1].any()


def test_mask_votes_half_pixels_and_border():
    vw = MC.axis_view()
    H, W = vw["H"], vw["W"]
    uv = [(2.5, 3.5), (3.5, 2.5), (-0.5, 0.0), (63.5, 0.0), (0.0, 47.5), (62.5, 46.5), (0.0, -0.5), (63.0, 47.0)]
    verts = np.asarray([MC.at_uv(vw, u, v) for u, v in uv] + [MC.at_uv(vw, 8.0, 4.0, -1.0), [1, 1, 0], [np.nan, 0, 1]],
                       np.float32)
    pixels = [(2, 4), (4, 2), (0, 0), None, None, (62, 46), (0, 0), (63, 47), None, None, None]   # (col, row), half to even
    n_img, _ = ops.mesh_mask_votes(_t(verts), vw["proj"], _t(np.zeros((1, H, W), bool)), 0)
    assert n_img.tolist() == [int(p is not None) for p in pixels]
    for i, p in enumerate(pixels):
        if p is None:
            continue
        for dc, dr in ((0, 0), (1, 0), (0, 1), (-1, 0)):
            c, r = p[0] + dc, p[1] + dr
            if not (0 <= c < W and 0 <= r < H):
                continue
            mask = np.zeros((1, H, W), bool)
            mask[0, r, c] = True
            for radius in (0, 1):
                want = MC.mask_votes_ref(verts, vw["proj"], mask, radius)
                got = ops.mesh_mask_votes(_t(verts), vw["proj"], _t(mask), radius)
                assert np.array_equal(got[1].cpu().numpy(), want[1])
                assert int(got[1][i]) == int((dc, dr) == (0, 0) or radius == 1)


# ---------------------------------------------------------------------------------------------------------------------
# depth maps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("name", ["sphere", "nested"])
def test_depth_maps_of_the_scenes(name, which):
    vw = MC.views(which)
    want, want_skipped = MC.scene_depth(name, which)
    verts, faces, _ = _mesh(name)
    depth, skipped = ops.mesh_depth_maps(verts, faces, vw["proj"], vw["H"], vw["W"])
    assert depth.dtype == torch.float32 and depth.shape == want.shape and skipped.dtype == torch.int32
    assert np.array_equal(_bits(depth), _bits(want)) and np.array_equal(skipped.cpu().numpy(), want_skipped)
    assert np.isfinite(want).any() and np.isinf(want).any()
    # twice; view by view; every face on the wave path; every face on the lane path
    again = ops.mesh_depth_maps(verts, faces, _t(vw["proj"]), vw["H"], vw["W"])[0]
    assert torch.equal(again.view(torch.int32), depth.view(torch.int32))
    single = torch.cat([ops.mesh_depth_maps(verts, faces, vw["proj"][k:k + 1], vw["H"], vw["W"])[0]
                        for k in range(len(vw["proj"]))])
    assert torch.equal(single.view(torch.int32), depth.view(torch.int32))
    for big_face in (1, 1 << 40):
        other = ops.mesh_depth_maps(verts, faces, vw["proj"], vw["H"], vw["W"], big_face=big_face)[0]
        assert torch.equal(other.view(torch.int32), depth.view(torch.int32))


def _single_faces():
    """name -> (verts fp32 [., 3], faces int32 [., 3]) in MC.axis_view(): uv positions at the depths 1, 2, 4"""
    vw = MC.axis_view()

    def tri(uv, z=(1.0, 2.0, 4.0), order=(0, 1, 2)):
        return (np.asarray([MC.at_uv(vw, u, v, d) for (u, v), d in zip(uv, z)], np.float32),
                np.asarray([order], np.int32))

    cases = {
        "whole_image": tri([(-100.0, -100.0), (300.0, -100.0), (-100.0, 300.0)]),           # 3072 pixels: one wave
        "straddles_border": tri([(-10.0, 5.0), (20.0, 10.0), (5.0, 60.0)]),
        "sub_pixel_no_centre": tri([(10.25, 10.25), (10.75, 10.25), (10.5, 10.75)]),
        "edges_through_centres": tri([(4.0, 4.0), (20.0, 4.0), (4.0, 20.0)]),
        "edges_through_centres_flipped": tri([(4.0, 4.0), (20.0, 4.0), (4.0, 20.0)], order=(0, 2, 1)),
        "zero_area": tri([(4.0, 4.0), (8.0, 8.0), (12.0, 12.0)]),
        "box_of_64": tri([(10.0, 10.0), (17.5, 10.25), (10.25, 17.5)]),                     # the last lane-path size
        "box_of_72": tri([(10.0, 10.0), (18.5, 10.25), (10.25, 17.5)]),                     # the first wave-path size
        "one_pixel": tri([(30.0, 30.0), (30.0, 30.0), (31.0, 30.5)], z=(2.0, 2.0, 2.0)),    # zero area as well
        "behind_camera": tri([(4.0, 4.0), (20.0, 4.0), (4.0, 20.0)], z=(1.0, 2.0, -1.0)),
        "beyond_fixed_range": tri([(4.0, 4.0), (70000.0, 4.0), (4.0, 20.0)]),
        "nan_vertex": (np.asarray([[np.nan, 0, 1], [0, 0, 1], [1, 0, 1]], np.float32), np.asarray([[0, 1, 2]], np.int32)),
        "no_faces": (tri([(4.0, 4.0), (20.0, 4.0), (4.0, 20.0)])[0], np.zeros((0, 3), np.int32)),
    }
    verts = np.concatenate([v for v, _ in cases.values()])
    faces = np.concatenate([f + 3 * i for i, (_, f) in enumerate(cases.values())]).astype(np.int32)
    cases["all_together"] = (verts, faces)
    return vw, cases


def test_depth_maps_of_single_faces():
    vw, cases = _single_faces()
    H, W = vw["H"], vw["W"]
    expect_skipped = {"behind_camera": 1, "beyond_fixed_range": 1, "nan_vertex": 1, "all_together": 3}
    for name, (verts, faces) in cases.items():
        want, want_skipped = MC.depth_maps_ref(verts, faces, vw["proj"], H, W)
        depth, skipped = ops.mesh_depth_maps(_t(verts), _t(faces), vw["proj"], H, W)
        assert np.array_equal(_bits(depth), _bits(want)), name
        assert skipped.tolist() == want_skipped.tolist() == [expect_skipped.get(name, 0)], name
        n = int(np.isfinite(want).sum())
        print(name, "pixels drawn", n)
        if name == "whole_image":
            assert n == H * W
        if name in ("sub_pixel_no_centre", "zero_area", "one_pixel", "behind_camera", "beyond_fixed_range", "nan_vertex",
                    "no_faces"):
            assert n == 0
        if name.startswith("edges_through_centres"):
            assert n == 17 * 18 // 2                       # inclusive edges: the legs and the diagonal are drawn
            assert np.array_equal(_bits(want), _bits(MC.depth_maps_ref(*cases["edges_through_centres"], vw["proj"], H,
                                                                        W)[0]))
    assert np.isfinite(MC.depth_maps_ref(*cases["straddles_border"], vw["proj"], H, W)[0][0, :, 0]).any()


def test_depth_maps_refuse_a_bad_index():
    verts, faces, _ = _mesh("sphere")
    vw = MC.views("A")
    for bad in (-1, len(verts)):
        f = faces.clone()
        f[5, 1] = bad
        with pytest.raises(HashmodError, match="face index"):
            ops.mesh_depth_maps(verts, f, vw["proj"], vw["H"], vw["W"])
    depth, skipped = ops.mesh_depth_maps(verts, faces, vw["proj"][:0], vw["H"], vw["W"])
    assert depth.shape == (0, vw["H"], vw["W"]) and skipped.shape == (0,)
    depth, skipped = ops.mesh_depth_maps(verts[:0], faces[:0], vw["proj"], vw["H"], vw["W"])
    assert torch.isinf(depth).all() and not skipped.any()


# ---------------------------------------------------------------------------------------------------------------------
# visibility votes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("name", ["sphere", "nested"])
def test_visible_votes(name, which):
    vw = MC.views(which)
    depth = MC.scene_depth(name, which)[0]
    verts = np.concatenate([MC.scene(name)["verts"], MC.special_vertices(vw)])
    d_verts, d_depth = _t(verts), _t(depth)
    for pad in (0, 1, 2):
        for tol in (0.0, 0.5 * MC.SPACING):
            want = MC.visible_votes_ref(verts, vw["proj"], depth, pad, tol)
            got = ops.mesh_visible_votes(d_verts, vw["proj"], d_depth, pad, tol)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (pad, tol)
    assert 0 < (want > 0).sum() < len(verts)
    # accumulated over chunks of views
    acc = torch.zeros(len(verts), dtype=torch.int32, device="cuda")
    for k in range(len(vw["proj"])):
        out = ops.mesh_visible_votes(d_verts, vw["proj"][k:k + 1], d_depth[k:k + 1], 2, 0.5 * MC.SPACING, out=acc)
        assert out is acc
    assert np.array_equal(acc.cpu().numpy(), want)
    assert ops.mesh_visible_votes(d_verts[:0], vw["proj"], d_depth).shape == (0,)


# ---------------------------------------------------------------------------------------------------------------------
# compaction
# ---------------------------------------------------------------------------------------------------------------------
def test_keep_vertices():
    m = MC.scene("nested")
    verts, faces, normals = _mesh("nested")
    rng = np.random.default_rng(11)
    for keep in (np.zeros(len(m["verts"]), bool), np.ones(len(m["verts"]), bool), rng.random(len(m["verts"])) < 0.85,
                 MC.radius_of(m["verts"]) > 0.5):
        want = MC.keep_vertices_ref(m["verts"], m["faces"], m["normals"], keep)
        _same_mesh(ops.mesh_keep_vertices(verts, faces, normals, _t(keep)), want)
        got = ops.mesh_keep_vertices(verts, faces, None, _t(keep))
        assert got[2] is None
        _same_mesh(got[:2], want[:2])
    got = ops.mesh_keep_vertices(verts, faces, normals, _t(np.ones(len(m["verts"]), bool)))
    assert all(torch.equal(g, w) for g, w in zip(got, (verts, faces, normals)))            # keep all: the mesh itself
    for bad in (-1, len(m["verts"])):
        f = faces.clone()
        f[7, 2] = bad
        with pytest.raises(HashmodError, match="face index"):
            ops.mesh_keep_vertices(verts, f, normals, _t(np.ones(len(m["verts"]), bool)))
    empty = ops.mesh_keep_vertices(verts[:0], faces[:0], None, torch.zeros(0, dtype=torch.bool, device="cuda"))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the whole
# ---------------------------------------------------------------------------------------------------------------------
def _cameras(vw):
    return _t(vw["intrinsics"]), _t(vw["pose"])


def _stats_equal(stats, want):
    assert isinstance(stats, CullStats)
    for k, v in want.items():
        assert getattr(stats, k) == v, (k, getattr(stats, k), v)


def test_cull_mesh_removes_the_inside():
    vw, m = MC.views("A"), MC.scene("nested")
    want, want_stats = MC.nested_cull_reference("A", 1)
    K, pose = _cameras(vw)
    masks = _t(MC.shell_masks("A"))
    got, stats = cull_mesh(_mesh("nested"), K, pose, masks, (vw["H"], vw["W"]), dilate=1)
    _same_mesh(got, want)
    _stats_equal(stats, want_stats)
    out = got[0].cpu().numpy()
    assert MC.radius_of(out).min() > 0.7                     # the inner sphere and the shell's inner wall are gone
    have = {tuple(v) for v in out.view(np.int32).tolist()}
    v = m["verts"].astype(np.float64)
    outer = MC.radius_of(v) > 0.7
    for k, P in enumerate(vw["proj"]):                       # the outer wall's front of every view is all there
        front = outer & (((vw["eyes"][k] - v) * v).sum(1) > 0)
        assert front.sum() > 500 and all(tuple(x) in have for x in m["verts"][front].view(np.int32).tolist())
    # the same through small chunks of views, a flat mask layout and a TriMesh
    got2, stats2 = cull_mesh(_mesh("nested"), K, pose, masks.reshape(len(masks), -1), (vw["H"], vw["W"]), dilate=1,
                             depth_bytes=1)
    _same_mesh(got2, want)
    assert stats2 == stats
    got3, stats3 = cull_mesh(TriMesh(m["verts"], m["faces"], m["normals"]), K, pose, masks, (vw["H"], vw["W"]),
                             dilate=1)
    _same_mesh(got3, want)
    assert stats3 == stats


def test_cull_mesh_rules():
    vw, m = MC.views("B"), MC.scene("nested")
    K, pose = _cameras(vw)
    res = (vw["H"], vw["W"])
    # the sphere's silhouette as the masks: the rim of the shell falls outside it
    masks = np.isfinite(MC.scene_depth("sphere", "B")[0])
    masks[1] = False
    for rule, min_views in (("all", None), ("min", 3), ("min", 0)):
        want, want_stats = MC.cull_ref(m["verts"], m["faces"], m["normals"], vw, masks, 2, rule, min_views,
                                       visibility=False)
        got, stats = cull_mesh(_mesh("nested"), K, pose, _t(masks), res, dilate=2, mask_rule=rule, min_views=min_views,
                               visibility=False)
        _same_mesh(got, want)
        _stats_equal(stats, want_stats)
        print(rule, min_views, stats)
    assert stats.kept_by_masks == len(m["verts"]) and stats.kept_by_visibility is None and stats.n_skipped is None
    want, want_stats = MC.cull_ref(m["verts"], m["faces"], m["normals"], vw, masks, 2, "min", 3, visibility=False)
    assert 0 < want_stats["kept_by_masks"] < len(m["verts"])
    # no masks: visibility alone; then the largest component of that
    want, want_stats = MC.cull_ref(m["verts"], m["faces"], m["normals"], vw, None, 0)
    got, stats = cull_mesh(_mesh("nested")[:2], K, pose, None, res, dilate=0)
    _same_mesh(got, want[:2] + (None,))
    _stats_equal(stats, want_stats)
    assert stats.kept_by_masks is None and got[2] is None
    # a mesh of two components after culling: the outer wall and a far-away copy of a few of its faces
    verts, faces, normals = _mesh("nested")
    verts2 = torch.cat([verts, verts[:300] * 0.1 + 0.88])
    faces2 = torch.cat([faces, faces[(faces < 300).all(1)] + len(verts)])
    normals2 = torch.cat([normals, normals[:300]])
    plain, _ = cull_mesh((verts2, faces2, normals2), K, pose, None, res, dilate=0)
    largest, stats = cull_mesh((verts2, faces2, normals2), K, pose, None, res, dilate=0, largest_component=True)
    want = ops.mesh_largest_component(*plain)
    assert all(torch.equal(g, w) for g, w in zip(largest, want))
    assert stats.n_verts_out == len(want[0]) < len(plain[0])
