"""The numpy restatement of the mesh-culling kernels (tests/mesh_cull_cases.py) against independent truths, so that the
GPU tests, which compare the kernels with it bit for bit, cannot pass vacuously; the new entry points' ABI and argument
checks; and the property of the contract that makes pad = 1 the default (runs anywhere)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import mc_ref
import mesh_cull_cases as MC
from hashmodnffbanks_idr_amd import _lib, ops
from hashmodnffbanks_idr_amd.evaluation import cull_mesh, view_projections

NEW_SYMBOLS = {
    "hm_mesh_mask_votes": (C.c_int, 12),
    "hm_mesh_depth_workspace_bytes": (C.c_int64, 2),
    "hm_mesh_depth_maps": (C.c_int, 15),
    "hm_mesh_visible_votes": (C.c_int, 12),
    "hm_mesh_keep_mark": (C.c_int, 8),
}


# ---------------------------------------------------------------------------------------------------------------------
# independent truths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1, 3, 100])
def test_dilation_is_scipy_binary_dilation(r):
    from scipy.ndimage import binary_dilation
    rng = np.random.default_rng(r)
    for H, W in ((48, 64), (45, 67), (1, 5)):
        for density in (0.002, 0.05):
            m = rng.random((H, W)) < density
            m[0, 0] = m[H - 1, W - 1] = True          # the corners: the zero border matters
            want = binary_dilation(m, structure=np.ones((2 * r + 1, 2 * r + 1), bool), border_value=0) if r else m
            assert np.array_equal(MC.dilate_ref(m, r), want)
    assert not MC.dilate_ref(np.zeros((5, 7), bool), 100).any() and MC.dilate_ref(np.eye(5, 7), 100).all()


def test_scenes_are_closed_surfaces():
    for name, n_surfaces in (("sphere", 1), ("nested", 3)):
        m = MC.scene(name)
        assert mc_ref.edge_check(m["faces"]) == (True, True)
        assert mc_ref.euler(m["verts"], m["faces"]) == 2 * n_surfaces
    r = MC.radius_of(MC.scene("nested")["verts"])
    assert ((r < 0.5).sum(), ((r > 0.5) & (r < 0.7)).sum(), (r > 0.7).sum()) == (192, 1032, 1392)


@pytest.mark.parametrize("which", ["A", "B"])
def test_sphere_depth_is_the_ray_sphere_depth(which):
    """The issue's bound is one lattice spacing, measured on a 32^3 lattice; at 24^3 the pixels next to the silhouette
    need a derived one.  The mesh lies between the spheres of radius R - delta and R: a vertex is the zero of the linear
    interpolant of r - R along a lattice edge, r is convex along a line with r'' <= 1/r <= 1/(R - h) there, so the vertex is
    inside the sphere by at most h^2/(8 (R - h)); a face lies in one cell, so it is a chord of at most sqrt(3) h, whose
    sagitta is at most R - sqrt(R^2 - 3 h^2/4).  A ray with impact parameter b <= R - delta therefore meets the mesh
    between its entry points into the two spheres, sqrt(R^2 - b^2) - sqrt((R - delta)^2 - b^2) apart (0.07 h at the
    centre, sqrt(2 R delta) = 1.03 h at b = R - delta); a ray with b > R - delta meets it somewhere on its chord of the
    outer sphere, 2 sqrt(R^2 - b^2) <= 2.05 h long.  Depth along the camera's z is shorter than along the ray."""
    vw = MC.views(which)
    depth, skipped = MC.scene_depth("sphere", which)
    assert not skipped.any()
    R, h = MC.SPHERE_R, MC.SPACING
    delta = h * h / (8 * (R - h)) + (R - np.sqrt(R * R - 0.75 * h * h)) + 1e-6      # + the fp32 coordinates
    for k in range(len(vw["proj"])):
        want = MC.sphere_depth_analytic(vw, k)
        fa, fd = np.isfinite(want), np.isfinite(depth[k])
        # coverage differs only next to the silhouette: within one pixel of a change of the analytic coverage
        grown, shrunk = MC.dilate_ref(fa, 1), ~MC.dilate_ref(~fa, 1)
        assert not ((fa != fd) & ~(grown & ~shrunk)).any()
        assert not (fd & ~fa).any()                                                   # the mesh is inside the sphere
        # the impact parameter of every pixel's ray, from the analytic depth of the sphere's centre plane
        o = vw["pose"][k][:3, 3].astype(np.float64)
        K, pose = vw["intrinsics"][k].astype(np.float64), vw["pose"][k].astype(np.float64)
        col, row = np.meshgrid(np.arange(vw["W"], dtype=np.float64), np.arange(vw["H"], dtype=np.float64))
        d = np.stack([(col - K[0, 2]) / K[0, 0], (row - K[1, 2]) / K[1, 1], np.ones_like(col)], -1) @ pose[:3, :3].T
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        b = np.linalg.norm(np.cross(d, -o), axis=-1)
        with np.errstate(invalid="ignore"):
            bound = np.where(b <= R - delta, np.sqrt(R * R - b * b) - np.sqrt((R - delta) ** 2 - b * b),
                             2 * np.sqrt(np.maximum(R * R - b * b, 0)))
        both = fa & fd
        diff = np.abs(np.where(both, depth[k], 0).astype(np.float64) - np.where(both, want, 0))
        err = diff[both]
        print(which, k, "coverage differs in", int((fa != fd).sum()), "pixels; largest error", err.max() / h,
              "spacings; pixels above one spacing:", int((err > h).sum()), "of", int(both.sum()))
        assert both.sum() > 300 and np.all(err <= bound[both] + 1e-6)
        inner = both & (b <= R - 0.1)                # away from the rim the issue's bound holds with room to spare
        assert diff[inner].max() <= h


def test_compaction_is_numpy_unique():
    m = MC.scene("nested")
    rng = np.random.default_rng(3)
    for keep in (rng.random(len(m["verts"])) < 0.8, np.ones(len(m["verts"]), bool), np.zeros(len(m["verts"]), bool)):
        v, f, n = MC.keep_vertices_ref(m["verts"], m["faces"], m["normals"], keep)
        alive = keep[m["faces"]].all(1)
        ids, inv = np.unique(m["faces"][alive], return_inverse=True)
        assert np.array_equal(v, m["verts"][ids]) and np.array_equal(n, m["normals"][ids])
        assert np.array_equal(f, inv.reshape(-1, 3)) and f.dtype == np.int32
    assert np.array_equal(v, np.zeros((0, 3))) and f.shape == (0, 3)
    assert MC.keep_vertices_ref(m["verts"], m["faces"], None, keep)[2] is None


def test_projection_conventions():
    vw = MC.axis_view()
    # half to even, exactly: u = 2.5 -> 2, 3.5 -> 4; the image border: -0.5 -> 0 (in), W - 0.5 -> W (out)
    pts = np.asarray([MC.at_uv(vw, 2.5, 3.5), MC.at_uv(vw, 3.5, 2.5), MC.at_uv(vw, -0.5, 0.0), MC.at_uv(vw, 63.5, 0.0),
                      MC.at_uv(vw, 0.0, 47.5), MC.at_uv(vw, 62.5, 46.5), MC.at_uv(vw, 8.0, 4.0, -1.0), [1, 1, 0],
                      [np.nan, 0, 1]], np.float32)
    u, v, w, ok = MC.project_ref(pts, vw["proj"][0])
    assert u[:6].tolist() == [2.5, 3.5, -0.5, 63.5, 0.0, 62.5] and v[:6].tolist() == [3.5, 2.5, 0.0, 0.0, 47.5, 46.5]
    col, row, inside = MC.pixel_ref(u, v, ok, vw["H"], vw["W"])
    assert inside.tolist() == [True, True, True, False, False, True, False, False, False]
    assert col[:3].tolist() == [2, 4, 0] and row[:2].tolist() == [4, 2] and (col[5], row[5]) == (62, 46)
    assert ok.tolist() == [True] * 6 + [False] * 3 and w[7] == 0
    X, Y, valid = MC.fixed_ref(u, v, ok)
    assert X[:2].tolist() == [640, 896] and valid[:6].all() and not valid[6:].any()
    far = np.asarray([MC.at_uv(vw, 65535.0, 0.0), MC.at_uv(vw, 65537.0, 0.0), MC.at_uv(vw, 0.0, -65537.0)], np.float32)
    assert MC.fixed_ref(*MC.project_ref(far, vw["proj"][0])[:2], np.ones(3, bool))[2].tolist() == [True, False, False]
    # the special vertices of the look_at views cover every class
    sp = MC.special_vertices(MC.VIEWS_A)
    u, v, w, ok = MC.project_ref(sp, MC.VIEWS_A["proj"][0])
    inside = MC.pixel_ref(u, v, ok, 48, 64)[2]
    assert 10 <= inside.sum() <= len(sp) - 10 and (~ok).sum() >= 6 and (ok & ~inside).sum() >= 6
    # view_projections is the cases' projection
    for vw in (MC.VIEWS_A, MC.VIEWS_B):
        P = view_projections(torch.from_numpy(vw["intrinsics"].copy()), torch.from_numpy(vw["pose"].copy()))
        assert P.dtype == np.float64 and np.array_equal(P, vw["proj"])
    assert view_projections(np.zeros((0, 4, 4)), np.zeros((0, 4, 4))).shape == (0, 3, 4)


# ---------------------------------------------------------------------------------------------------------------------
# the property of the contract (it carries over to the device through the bit-exact GPU tests)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B"])
def test_pad_one_keeps_every_front_facing_vertex(which):
    m, vw = MC.scene("sphere"), MC.views(which)
    depth, _ = MC.scene_depth("sphere", which)
    v = m["verts"].astype(np.float64)
    lost0 = 0
    for k, P in enumerate(vw["proj"]):
        front = ((vw["eyes"][k] - v) * v).sum(1) > 0
        u, vv, w, ok = MC.project_ref(m["verts"], P)
        inside = MC.pixel_ref(u, vv, ok, vw["H"], vw["W"])[2]
        assert (front & inside).sum() > 300
        assert not (front & inside & ~MC.visible_ref(m["verts"], P, depth[k], 1, 0.0)).any()
        lost0 += int((front & inside & ~MC.visible_ref(m["verts"], P, depth[k], 0, 0.0)).sum())
        assert not MC.visible_ref(m["verts"], P, depth[k], 1, 0.0).all()          # the far side is hidden
    assert lost0 > 100                                                             # why pad = 0 is not the default


@pytest.mark.parametrize("which", ["A", "B"])
def test_no_inner_vertex_is_visible(which):
    m, vw = MC.scene("nested"), MC.views(which)
    depth, skipped = MC.scene_depth("nested", which)
    n_vis = MC.visible_votes_ref(m["verts"], vw["proj"], depth, 1, 0.0)
    r = MC.radius_of(m["verts"])
    assert not skipped.any() and (r < 0.5).sum() == 192
    assert not n_vis[r < 0.5].any()                    # the inner sphere
    assert not n_vis[(r > 0.5) & (r < 0.7)].any()      # the shell's inner wall
    assert n_vis[r > 0.7].all()                        # every vertex of the outer wall is seen by some view


def test_cull_reference_removes_the_inside():
    m = MC.scene("nested")
    (v, f, n), st = MC.nested_cull_reference("A", 1)
    print(st)
    r = MC.radius_of(v)
    assert st["kept_by_masks"] == len(m["verts"]) and st["n_verts_out"] == len(v) == 1392 and r.min() > 0.7
    assert mc_ref.euler(v, f) == 2 and len(n) == len(v)


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


def test_exports_refuse_bad_arguments_on_the_host():
    """-1 (HM_ERR_INVALID) from the host-side checks, before any pointer is used or any launch is made: with NULL and
    with host pointers alike"""
    L = _lib.lib()
    host = np.zeros(4096, np.float64)
    hp = host.ctypes.data_as(C.c_void_p)
    for p in (None, hp):
        assert L.hm_mesh_mask_votes(p, 1 << 31, p, 1, p, 48, 64, 1, 0, p, p, None) == -1
        assert L.hm_mesh_mask_votes(p, 8, p, 1, p, 0, 64, 1, 0, p, p, None) == -1
        assert L.hm_mesh_mask_votes(p, 8, p, 1, p, 48, 65537, 1, 0, p, p, None) == -1
        assert L.hm_mesh_mask_votes(p, 8, p, 1, p, 48, 64, -1, 0, p, p, None) == -1
        assert L.hm_mesh_depth_maps(p, 8, p, -1, p, 1, 48, 64, 64, p, p, p, 1 << 20, p, None) == -1
        assert L.hm_mesh_depth_maps(p, 8, p, 2, p, 1, 65536, 65536, 64, p, p, p, 1 << 20, p, None) == -1
        assert L.hm_mesh_depth_maps(p, 8, p, 2, p, 1, 48, 64, 0, p, p, p, 1 << 20, p, None) == -1
        assert L.hm_mesh_depth_maps(p, 8, p, 2, p, 1, 48, 64, 64, p, p, p, 16, p, None) == -1      # workspace too small
        assert L.hm_mesh_visible_votes(p, 8, p, 1, p, 48, 64, 65, 0.0, 0, p, None) == -1
        assert L.hm_mesh_visible_votes(p, 8, p, 1, p, 48, 64, 1, float("nan"), 0, p, None) == -1
        assert L.hm_mesh_visible_votes(p, -1, p, 1, p, 48, 64, 1, 0.0, 0, p, None) == -1
        assert L.hm_mesh_keep_mark(p, 1 << 31, 8, p, p, p, p, None) == -1
        assert L.hm_mesh_keep_mark(p, 2, -1, p, p, p, p, None) == -1
    assert L.hm_mesh_mask_votes(None, 8, None, 1, None, 48, 64, 1, 0, None, None, None) == -1
    assert L.hm_mesh_depth_maps(None, 8, None, 2, None, 1, 48, 64, 64, None, None, None, 1 << 20, None, None) == -1
    assert L.hm_mesh_visible_votes(None, 8, None, 1, None, 48, 64, 1, 0.0, 0, None, None) == -1
    assert L.hm_mesh_keep_mark(None, 2, 8, None, None, None, None, None) == -1
    assert b"NULL" in L.hm_last_error()
    assert L.hm_mesh_depth_workspace_bytes(-1, 0) == -1 and L.hm_mesh_depth_workspace_bytes(0, 1 << 31) == -1
    assert L.hm_mesh_depth_workspace_bytes(0, 0) > 0
    assert L.hm_mesh_depth_workspace_bytes(1000, 2000) >= 16 * 1000 + 4 * 2000 + 4
    # nothing to do is not an error
    assert L.hm_mesh_mask_votes(None, 0, None, 1, None, 48, 64, 1, 0, None, None, None) == 0
    assert L.hm_mesh_keep_mark(None, 0, 8, None, None, None, None, None) == 0


def test_ops_check_their_arguments():
    m, vw = MC.scene("sphere"), MC.VIEWS_A
    verts, faces, normals = (torch.from_numpy(m[k].copy()) for k in ("verts", "faces", "normals"))
    proj = vw["proj"]
    masks = torch.ones((4, 48, 64), dtype=torch.bool)
    depth = torch.zeros((4, 48, 64))
    keep = torch.ones(len(verts), dtype=torch.bool)
    calls = {
        "mesh_mask_votes": lambda **k: ops.mesh_mask_votes(k.get("verts", verts), k.get("proj", proj),
                                                           k.get("masks", masks), k.get("dilate", 1)),
        "mesh_depth_maps": lambda **k: ops.mesh_depth_maps(k.get("verts", verts), k.get("faces", faces),
                                                           k.get("proj", proj), k.get("H", 48), k.get("W", 64)),
        "mesh_visible_votes": lambda **k: ops.mesh_visible_votes(k.get("verts", verts), k.get("proj", proj),
                                                                 k.get("depth", depth), k.get("pad", 1),
                                                                 k.get("tol", 0.0)),
        "mesh_keep_vertices": lambda **k: ops.mesh_keep_vertices(k.get("verts", verts), k.get("faces", faces),
                                                                 k.get("normals", normals), k.get("keep", keep)),
    }
    for name, call in calls.items():
        with pytest.raises(_lib.HashmodError, match="no CPU fallback"):
            call()
        for bad in (verts.double(), torch.zeros(8, 4), torch.zeros(3, 8).t(), None):
            with pytest.raises(ValueError, match="verts"):
                call(verts=bad)
    for name in ("mesh_mask_votes", "mesh_depth_maps", "mesh_visible_votes"):
        for bad in (proj.astype(np.float32), proj[:, :, :3], proj[0], torch.zeros(4, 3, 4), None):
            with pytest.raises(ValueError, match="proj"):
                calls[name](proj=bad)
    for name in ("mesh_depth_maps", "mesh_keep_vertices"):
        for bad in (faces.long(), torch.zeros((4, 4), dtype=torch.int32)):
            with pytest.raises(ValueError, match="faces"):
                calls[name](faces=bad)
    for bad in (masks.float(), masks[:3], masks[0], None):
        with pytest.raises(ValueError, match="masks"):
            calls["mesh_mask_votes"](masks=bad)
    for bad in (-1, 1.0, None, True):
        with pytest.raises(ValueError, match="dilate"):
            calls["mesh_mask_votes"](dilate=bad)
    for H, W in ((0, 64), (48, 65537), (65536, 65536), (48.0, 64)):
        with pytest.raises(ValueError, match="H and W"):
            calls["mesh_depth_maps"](H=H, W=W)
    for bad in (depth.double(), depth[:3], depth[0], depth[:, :, ::2], None):
        with pytest.raises(ValueError, match="depth"):
            calls["mesh_visible_votes"](depth=bad)
    for bad in (-1, 65, 1.0):
        with pytest.raises(ValueError, match="pad"):
            calls["mesh_visible_votes"](pad=bad)
    with pytest.raises(ValueError, match="tol"):
        calls["mesh_visible_votes"](tol=float("nan"))
    for bad in (keep.to(torch.uint8), keep[:-1], None):
        with pytest.raises(ValueError, match="keep"):
            calls["mesh_keep_vertices"](keep=bad)
    with pytest.raises(ValueError, match="normals"):
        calls["mesh_keep_vertices"](normals=normals[:-1])
    with pytest.raises(ValueError, match="devices"):
        calls["mesh_keep_vertices"](keep=keep.to("meta"))
    # the front end
    K, pose = torch.from_numpy(vw["intrinsics"].copy()), torch.from_numpy(vw["pose"].copy())
    with pytest.raises(TypeError, match="dilate"):
        cull_mesh((verts, faces), K, pose, masks, (48, 64))
    with pytest.raises(ValueError, match="mask_rule"):
        cull_mesh((verts, faces), K, pose, masks, (48, 64), dilate=1, mask_rule="any")
    with pytest.raises(ValueError, match="min_views"):
        cull_mesh((verts, faces), K, pose, masks, (48, 64), dilate=1, mask_rule="min")
    with pytest.raises(ValueError, match="masks"):
        cull_mesh((verts, faces), K, pose, masks[:, :40], (48, 64), dilate=1)
    with pytest.raises(ValueError, match="mesh"):
        cull_mesh("mesh.ply", K, pose, masks, (48, 64), dilate=1)
    with pytest.raises(_lib.HashmodError, match="no CPU fallback"):
        cull_mesh((verts, faces, normals), K, pose, masks, (48, 64), dilate=1)
