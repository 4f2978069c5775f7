"""The numpy restatement of the mesh-colouring kernel (tests/mesh_color_cases.py) against independent truths, so that
the GPU tests, which compare the kernel with it bit for bit, cannot pass vacuously; the new entry point's ABI and argument
checks; TriMesh's colours (runs anywhere)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import mesh_color_cases as CC
import mesh_cull_cases as MC
from hashmodnffbanks_idr_amd import _lib, ops
from hashmodnffbanks_idr_amd.evaluation import ColorStats, color_mesh, color_mesh_for_dataset  # noqa: F401
from hashmodnffbanks_idr_amd.utils.plots import TriMesh, colors_to_uint8

NEW_SYMBOLS = {"hm_mesh_vertex_colors": (C.c_int, 21)}
EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------------------------------------------------------------
# independent truths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1, 3, 100])
def test_erosion_is_scipy_binary_erosion(r):
    from scipy.ndimage import binary_erosion
    rng = np.random.default_rng(r)
    for H, W in ((48, 64), (45, 67), (1, 5)):
        for density in (0.998, 0.95):
            for corner in (True, False):                   # set and cleared corners: the set border matters
                m = rng.random((H, W)) < density
                m[0, 0] = m[H - 1, W - 1] = corner
                want = binary_erosion(m, structure=np.ones((2 * r + 1, 2 * r + 1), bool), border_value=1) if r else m
                assert np.array_equal(CC.erode_ref(m, r), want)
    assert CC.erode_ref(np.ones((5, 7), bool), 100).all() and not CC.erode_ref(1 - np.eye(5, 7), 100).any()


def test_erosion_is_the_window_count_rule():
    """what the kernel computes: the count of the clamped window, from four reads of the summed-area table, equals the
    clamped window's area"""
    rng = np.random.default_rng(2)
    for H, W in ((45, 67), (1, 5)):
        m = rng.random((H, W)) < 0.9
        sat = np.zeros((H + 1, W + 1), np.int64)
        sat[1:, 1:] = m.cumsum(0).cumsum(1)
        for r in (0, 1, 2, 100):
            row, col = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            c0, c1 = np.maximum(col - r, 0), np.minimum(col + r, W - 1) + 1
            r0, r1 = np.maximum(row - r, 0), np.minimum(row + r, H - 1) + 1
            count = (sat[r1, c1] - sat[r0, c1]) - (sat[r1, c0] - sat[r0, c0])
            assert np.array_equal(count == (c1 - c0) * (r1 - r0), CC.erode_ref(m, r))


def test_bilinear_taps_are_scipy_map_coordinates():
    """Bound: with M the largest |tap|, each of the three interpolations (a (1 - f)) + (b f) carries a relative error
    of at most 3 roundings (1 - f, a product, the sum; all weights in [0, 1], so absolute error <= 1.5 eps M each), the
    second level passes the first one's on with weight <= 1, and f = u - floor(u) is off by at most eps/2 where it is
    not exact (u in [-0.5, 0)), which moves the value by at most eps M per level: |restatement - exact| <= 5 eps M.
    scipy's order-1 spline evaluates the same four products with weights it rounds once each and sums them in another
    order: the same bound.  Together 10 eps M; the test allows 16 eps M, 3.6e-15 M."""
    from scipy.ndimage import map_coordinates
    rng = np.random.default_rng(0)
    for H, W in ((48, 64), (45, 67), (1, 5)):
        img = rng.uniform(-1, 1, (H, W, 3)).astype(np.float32)
        u = np.concatenate([rng.uniform(-0.5, W - 0.5, 500), [0.0, W - 1.0, 2.5, 3.5, -0.5, -0.25, W - 0.75]])
        v = np.concatenate([rng.uniform(-0.5, H - 0.5, 500), [0.0, H - 1.0, 3.5, 2.5, -0.25, -0.5, H - 0.75]])
        u, v = np.minimum(u, np.nextafter(W - 0.5, 0)), np.minimum(v, np.nextafter(H - 0.5, 0))
        got = CC.bilinear_ref(img, u, v)
        for k in range(3):
            want = map_coordinates(img[:, :, k].astype(np.float64), [v, u], order=1, mode="nearest")
            err = np.abs(got[:, k] - want).max()
            print(H, W, k, "largest difference", err / EPS, "eps")
            assert err <= 16 * EPS * np.abs(img).max()


@pytest.mark.parametrize("W", [64, 67])
def test_bilinear_taps_return_the_edge_pixel(W):
    """u in [-0.5, 0) and in [W - 1, W - 0.5]: both taps are the edge pixel a, and (a (1 - f)) + (a f) is a up to the
    roundings of the two products and the sum (1 - f is exact there), 1.5 eps |a| - the fp32 colour is a exactly"""
    rng = np.random.default_rng(W)
    img = rng.uniform(-1, 1, (6, W, 3)).astype(np.float32)
    row = np.full(4, 2.0)
    for us, edge in ((np.array([-0.5, -0.25, -0.3, np.nextafter(0.0, -1)]), 0),
                     (np.array([W - 1.0, W - 0.75, W - 0.7, np.nextafter(W - 0.5, 0)]), W - 1)):
        got = CC.bilinear_ref(img, us, row)
        a = img[2, edge].astype(np.float64)
        assert np.all(np.abs(got - a) <= 1.5 * EPS * np.abs(a))
        assert np.array_equal(got.astype(np.float32), img[[2] * 4, edge])
        got = CC.bilinear_ref(np.ascontiguousarray(img.transpose(1, 0, 2)), row, us)      # the rows likewise
        assert np.array_equal(got.astype(np.float32), img[[2] * 4, edge])
    assert np.array_equal(CC.bilinear_ref(img, np.array([W - 1.0, 0.0]), np.array([5.0, 0.0])),
                          img[[5, 0], [W - 1, 0]].astype(np.float64))                   # exactly on a pixel: exactly it


# ---------------------------------------------------------------------------------------------------------------------
# the analytic sphere
# ---------------------------------------------------------------------------------------------------------------------
SPHERE_BOUND = 2 * 0.0015132        # twice the restatement's largest error on the CPU: the docstring below


def _sphere_error(images, masks, proj=None):
    """(coloured bool [V], the largest |colour - g(vertex)| over the coloured vertices and the channels) of the sphere
    under views A with erode = 1 and min_cos = 0.5.  The scene's normals are the field's gradient, and the field is
    positive inside the material: they point inwards, so the outward normals are their negatives."""
    m, vw = MC.scene("sphere"), MC.views("A")
    depth, _ = MC.scene_depth("sphere", "A")
    acc, n_used = CC.vertex_colors_ref(m["verts"], -m["normals"], vw["proj"] if proj is None else proj,
                                       CC.view_centers(vw), images, depth, masks, erode=1, min_cos=0.5)
    colors = CC.colors_finish_ref(acc, n_used, "blend")
    colored = n_used > 0
    return colored, np.abs(colors.astype(np.float64) - CC.sphere_color(m["verts"]))[colored].max()


def test_sphere_takes_the_colours_of_its_photographs():
    """Measured bound.  The photographs show g(hit) = hit / (2 R) of the analytic sphere, so a vertex should get
    g(vertex) up to the mesh-to-sphere gap (test_sphere_depth_is_the_ray_sphere_depth: a vertex is inside the sphere by
    at most h^2 / (8 (R - h)) = 0.0018, and g has the Lipschitz constant 1 / (2 R) = 0.83) and the interpolation of g
    between pixel centres.  The restatement's largest error on the CPU is 0.0015132 (710.6 of 1000 vertices coloured,
    an ideal sphere has 70 %); the bound is twice that.  The negative controls miss it by two orders of magnitude:
    0.70 with two channels swapped, 1.49 with the images transposed, 0.95 with the views permuted."""
    images, masks = CC.sphere_images("A")
    colored, err = _sphere_error(images, masks)
    print("coloured", colored.mean(), "largest error", err)
    assert colored.mean() >= 0.5
    assert err <= SPHERE_BOUND
    H, W = images.shape[1:3]
    # (u, v) swapped: pixel (row, col) shows what pixel (col, row) showed (columns beyond H repeat the last)
    transposed = np.stack([im[np.minimum(np.arange(W), H - 1)[None, :], np.arange(H)[:, None]] for im in images])
    controls = {"channels swapped": (images[..., [1, 0, 2]], masks, None),
                "transposed in (u, v)": (transposed, masks, None),
                "views permuted against their projections": (images, masks, np.roll(MC.views("A")["proj"], 1, 0))}
    for name, (img, msk, proj) in controls.items():
        c, e = _sphere_error(img, msk, proj)
        print(name, "coloured", c.mean(), "largest error", e)
        assert c.any() and e > 10 * SPHERE_BOUND, name


# ---------------------------------------------------------------------------------------------------------------------
# occlusion, chunks, ties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B"])
def test_inner_shells_get_no_colour(which):
    m, vw = MC.scene("nested"), MC.views(which)
    depth, _ = MC.scene_depth("nested", which)
    images = CC.noise_images(which)
    inner = MC.radius_of(m["verts"]) < 0.7
    assert inner.sum() == 192 + 1032
    _, n_used = CC.vertex_colors_ref(m["verts"], None, vw["proj"], CC.view_centers(vw), images, depth)
    assert not n_used[inner].any() and n_used[~inner].all()
    _, n_open = CC.vertex_colors_ref(m["verts"], None, vw["proj"], CC.view_centers(vw), images,
                                     np.full_like(depth, np.inf))
    assert n_open[inner].all()                         # without the depth maps every view that has them colours them


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("mode", CC.MODES)
def test_restatement_does_not_depend_on_the_split(mode):
    m, vw = MC.scene("nested"), MC.views("B")
    depth, _ = MC.scene_depth("nested", "B")
    images, centers, n = CC.noise_images("B"), CC.view_centers(vw), len(vw["proj"])
    args = dict(masks=MC.shell_masks("B"), erode=1, min_cos=0.2, power=3, mode=mode)
    acc, n_used = CC.vertex_colors_ref(m["verts"], -m["normals"], vw["proj"], centers, images, depth, **args)
    assert (n_used > 1).sum() > 300
    for k in range(n + 1):
        part = CC.vertex_colors_ref(m["verts"], -m["normals"], vw["proj"][:k], centers[:k], images[:k], depth[:k],
                                    **{**args, "masks": args["masks"][:k]})
        got = CC.vertex_colors_ref(m["verts"], -m["normals"], vw["proj"][k:], centers[k:], images[k:], depth[k:],
                                   **{**args, "masks": args["masks"][k:]}, out=part)
        assert np.array_equal(_bits(got[0]), _bits(acc)) and np.array_equal(got[1], n_used), k


def test_best_mode_keeps_the_first_of_equal_views():
    m, vw = MC.scene("sphere"), MC.views("A")
    depth, _ = MC.scene_depth("sphere", "A")
    images, centers = CC.noise_images("A"), CC.view_centers(vw)
    two = [0, 0]
    other = np.stack([images[0], images[1]])             # the same view twice, with different photographs
    acc, n_used = CC.vertex_colors_ref(m["verts"], -m["normals"], vw["proj"][two], centers[two], other, depth[two],
                                       mode="best")
    first = CC.vertex_colors_ref(m["verts"], -m["normals"], vw["proj"][:1], centers[:1], images[:1], depth[:1],
                                 mode="best")
    assert np.array_equal(_bits(acc), _bits(first[0])) and np.array_equal(n_used, 2 * first[1]) and first[1].sum() > 300
    blend = CC.vertex_colors_ref(m["verts"], -m["normals"], vw["proj"][two], centers[two], other, depth[two])
    assert not np.array_equal(_bits(blend[0]), _bits(acc))


def test_colors_finish():
    acc = np.array([[1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 0.0, 0.0], [0.3, 0.6, 0.9, 3.0]])
    n_used = np.array([2, 0, 3], np.int32)
    fill = (0.5, -1.0, 0.25)
    for mode in CC.MODES:
        want = CC.colors_finish_ref(acc, n_used, mode, fill)
        got = ops.mesh_colors_finish(torch.from_numpy(acc), torch.from_numpy(n_used), mode, fill)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
        assert want[1].tolist() == list(fill)
    assert CC.colors_finish_ref(acc, n_used, "blend")[0].tolist() == [0.25, 0.5, 0.75]
    assert CC.colors_finish_ref(acc, n_used, "best")[0].tolist() == [1.0, 2.0, 3.0]
    for bad in (dict(mode="mean"), dict(fill=(0.0, 0.0)), dict(fill=None), dict(acc=torch.zeros(3, 4)),
                dict(n_used=torch.zeros(2, dtype=torch.int32)), dict(n_used=torch.zeros(3))):
        k = {"acc": torch.from_numpy(acc), "n_used": torch.from_numpy(n_used), "mode": "blend", "fill": fill, **bad}
        with pytest.raises(ValueError, match="mesh_colors_finish"):
            ops.mesh_colors_finish(k["acc"], k["n_used"], k["mode"], k["fill"])


# ---------------------------------------------------------------------------------------------------------------------
# ABI and argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_symbol():
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


def _call(L, p, **k):
    a = dict(n_verts=8, n_views=1, H=48, W=64, pad=1, tol=0.0, erode=1, min_cos=0.0, power=1, mode=0, accumulate=0)
    a.update(k)
    return L.hm_mesh_vertex_colors(p, p, a["n_verts"], p, p, p, p, p, a["n_views"], a["H"], a["W"], a["pad"],
                                   a["tol"], a["erode"], a["min_cos"], a["power"], a["mode"], a["accumulate"], p, p,
                                   None)


def test_export_refuses_bad_arguments_on_the_host():
    """-1 (HM_ERR_INVALID) from the host-side checks, before any pointer is used or any launch is made: with NULL and
    with host pointers alike"""
    L = _lib.lib()
    host = np.zeros(4096, np.float64)
    nan = float("nan")
    bad = [dict(n_verts=-1), dict(n_verts=1 << 31), dict(n_views=-1), dict(n_views=1 << 31), dict(H=0), dict(W=65537),
           dict(H=65536, W=65536), dict(pad=-1), dict(pad=65), dict(erode=-1), dict(erode=65537), dict(tol=nan),
           dict(min_cos=nan), dict(min_cos=-0.1), dict(min_cos=1.0), dict(power=-1), dict(power=9), dict(mode=-1),
           dict(mode=2)]
    for p in (None, host.ctypes.data_as(C.c_void_p)):
        for k in bad:
            assert _call(L, p, **k) == -1, k
            assert b"hm_mesh_vertex_colors" in L.hm_last_error()
    assert _call(L, None) == -1 and b"NULL" in L.hm_last_error()
    assert _call(L, None, n_views=0) == -1 and b"NULL" in L.hm_last_error()     # verts, acc, n_used are needed
    # nothing to do is not an error - after the checks
    assert _call(L, None, n_verts=0) == 0 and _call(L, None, n_verts=0, n_views=0) == 0
    assert _call(L, None, n_verts=0, power=9) == -1
    hp = host.ctypes.data_as(C.c_void_p)
    assert _call(L, hp, n_views=0, accumulate=1) == 0                            # no views to add: no launch


def test_ops_check_their_arguments():
    m, vw = MC.scene("sphere"), MC.VIEWS_A
    verts, faces, normals = (torch.from_numpy(m[k].copy()) for k in ("verts", "faces", "normals"))
    base = dict(verts=verts, normals=normals, proj=vw["proj"], centers=CC.view_centers(vw),
                images=torch.zeros((4, 48, 64, 3)), depth=torch.zeros((4, 48, 64)))
    opts = dict(masks=torch.ones((4, 48, 64), dtype=torch.bool), erode=1, pad=1, tol=0.0, min_cos=0.0, power=1,
                mode="blend", out=None)

    def call(**k):
        a = {**base, **opts, **k}
        return ops.mesh_vertex_colors(*(a[n] for n in base), **{n: a[n] for n in opts})

    with pytest.raises(_lib.HashmodError, match="no CPU fallback"):
        call()
    with pytest.raises(_lib.HashmodError, match="no CPU fallback"):
        call(normals=None, masks=None)
    acc, n_used = torch.zeros((len(verts), 4), dtype=torch.float64), torch.zeros(len(verts), dtype=torch.int32)
    with pytest.raises(_lib.HashmodError, match="no CPU fallback"):
        call(out=(acc, n_used))
    images, depth, masks = base["images"], base["depth"], opts["masks"]
    bad = {
        "verts": (verts.double(), torch.zeros(8, 4), torch.zeros(3, 8).t(), None),
        "normals": (normals.double(), normals[:-1], torch.zeros(3, len(verts)).t(), normals.numpy()),
        "proj": (vw["proj"].astype(np.float32), vw["proj"][:, :, :3], vw["proj"][0], torch.zeros(4, 3, 4), None),
        "centers": (base["centers"].astype(np.float32), base["centers"][:3], base["centers"][:, :2], None,
                    torch.zeros(4, 3)),
        "images": (images.double(), images[:3], images[0], images[..., :2], images[:, :, ::2], None),
        "depth": (depth.double(), depth[:3], depth[0], depth[:, :, ::2], depth[:, :40], None),
        "masks": (masks.float(), masks[:3], masks[0], masks[:, :40], masks.numpy()),
        "erode": (-1, 1.0, None, True),
        "pad": (-1, 65, 1.0, True),
        "tol": (float("nan"), None, "0"),
        "min_cos": (-0.1, 1.0, float("nan"), None, True),
        "power": (-1, 9, 1.0, None, True),
        "mode": ("mean", 0, None),
        "out": (acc, (acc,), (acc.float(), n_used), (acc[:-1], n_used), (acc, n_used.long()), (acc, n_used[:-1]),
                (acc.t().contiguous().t(), n_used)),
    }
    for name, values in bad.items():
        for value in values:
            with pytest.raises(ValueError, match=name):
                call(**{name: value})
    with pytest.raises(ValueError, match="H and W"):
        call(images=torch.zeros((4, 0, 64, 3)), depth=torch.zeros((4, 0, 64)), masks=None)
    with pytest.raises(ValueError, match="devices"):
        call(depth=depth.to("meta"))
    with pytest.raises(ValueError, match="devices"):
        call(out=(acc.to("meta"), n_used.to("meta")))
    # the front end
    K, pose = torch.from_numpy(vw["intrinsics"].copy()), torch.from_numpy(vw["pose"].copy())
    mesh = (verts, faces, normals)
    with pytest.raises(ValueError, match="view_bytes"):
        color_mesh(mesh, K, pose, images, (48, 64), view_bytes=0)
    with pytest.raises(ValueError, match="mode"):
        color_mesh(mesh, K, pose, images, (48, 64), mode="mean")
    with pytest.raises(ValueError, match="per view"):
        color_mesh(mesh, K, pose, images[:3], (48, 64))
    with pytest.raises(ValueError, match="per view"):
        color_mesh(mesh, K, pose, images, (48, 64), masks=masks[:3])
    with pytest.raises(ValueError, match="mesh"):
        color_mesh("mesh.ply", K, pose, images, (48, 64))
    with pytest.raises(ValueError, match="images"):
        color_mesh(mesh, K, pose, images[:, :40], (48, 64), device="cpu")
    with pytest.raises(ValueError, match="masks"):
        color_mesh(mesh, K, pose, images, (48, 64), masks=masks[:, :40], device="cpu")
    with pytest.raises(_lib.HashmodError, match="no CPU fallback"):
        color_mesh(mesh, K, pose, images.reshape(4, -1, 3), (48, 64), masks=masks.reshape(4, -1), device="cpu")


# ---------------------------------------------------------------------------------------------------------------------
# TriMesh carries colours
# ---------------------------------------------------------------------------------------------------------------------
def _two_triangles():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [6, 5, 5], [5, 6, 5]], np.float32)
    faces = np.array([[3, 4, 5], [0, 1, 2]], np.int32)
    normals = np.tile(np.array([[0, 0, 1]], np.float32), (6, 1))
    colors = np.arange(18, dtype=np.uint8).reshape(6, 3) * 13
    return verts, faces, normals, colors


def test_trimesh_exports_its_colours():
    verts, faces, normals, colors = _two_triangles()
    plain = TriMesh(verts, faces, normals).export()
    mesh = TriMesh(verts, faces, normals, vertex_colors=colors)
    assert mesh.vertex_colors is colors or np.array_equal(mesh.vertex_colors, colors)
    data = mesh.export()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 6"]
    assert lines[3:12] == ["property float %s" % n for n in ("x", "y", "z", "nx", "ny", "nz")] + \
        ["property uchar %s" % n for n in ("red", "green", "blue")]
    assert lines[12:] == ["element face 2", "property list uchar int vertex_indices", ""]
    assert len(body) == 6 * 27 + 2 * 13
    for i in range(6):
        rec = body[27 * i:27 * (i + 1)]
        assert np.array_equal(np.frombuffer(rec[:24], "<f4"), np.concatenate([verts[i], normals[i]]))
        assert list(rec[24:]) == colors[i].tolist()
    assert body[6 * 27:] == plain.split(b"end_header\n", 1)[1][6 * 24:]                # the faces are the same bytes
    # without colours: the bytes of a mesh built without the new argument, and no colour property
    assert TriMesh(verts, faces, normals, vertex_colors=None).export() == plain and b"red" not in plain
    assert len(plain.split(b"end_header\n", 1)[1]) == 6 * 24 + 2 * 13
    for bad in (colors.astype(np.float32), colors[:5], colors[:, :2], colors.astype(np.int32)):
        with pytest.raises(ValueError, match="vertex_colors"):
            TriMesh(verts, faces, normals, vertex_colors=bad)


def test_trimesh_split_and_transform_keep_the_colours():
    verts, faces, normals, colors = _two_triangles()
    mesh = TriMesh(verts, faces, normals, vertex_colors=colors)
    parts = mesh.split()
    assert len(parts) == 2
    assert np.array_equal(parts[0].vertex_colors, colors[:3]) and np.array_equal(parts[1].vertex_colors, colors[3:])
    assert parts[0].vertex_colors.dtype == np.uint8
    assert all(p.vertex_colors is None for p in TriMesh(verts, faces, normals).split())
    M = np.diag([2.0, 2.0, -2.0, 1.0])
    M[:3, 3] = (1.0, 2.0, 3.0)
    assert np.array_equal(mesh.apply_transform(M).vertex_colors, colors)


def test_colors_to_uint8():
    c = np.array([[-1.0, 1.0, 0.0], [-1.5, 1.5, 1e9], [1 / 255, -1 + 2 * 126.5 / 255, -1 + 2 * 127.5 / 255]])
    # 0 -> 127.5 -> 128 and 1/255 -> 128.0 (+ an ulp) -> 128; .5 goes to the even byte: 126.5 -> 126, 127.5 -> 128
    assert colors_to_uint8(c).tolist() == [[0, 255, 128], [0, 255, 255], [128, 126, 128]]
    got = colors_to_uint8(torch.tensor([[-1.0, 0.0, 1.0]]))
    assert got.dtype == np.uint8 and got.shape == (1, 3) and got.tolist() == [[0, 128, 255]]
    half = np.array([[2 * 0.5 / 255 - 1, 2 * 1.5 / 255 - 1, 2 * 2.5 / 255 - 1]])
    print("the .5 cases land on", (np.clip((half + 1) / 2, 0, 1) * 255).tolist())
