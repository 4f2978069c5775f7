"""The numpy restatement of the mesh renderer (tests/mesh_render_cases.py) against independent truths, so that the GPU
tests, which compare csrc/hm_mesh_render.hip with it bit for bit, cannot pass vacuously; the new entry points' ABI and
argument checks (runs anywhere)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import mesh_cull_cases as MC
import mesh_render_cases as MR
from hashmodnffbanks_idr_amd import _lib, ops

NEW_SYMBOLS = {
    "hm_mesh_render_workspace_bytes": (C.c_int64, 4),
    "hm_mesh_render": (C.c_int, 21),
}
EPS64, U32 = 2.0 ** -53, 2.0 ** -24          # the unit roundoffs of fp64 and fp32


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# depth: the depth maps' bits, and the sphere
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("name", ["sphere", "nested"])
def test_depth_is_the_depth_maps(name, which):
    want, want_skipped = MC.scene_depth(name, which)
    got = MR.scene_render(name, which)
    assert np.array_equal(_bits(got["depth"]), _bits(want)) and np.array_equal(got["n_skipped"], want_skipped)
    assert np.array_equal(got["face_id"] >= 0, np.isfinite(want)) and (got["face_id"] >= 0).any()
    assert got["face_id"].max() < len(MC.scene(name)["faces"]) and got["face_id"].min() == -1
    bg = np.asarray((-1.0, 0.5, 2.0), np.float32)
    assert np.array_equal(got["image"][got["face_id"] < 0], np.broadcast_to(bg, (int((got["face_id"] < 0).sum()), 3)))
    assert not got["weights"][got["face_id"] < 0].any()


@pytest.mark.parametrize("which", ["A", "B"])
def test_sphere_depth_is_the_ray_sphere_depth(which):
    """The bound of test_mesh_cull_cpu.test_sphere_depth_is_the_ray_sphere_depth, derived there: the mesh lies between
    the spheres of radius R - delta and R, delta = h^2/(8 (R - h)) + (R - sqrt(R^2 - 3 h^2/4)), so a ray with impact
    parameter b <= R - delta meets it within sqrt(R^2 - b^2) - sqrt((R - delta)^2 - b^2) of the sphere, any other on its
    chord 2 sqrt(R^2 - b^2) of the sphere; depth along the camera's z is shorter than along the ray."""
    vw = MC.views(which)
    depth = MR.scene_render("sphere", which)["depth"]
    R, h = MC.SPHERE_R, MC.SPACING
    delta = h * h / (8 * (R - h)) + (R - np.sqrt(R * R - 0.75 * h * h)) + 1e-6
    for k in range(len(vw["proj"])):
        want = MC.sphere_depth_analytic(vw, k)
        both = np.isfinite(want) & np.isfinite(depth[k])
        assert not (np.isfinite(depth[k]) & ~np.isfinite(want)).any()
        K, pose = vw["intrinsics"][k].astype(np.float64), vw["pose"][k].astype(np.float64)
        col, row = np.meshgrid(np.arange(vw["W"], dtype=np.float64), np.arange(vw["H"], dtype=np.float64))
        d = np.stack([(col - K[0, 2]) / K[0, 0], (row - K[1, 2]) / K[1, 1], np.ones_like(col)], -1) @ pose[:3, :3].T
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        b = np.linalg.norm(np.cross(d, -pose[:3, 3]), axis=-1)
        with np.errstate(invalid="ignore"):
            bound = np.where(b <= R - delta, np.sqrt(R * R - b * b) - np.sqrt((R - delta) ** 2 - b * b),
                             2 * np.sqrt(np.maximum(R * R - b * b, 0)))
        err = np.abs(depth[k].astype(np.float64)[both] - want[both])
        print(which, k, "largest error", err.max() / h, "spacings over", int(both.sum()), "pixels")
        assert both.sum() > 300 and np.all(err <= bound[both] + 1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# interpolation
# ---------------------------------------------------------------------------------------------------------------------
G, C0 = np.array([1.0, -0.5, 0.25]), 0.125       # the attribute A(p) = C0 + G . p: dyadic, exact on dyadic vertices


def _exact_triangles():
    """[(verts fp32 [3,3], faces int32 [1,3])] in MC.axis_view(): corners at multiples of 1/256 pixel, depths 1, 2, 4"""
    vw = MC.axis_view()
    out = []
    for uv, z, order in (([(4.0, 4.0), (40.5, 6.25), (10.0 + 3 / 256, 30.0 + 129 / 256)], (1.0, 2.0, 4.0), (0, 1, 2)),
                         ([(4.0, 4.0), (40.5, 6.25), (10.0 + 3 / 256, 30.0 + 129 / 256)], (4.0, 1.0, 2.0), (2, 1, 0)),
                         ([(60.0 + 255 / 256, 2.0), (20.0, 44.0 + 1 / 256), (55.5, 40.0)], (2.0, 2.0, 0.5), (0, 1, 2))):
        v = np.asarray([MC.at_uv(vw, a, b, d) for (a, b), d in zip(uv, z)], np.float64)
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)               # exact in fp32
        u, vv, w, ok = MC.project_ref(v.astype(np.float32), vw["proj"][0])
        assert ok.all() and u.tolist() == [a for a, _ in uv] and vv.tolist() == [b for _, b in uv]
        X, Y, valid = MC.fixed_ref(u, vv, ok)
        assert valid.all() and np.array_equal(X / 256.0, u) and np.array_equal(Y / 256.0, vv)   # the snap is exact
        out.append((v.astype(np.float32), np.asarray([order], np.int32)))
    return vw, out


def test_affine_attribute_is_the_function_at_the_ray_plane_point():
    """An attribute that is an affine function A(p) = C0 + G . p of the world position, interpolated perspective-
    correctly over a triangle, is A at the point where the pixel's ray meets the triangle's plane.  The corners project
    exactly onto multiples of 1/256 pixel (checked), so the raster's triangle is the projected one; the vertex
    attributes are dyadic and exact in fp32 (checked).  With eps = 2^-53:

    the restatement: E_m and area are exact integers below 2^53; b_m = E_m / area and t_m = b_m iw_m carry two
    roundings each (iw_m = 1/w_m is exact for the power-of-two depths); the t_m are all >= 0 or all <= 0, so
    s = (t0 + t1) + t2 has a relative error of (1 + eps)^4 - 1; each product t_m a_m has three roundings and the two
    sums add two, so the numerator is off by at most 5 eps sum |t_m a_m| (1 + O(eps)); the division adds one rounding.
    With sum |t_m| |a_m| / |s| <= max |a_m| (a convex combination) the fp64 value y is within
    e_k = (5 + 4 + 1 + 1) eps max |a_m|  of the exact one (one eps of slack for the O(eps^2) terms), and the fp32
    result within 2^-24 |y| of y.

    the truth (fp64): n = e1 x e2 has three roundings per component, bounded with nabs = |e1| x |e2| taken over absolute
    values; n . x adds one product and two sums, six roundings per term: depth = (n . v0) / (n . d) has a relative error
    of at most Kd eps, Kd = 6 (nabs . |v0| / |n . v0| + nabs . |d| / |n . d|) + 1, both ratios computed from the data
    here; d is exact (dyadic pixel offsets, identity pose); p = depth d adds one rounding, G . p three products and two
    sums, + C0 one more:  e_t = eps ((Kd + 1 + 3) sum |G_i p_i| + |C0| + |A|).

    |image - A| <= 2^-24 (|A| + e_k + e_t) + e_k + e_t."""
    vw, tris = _exact_triangles()
    H, W = vw["H"], vw["W"]
    n_checked = 0
    for verts, faces in tris:
        attrs64 = C0 + verts.astype(np.float64) @ G
        attrs = attrs64.astype(np.float32)
        assert np.array_equal(attrs.astype(np.float64), attrs64)
        res = MR.render_ref(verts, faces, vw["proj"][0], H, W, attrs[:, None], background=7.0)
        tri = verts[faces[0]].astype(np.float64)
        e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
        n = np.cross(e1, e2)
        nabs = np.array([abs(e1[1] * e2[2]) + abs(e1[2] * e2[1]), abs(e1[2] * e2[0]) + abs(e1[0] * e2[2]),
                         abs(e1[0] * e2[1]) + abs(e1[1] * e2[0])])
        amax = np.abs(attrs64).max()
        rows, cols = np.nonzero(res["face_id"] == 0)
        assert len(rows) > 200 and (res["image"][res["face_id"] < 0] == 7.0).all()
        worst = 0.0
        for r, c in zip(rows, cols):
            p, depth = MR.ray_plane_point(vw, 0, float(c), float(r), tri)
            d = p / depth
            A = C0 + G @ p
            Kd = 6 * (nabs @ np.abs(tri[0]) / abs(n @ tri[0]) + nabs @ np.abs(d) / abs(n @ d)) + 1
            e_t = EPS64 * ((Kd + 4) * (np.abs(G * p)).sum() + abs(C0) + abs(A))
            e_k = 11 * EPS64 * amax
            bound = U32 * (abs(A) + e_k + e_t) + e_k + e_t
            err = abs(float(res["image"][r, c, 0]) - A)
            worst = max(worst, err / bound)
            assert err <= bound, (r, c, err, bound)
            # the depth output is the same point's depth along the camera's z, rounded to fp32
            assert abs(float(res["depth"][r, c]) - depth) <= U32 * depth + (Kd + 11) * EPS64 * depth
        n_checked += len(rows)
        print("pixels", len(rows), "largest error / bound", worst)
    assert n_checked > 1000


@pytest.mark.parametrize("which", ["A", "B"])
def test_interpolated_w_is_the_depth(which):
    """attrs[:, 0] = float32(w_m): image = sum b_m iw_m w'_m / s with w'_m = w_m (1 + d_m), |d_m| <= 2^-24, is
    (1 / s) (1 + d), d a convex combination of the d_m (the weights are >= 0) up to a few eps: the fp64 values of image
    and depth differ by less than 2^-24 of their size, which is less than one fp32 ulp, so their roundings are equal or
    adjacent floats."""
    m, vw = MC.scene("sphere"), MC.views(which)
    for k, P in enumerate(vw["proj"]):
        w = MC.project_ref(m["verts"], P)[2].astype(np.float32)
        res = MR.render_ref(m["verts"], m["faces"], P, vw["H"], vw["W"], w[:, None])
        on = res["face_id"] >= 0
        assert on.sum() > 300
        step = np.abs(_bits(res["image"][..., 0])[on].astype(np.int64) - _bits(res["depth"])[on].astype(np.int64))
        print(which, k, "pixels", int(on.sum()), "differing by one ulp", int((step == 1).sum()))
        assert step.max() <= 1


@pytest.mark.parametrize("name,which", [("sphere", "A"), ("nested", "B")])
def test_weights_are_a_partition_of_one(name, which):
    """each weight is float32 of a value in [0, 1] whose fp64 sum is 1 within a few eps: the three roundings add at most
    2^-24 sum w_m = half an ulp of 1; the bound asked for is 2 ulp"""
    res = MR.scene_render(name, which)
    on = res["face_id"] >= 0
    w = res["weights"][on].astype(np.float64)
    assert (w >= 0).all() and (w <= 1).all()
    assert np.abs(w.sum(1) - 1.0).max() <= 2 * 2.0 ** -23
    # the weights interpolate the positions: image is their combination of the face's corners, up to the fp32 roundings
    m = MC.scene(name)
    corners = m["verts"][m["faces"][res["face_id"][on]]].astype(np.float64)           # [K, 3 corners, 3]
    assert np.abs((w[:, :, None] * corners).sum(1) - res["image"][on]).max() <= 4 * U32 * np.abs(m["verts"]).max()


# ---------------------------------------------------------------------------------------------------------------------
# the tie rule
# ---------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_smaller_face():
    vw, cases = MR.tie_cases()
    for name, (verts, faces, pixels) in cases.items():
        res = MR.render_ref(verts, faces, vw["proj"][0], vw["H"], vw["W"])
        alone = [MR.render_ref(verts, faces[i:i + 1], vw["proj"][0], vw["H"], vw["W"]) for i in range(2)]
        both = (alone[0]["face_id"] >= 0) & (alone[1]["face_id"] >= 0)
        tie = both & (_bits(alone[0]["depth"]) == _bits(alone[1]["depth"]))
        assert tie.any() and (res["face_id"][tie] == 0).all(), name
        if pixels is None:
            assert np.array_equal(tie, both) and tie.sum() > 200 and set(np.unique(res["face_id"])) == {-1, 0}, name
        else:
            assert tie[pixels].all() and tie.sum() == len(pixels[0]), name        # exactly the centres on the edge
            assert (res["face_id"] == 1).sum() > 30 and (res["face_id"] == 0).sum() > 30, name   # both are seen


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


def _render(L, p, *, n_verts=8, n_faces=2, n_views=1, H=48, W=64, big_face=64, attrs="p", n_attr=3, image="p",
            ws_bytes=1 << 24, stream=None):
    pick = {"p": p, None: None}
    return L.hm_mesh_render(p, n_verts, p, n_faces, p, n_views, H, W, big_face, pick[attrs], n_attr, p, p, p, p,
                            pick[image], p, p, ws_bytes, p, stream)


def test_exports_refuse_bad_arguments_on_the_host():
    """-1 (HM_ERR_INVALID) and the function's name in hm_last_error() from the host-side checks, before any pointer is
    used or any launch is made: with host pointers, which a launch would fault on"""
    L = _lib.lib()
    host = np.zeros(4096, np.float64)
    hp = host.ctypes.data_as(C.c_void_p)
    bad = [dict(n_attr=17), dict(n_attr=-1), dict(big_face=0), dict(image=None), dict(attrs=None),
           dict(attrs=None, image=None, n_attr=3), dict(ws_bytes=16), dict(H=65536, W=65536), dict(H=0), dict(W=65537),
           dict(n_faces=-1), dict(n_verts=1 << 31), dict(n_views=-1)]
    for kw in bad:
        assert _render(L, hp, **kw) == -1, kw
        assert b"hm_mesh_render" in L.hm_last_error(), kw
    assert L.hm_mesh_render(None, 8, None, 2, None, 1, 48, 64, 64, None, 0, None, None, None, None, None, None, None,
                            1 << 24, None, None) == -1
    assert b"hm_mesh_render" in L.hm_last_error() and b"NULL" in L.hm_last_error()
    # every pointer but one
    for missing in range(5):
        ptrs = [hp] * 5
        ptrs[missing] = None
        proj, face_id, depth, n_skipped, status = ptrs
        assert L.hm_mesh_render(hp, 8, hp, 2, proj, 1, 48, 64, 64, None, 0, None, face_id, depth, None, None, n_skipped,
                                hp, 1 << 24, status, None) == -1
        assert b"hm_mesh_render: NULL pointer" in L.hm_last_error()
    need = L.hm_mesh_render_workspace_bytes(1000, 2000, 48, 64)
    assert need >= L.hm_mesh_depth_workspace_bytes(1000, 2000) + 8 * 48 * 64
    assert _render(L, hp, n_verts=1000, n_faces=2000, ws_bytes=need - 1) == -1
    assert b"workspace too small" in L.hm_last_error()
    for args in ((-1, 0, 48, 64), (0, 1 << 31, 48, 64), (8, 2, 0, 64), (8, 2, 65536, 65536)):
        assert L.hm_mesh_render_workspace_bytes(*args) == -1
        assert b"hm_mesh_render_workspace_bytes" in L.hm_last_error()
    assert L.hm_mesh_render_workspace_bytes(0, 0, 1, 1) > 0
    # nothing to do is not an error
    assert _render(L, None, n_faces=0, n_views=0, attrs=None, image=None, n_attr=0) == 0


def test_op_checks_its_arguments():
    m, vw = MC.scene("sphere"), MC.VIEWS_A
    verts, faces = (torch.from_numpy(m[k].copy()) for k in ("verts", "faces"))
    attrs = verts.clone()

    def call(**k):
        return ops.mesh_render(k.get("verts", verts), k.get("faces", faces), k.get("proj", vw["proj"]), k.get("H", 48),
                               k.get("W", 64), attrs=k.get("attrs", attrs), background=k.get("background", 0.0),
                               big_face=k.get("big_face", 64))

    with pytest.raises(_lib.HashmodError, match="no CPU fallback"):
        call()
    for bad in (verts.double(), torch.zeros(8, 4), None):
        with pytest.raises(ValueError, match="verts"):
            call(verts=bad)
    for bad in (vw["proj"].astype(np.float32), vw["proj"][0], None):
        with pytest.raises(ValueError, match="proj"):
            call(proj=bad)
    for bad in (faces.long(), torch.zeros((4, 4), dtype=torch.int32)):
        with pytest.raises(ValueError, match="faces"):
            call(faces=bad)
    for H, W in ((0, 64), (48, 65537), (65536, 65536), (48.0, 64)):
        with pytest.raises(ValueError, match="H and W"):
            call(H=H, W=W)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="big_face"):
            call(big_face=bad)
    for bad in (attrs.double(), attrs[:-1], attrs[:, 0], torch.zeros(len(verts), 17), torch.zeros(3, len(verts)).t(),
                attrs.numpy()):
        with pytest.raises(ValueError, match="attrs"):
            call(attrs=bad)
    for bad in ((0.0, 1.0), (0.0,) * 4, "white", None):
        with pytest.raises(ValueError, match="background"):
            call(background=bad)
    with pytest.raises(ValueError, match="background"):
        call(attrs=None, background=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="devices"):
        call(attrs=attrs.to("meta"))
