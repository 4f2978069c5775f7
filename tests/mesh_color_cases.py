"""The numpy restatement that serves as the reference of csrc/hm_mesh_color.hip, ops.mesh_colors_finish and
evaluation/color.py, in float64 with one rounding per operation, the kernel's associations and a plain loop over the
views (numpy only; built on tests/mesh_cull_cases.py):

  erode_ref                     the square erosion with a set border (cv2.erode's default)
  bilinear_ref                  the four clamped taps and the three interpolations of one view
  vertex_colors_ref             (acc, n_used) of the views, optionally continued from earlier ones
  colors_finish_ref             the colours of (acc, n_used)
  color_mesh_ref                color_mesh's composition with depth_maps_ref

and the synthetic photographs of the analytic sphere (sphere_images)."""
import functools

import numpy as np

import mesh_cull_cases as MC

MODES = ("blend", "best")


def erode_ref(mask, r):
    """mask [H,W] eroded by the (2r+1)^2 square, set outside the image: the AND of the shifted copies = the complement
    of the complement's dilation with a zero border"""
    m = np.asarray(mask) != 0
    return ~MC.dilate_ref(~m, r)


def bilinear_ref(image, u, v):
    """[V,3] float64 of image [H,W,3] at (u, v) float64 [V] with rint(u) in [0, W), rint(v) in [0, H): c0 = floor(u),
    fu = u - c0, taps c0, c0 + 1 clamped (rows likewise); top = (a (1 - fu)) + (b fu), val = (top (1 - fv)) + (bot fv)"""
    H, W = image.shape[:2]
    img = np.asarray(image).astype(np.float64)
    fc, fr = np.floor(u), np.floor(v)
    fu, fv = (u - fc)[:, None], (v - fr)[:, None]
    ca, cb = np.clip(fc.astype(np.int64), 0, W - 1), np.clip(fc.astype(np.int64) + 1, 0, W - 1)
    ra, rb = np.clip(fr.astype(np.int64), 0, H - 1), np.clip(fr.astype(np.int64) + 1, 0, H - 1)
    top = img[ra, ca] * (1.0 - fu) + img[ra, cb] * fu
    bot = img[rb, ca] * (1.0 - fu) + img[rb, cb] * fu
    return top * (1.0 - fv) + bot * fv


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def contributes_ref(verts, normals, P, center, depth, mask, erode, pad, tol, min_cos, power):
    """(contributes bool [V], weight float64 [V], u, v) of one view: the four tests in the kernel's order"""
    H, W = depth.shape
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    u, v, _, ok = MC.project_ref(v32, P)
    col, row, inside = MC.pixel_ref(u, v, ok, H, W)
    keep = inside & MC.visible_ref(v32, P, np.asarray(depth, np.float32), pad, tol)
    if mask is not None:
        keep &= erode_ref(mask, erode)[row, col]
    w = np.ones(len(v32))
    if normals is not None:
        n = [np.asarray(normals, np.float32).reshape(-1, 3)[:, a].astype(np.float64) for a in range(3)]
        with np.errstate(all="ignore"):
            d = [np.float64(center[a]) - v32[:, a].astype(np.float64) for a in range(3)]
            den = np.sqrt(_dot(n, n) * _dot(d, d))
            cos = _dot(n, d) / den
            keep &= (den > 0) & np.isfinite(cos) & (cos > min_cos)
            for _ in range(power):
                w = w * cos
    return keep, w, u, v


def vertex_colors_ref(verts, normals, proj, centers, images, depth, masks=None, erode=0, pad=1, tol=0.0, min_cos=0.0,
                      power=1, mode="blend", out=None):
    """(acc [V,4] float64, n_used [V] int32) as hm_mesh_vertex_colors computes them; `out`, when given, is continued (a
    copy: the arguments are left alone)"""
    assert mode in MODES
    n_verts = len(np.asarray(verts).reshape(-1, 3))
    acc = np.zeros((n_verts, 4)) if out is None else np.array(out[0], np.float64)
    n_used = np.zeros(n_verts, np.int32) if out is None else np.array(out[1], np.int32)
    for k in range(len(proj)):
        keep, w, u, v = contributes_ref(verts, normals, proj[k], centers[k], depth[k],
                                        None if masks is None else masks[k], erode, pad, tol, min_cos, power)
        idx = np.flatnonzero(keep)
        val = bilinear_ref(images[k], u[idx], v[idx])
        wk = w[idx]
        n_used[idx] += 1
        with np.errstate(all="ignore"):
            if mode == "blend":
                acc[idx, :3] = acc[idx, :3] + wk[:, None] * val
                acc[idx, 3] = acc[idx, 3] + wk
            else:
                better = wk > acc[idx, 3]
                acc[idx[better], :3] = val[better]
                acc[idx[better], 3] = wk[better]
    return acc, n_used


def colors_finish_ref(acc, n_used, mode, fill=(0.0, 0.0, 0.0)):
    """fp32 [V,3]: acc[:, :3] / acc[:, 3:] in float64 (blend) or acc[:, :3] (best), `fill` where no view contributed"""
    assert mode in MODES
    with np.errstate(all="ignore"):
        rgb = acc[:, :3] / acc[:, 3:] if mode == "blend" else acc[:, :3]
        rgb = rgb.astype(np.float32)
    return np.where((np.asarray(n_used) > 0)[:, None], rgb, np.asarray(fill, np.float32)[None, :])


def view_centers(vw):
    """[n,3] float64: the camera centres pose[:, :3, 3] of a view set"""
    return np.ascontiguousarray(vw["pose"][:, :3, 3].astype(np.float64))


def color_mesh_ref(verts, faces, normals, vw, images, masks=None, erode=1, pad=1, tol=0.0, min_cos=0.0, power=1,
                   mode="blend", fill=(0.0, 0.0, 0.0), depth=None):
    """(colors fp32 [V,3], stats dict) as evaluation.color.color_mesh composes the steps; `depth`, when given, is
    depth_maps_ref's (depth, n_skipped) of this mesh and these views (the cached one of a scene)"""
    H, W = vw["H"], vw["W"]
    maps, skipped = MC.depth_maps_ref(verts, faces, vw["proj"], H, W) if depth is None else depth
    acc, n_used = vertex_colors_ref(verts, normals, vw["proj"], view_centers(vw), images, maps, masks, erode, pad, tol,
                                    min_cos, power, mode)
    stats = {"n_verts": len(verts), "n_colored": int((n_used > 0).sum()), "n_skipped": tuple(int(s) for s in skipped)}
    return colors_finish_ref(acc, n_used, mode, fill), stats


# ---------------------------------------------------------------------------------------------------------------------
# photographs
# ---------------------------------------------------------------------------------------------------------------------
def sphere_color(points, radius=MC.SPHERE_R):
    """g(x) = x / (2 R): a colour that is linear in the position on the sphere, in [-0.5, 0.5]^3"""
    return np.asarray(points, np.float64) / (2.0 * radius)


@functools.lru_cache(maxsize=None)
def sphere_images(which, radius=MC.SPHERE_R):
    """(images fp32 [n,H,W,3], masks bool [n,H,W]) of the analytic sphere: a pixel shows g(hit) of its centre ray's
    hit and white (1, 1, 1) off the sphere; the masks are the silhouettes.  Read-only."""
    vw = MC.views(which)
    H, W = vw["H"], vw["W"]
    images, masks = [], []
    for k in range(len(vw["proj"])):
        K, pose = vw["intrinsics"][k].astype(np.float64), vw["pose"][k].astype(np.float64)
        z = MC.sphere_depth_analytic(vw, k, radius)                       # along the camera's z: d_cam has z = 1
        col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        d = np.stack([(col - K[0, 2]) / K[0, 0], (row - K[1, 2]) / K[1, 1], np.ones_like(col)], -1) @ pose[:3, :3].T
        hit = np.isfinite(z)
        x = pose[:3, 3] + np.where(hit, z, 0.0)[..., None] * d
        images.append(np.where(hit[..., None], sphere_color(x, radius), 1.0).astype(np.float32))
        masks.append(hit)
    images, masks = np.stack(images), np.stack(masks)
    images.setflags(write=False)
    masks.setflags(write=False)
    return images, masks


@functools.lru_cache(maxsize=None)
def noise_images(which, seed=5):
    """fp32 [n,H,W,3] in [-1, 1): every pixel differs from its neighbours, so a wrong tap or weight shows.  Read-only."""
    vw = MC.views(which)
    img = np.random.default_rng(seed).uniform(-1, 1, (len(vw["proj"]), vw["H"], vw["W"], 3)).astype(np.float32)
    img.setflags(write=False)
    return img
