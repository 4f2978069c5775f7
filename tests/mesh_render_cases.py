"""The numpy restatement of csrc/hm_mesh_render.hip (numpy only), in float64 and int64 with one rounding per operation,
on the projection and the raster of tests/mesh_cull_cases.py:

  render_ref       one view: a loop over the faces that keeps the minimum (z bits, face) key per pixel, then the resolve
  renders_ref      all views of a view set
  scene_render     the cached reference of a scene of mesh_cull_cases in a view set, the vertex positions as attributes
  tie_cases        coincident triangles and triangles that share an edge through pixel centres, in both orders
  ray_plane_point  where a pixel's ray meets a triangle's plane, in float64: the independent truth of the interpolation

Everything slow is computed once and read-only."""
import functools

import numpy as np

import mesh_cull_cases as MC

NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _edges(xs, ys, Xp, Yp):
    E = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        E.append((xs[c] - xs[b]) * (Yp - ys[b]) - (ys[c] - ys[b]) * (Xp - xs[b]))
    return E


def _attr_table(attrs, n_verts):
    """fp32 [V, C]: a [V] vector is one channel; [V, 0] stays zero channels"""
    attrs = np.asarray(attrs, np.float32)
    return attrs.reshape(n_verts, attrs.shape[1] if attrs.ndim == 2 else 1)


def render_ref(verts, faces, P, H, W, attrs=None, background=0.0):
    """dict(face_id [H,W] int32, depth [H,W] fp32, weights [H,W,3] fp32, image [H,W,C] fp32 or None, n_skipped) of one
    view.  The raster is mesh_cull_cases.depth_map_ref's, face by face, but a covered sample with z finite and > 0
    lowers the pixel's key (z bits << 32) | face instead of its depth; the resolve recomputes E_m, area and
    b_m = E_m / area of the winning face and forms t_m = b_m iw_m, s = (t0 + t1) + t2, weight m = float32(t_m / s) and
    channel c = float32((((t0 a0c) + (t1 a1c)) + (t2 a2c)) / s)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    u, v, w, ok = MC.project_ref(verts, P)
    X, Y, valid = MC.fixed_ref(u, v, ok)
    with np.errstate(all="ignore"):
        iw = 1.0 / w
    keys = np.full((H, W), NO_KEY, np.uint64)
    skipped = 0
    for i, f in enumerate(faces):
        if not valid[f].all():
            skipped += 1
            continue
        xs, ys = [int(a) for a in X[f]], [int(a) for a in Y[f]]
        area = (xs[1] - xs[0]) * (ys[2] - ys[0]) - (ys[1] - ys[0]) * (xs[2] - xs[0])
        if area == 0:
            continue
        c0, c1 = max(-((-min(xs)) // 256), 0), min(max(xs) // 256, W - 1)
        r0, r1 = max(-((-min(ys)) // 256), 0), min(max(ys) // 256, H - 1)
        if c0 > c1 or r0 > r1:
            continue
        Xp = 256 * np.arange(c0, c1 + 1, dtype=np.int64)[None, :]
        Yp = 256 * np.arange(r0, r1 + 1, dtype=np.int64)[:, None]
        E = _edges(xs, ys, Xp, Yp)
        covered = ((E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)) | ((E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0))
        if not covered.any():
            continue
        bary = [e.astype(np.float64) / np.float64(area) for e in E]
        with np.errstate(all="ignore"):
            z = (1.0 / ((bary[0] * iw[f[0]] + bary[1] * iw[f[1]]) + bary[2] * iw[f[2]])).astype(np.float32)
        good = covered & np.isfinite(z) & (z > 0)
        key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(i)
        box = keys[r0:r1 + 1, c0:c1 + 1]
        box[good] = np.minimum(box[good], key[good])
    # the resolve, all drawn pixels at once
    drawn = keys != NO_KEY
    face_id = np.where(drawn, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(drawn, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf))
    weights = np.zeros((H, W, 3), np.float32)
    image = None
    if attrs is not None:
        attrs = _attr_table(attrs, len(X))
        image = np.empty((H, W, attrs.shape[1]), np.float32)
        image[:] = np.broadcast_to(np.asarray(background, np.float32), (attrs.shape[1],))
    row, col = np.nonzero(drawn)
    if len(row):
        f = faces[face_id[row, col]]                                     # [K, 3]
        xs, ys = [X[f[:, m]] for m in range(3)], [Y[f[:, m]] for m in range(3)]
        area = (xs[1] - xs[0]) * (ys[2] - ys[0]) - (ys[1] - ys[0]) * (xs[2] - xs[0])
        E = _edges(xs, ys, 256 * col.astype(np.int64), 256 * row.astype(np.int64))
        with np.errstate(all="ignore"):
            t = [(E[m].astype(np.float64) / area.astype(np.float64)) * iw[f[:, m]] for m in range(3)]
            s = (t[0] + t[1]) + t[2]
            for m in range(3):
                weights[row, col, m] = (t[m] / s).astype(np.float32)
            if image is not None:
                a = [attrs[f[:, m]].astype(np.float64) for m in range(3)]    # [K, C]
                num = ((t[0][:, None] * a[0]) + (t[1][:, None] * a[1])) + (t[2][:, None] * a[2])
                image[row, col] = (num / s[:, None]).astype(np.float32)
    return {"face_id": face_id, "depth": depth.astype(np.float32), "weights": weights, "image": image,
            "n_skipped": skipped}


def renders_ref(verts, faces, proj, H, W, attrs=None, background=0.0):
    """the views stacked: face_id [n,H,W], depth, weights, image (or None), n_skipped [n] int32"""
    out = [render_ref(verts, faces, P, H, W, attrs, background) for P in proj]
    C = 0 if attrs is None else _attr_table(attrs, len(np.asarray(verts).reshape(-1, 3))).shape[1]
    empty = {"face_id": np.zeros((0, H, W), np.int32), "depth": np.zeros((0, H, W), np.float32),
             "weights": np.zeros((0, H, W, 3), np.float32), "image": np.zeros((0, H, W, C), np.float32)}
    res = {k: (np.stack([o[k] for o in out]) if out else e) for k, e in empty.items()}
    if attrs is None:
        res["image"] = None
    res["n_skipped"] = np.asarray([o["n_skipped"] for o in out], np.int32)
    return res


@functools.lru_cache(maxsize=None)
def scene_render(name, which):
    """renders_ref of a scene of mesh_cull_cases in a view set with the vertex positions as attributes and the
    background (-1, 0.5, 2), read-only"""
    m, vw = MC.scene(name), MC.views(which)
    res = renders_ref(m["verts"], m["faces"], vw["proj"], vw["H"], vw["W"], m["verts"], (-1.0, 0.5, 2.0))
    for a in res.values():
        a.setflags(write=False)
    return res


def tie_cases():
    """name -> (verts, faces, pixels (rows, cols) that must show face 0)"""
    vw = MC.axis_view()
    tri = np.asarray([MC.at_uv(vw, 4.0, 4.0, 1.0), MC.at_uv(vw, 30.0, 6.0, 2.0), MC.at_uv(vw, 8.0, 28.0, 4.0)],
                     np.float32)
    coincident = (np.concatenate([tri, tri]), np.asarray([[0, 1, 2], [3, 4, 5]], np.int32))
    # two triangles on the two sides of the edge u = 10 from v = 4 to v = 20, which passes through 17 pixel centres
    quad = np.asarray([MC.at_uv(vw, 10.0, 4.0, 1.0), MC.at_uv(vw, 10.0, 20.0, 2.0), MC.at_uv(vw, 3.0, 12.0, 4.0),
                       MC.at_uv(vw, 18.0, 10.0, 2.0)], np.float32)
    left, right = [0, 1, 2], [1, 0, 3]
    edge = (np.arange(4, 21), np.full(17, 10))
    return vw, {"coincident": coincident + (None,),
                "coincident_other_winding": (coincident[0], np.asarray([[0, 1, 2], [5, 4, 3]], np.int32), None),
                "shared_edge": (quad, np.asarray([left, right], np.int32), edge),
                "shared_edge_swapped": (quad, np.asarray([right, left], np.int32), edge)}


def ray_plane_point(view, k, col, row, tri):
    """the point (float64 [3], world) where the ray of pixel centre (col, row) of view k meets the plane of the triangle
    tri [3,3], and its depth along the camera's z"""
    K, pose = view["intrinsics"][k].astype(np.float64), view["pose"][k].astype(np.float64)
    d = pose[:3, :3] @ np.array([(col - K[0, 2]) / K[0, 0], (row - K[1, 2]) / K[1, 1], 1.0])      # z = 1 along the axis
    o = pose[:3, 3]
    tri = np.asarray(tri, np.float64)
    n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    depth = (n @ (tri[0] - o)) / (n @ d)
    return o + depth * d, depth
