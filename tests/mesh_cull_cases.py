"""Shared inputs of the mesh-culling tests (numpy only) and the numpy restatement that serves as the reference of
csrc/hm_mesh_cull.hip and evaluation/cull.py, in float64 and int64 with one rounding per operation:

  project_ref, pixel_ref, fixed_ref      a vertex seen by a view (csrc/hm_view_dev.h)
  dilate_ref, mask_votes_ref             the square dilation and the per-vertex mask votes
  depth_map_ref                          the raster, a loop over the faces
  visible_votes_ref, keep_vertices_ref   the visibility votes and the compaction
  cull_ref                               cull_mesh's composition of them

Scenes: a sphere of radius 0.6 and a "nested" scene, a sphere of radius 0.3 inside the shell | |x| - 0.7 | < 0.05, both
through tests/mc_ref.marching_cubes on a 24^3 lattice of [-1, 1]^3.  Views: look_at cameras, VIEWS_A four at 64 x 48,
VIEWS_B five at 67 x 45.  Everything slow is computed once and read-only."""
import functools

import numpy as np

import mc_ref

LATTICE = 24
SPACING = 2.0 / (LATTICE - 1)
SPHERE_R = 0.6
INNER_R, SHELL_R, SHELL_HALF = 0.3, 0.7, 0.05
FIXED_LIMIT = float(1 << 24)


# ---------------------------------------------------------------------------------------------------------------------
# cameras
# ---------------------------------------------------------------------------------------------------------------------
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """camera-to-world pose [4,4] fp32: x right, y down, z forward (the dataset's, OpenCV's, convention)"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, eye
    return pose.astype(np.float32)


def intrinsics(focal, H, W):
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = focal
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    return K


def projections(K, pose):
    """P [n,3,4] float64 = K[:3,:3] @ inv(pose)[:3,:4], the product in float64"""
    K, pose = np.asarray(K, np.float64), np.asarray(pose, np.float64)
    return np.ascontiguousarray(K[:, :3, :3] @ np.linalg.inv(pose)[:, :3, :4])


def _views(eyes, focal, H, W):
    pose = np.stack([look_at(e) for e in eyes])
    K = np.stack([intrinsics(focal, H, W)] * len(eyes))
    for a in (pose, K):
        a.setflags(write=False)
    return {"H": H, "W": W, "pose": pose, "intrinsics": K, "proj": projections(K, pose), "eyes": np.asarray(eyes)}


# the whole shell (radius 0.75) is inside every image: its silhouette has tan = 0.75 / sqrt(9 - 0.75^2) = 0.258
VIEWS_A = _views([(3.0, 0.0, 0.0), (-1.5, 2.4, 1.0), (0.3, -2.0, 2.2), (-1.0, -1.0, -2.6)], 80.0, 48, 64)
VIEWS_B = _views([(0.0, 3.0, 0.5), (2.0, 2.0, 1.0), (-2.5, 0.5, -1.5), (0.5, -2.9, 0.2), (1.0, 1.0, 2.7)], 77.0, 45, 67)


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def _lattice_radius():
    a = np.linspace(-1.0, 1.0, LATTICE)
    x, y, z = np.meshgrid(a, a, a, indexing="ij")
    return np.sqrt(x * x + y * y + z * z)


@functools.lru_cache(maxsize=None)
def scene(name):
    """dict(verts fp32 [V,3] in [-1,1]^3, faces int32 [F,3], normals fp32 [V,3]) of "sphere" or "nested".  The field is
    positive INSIDE the material: the shell is 1.15 lattice spacings thick, and on a cell face with two diagonal
    material corners the table joins the corners below the level - with the usual sign that is the free space on both
    sides of the shell, which riddles it with tunnels (Euler characteristic -234, and the inner sphere is seen through
    them); with this sign the three surfaces are closed (Euler characteristic 6: test_mesh_cull_cpu).  The raster draws
    both windings, so the orientation does not matter to it."""
    r = _lattice_radius()
    sdf = {"sphere": r - SPHERE_R, "nested": np.minimum(r - INNER_R, np.abs(r - SHELL_R) - SHELL_HALF)}[name]
    v, f, n = mc_ref.marching_cubes((-sdf).astype(np.float32), 0.0, (SPACING,) * 3)
    out = {"verts": np.ascontiguousarray(v - np.float32(1.0), np.float32), "faces": np.ascontiguousarray(f, np.int32),
           "normals": np.ascontiguousarray(n, np.float32)}
    for a in out.values():
        a.setflags(write=False)
    return out


def radius_of(verts):
    return np.linalg.norm(np.asarray(verts, np.float64), axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# a vertex seen by a view
# ---------------------------------------------------------------------------------------------------------------------
def project_ref(verts, P):
    """(u, v, w, ok) float64 [V] of fp32 verts through one P [3,4]: p_a = ((P[a,0] x + P[a,1] y) + P[a,2] z) + P[a,3]"""
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    x, y, z = (v32[:, a].astype(np.float64) for a in range(3))
    P = np.asarray(P, np.float64)
    with np.errstate(all="ignore"):
        p = [((P[a, 0] * x + P[a, 1] * y) + P[a, 2] * z) + P[a, 3] for a in range(3)]
        w = p[2]
        u, v = p[0] / w, p[1] / w
    ok = np.isfinite(v32).all(1) & np.isfinite(w) & (w > 0)
    return u, v, w, ok


def pixel_ref(u, v, ok, H, W):
    """(col, row, in_image): rint half to even, compared as doubles; col = row = 0 where not in the image"""
    with np.errstate(all="ignore"):
        c, r = np.rint(u), np.rint(v)
        inside = ok & (c >= 0) & (c < W) & (r >= 0) & (r < H)
    return np.where(inside, c, 0).astype(np.int64), np.where(inside, r, 0).astype(np.int64), inside


def fixed_ref(u, v, ok):
    """(X, Y, valid): rint(256 u), rint(256 v), valid iff projectable and both below 2^24 in magnitude"""
    with np.errstate(all="ignore"):
        x, y = np.rint(u * 256.0), np.rint(v * 256.0)
        valid = ok & (np.abs(x) < FIXED_LIMIT) & (np.abs(y) < FIXED_LIMIT)
    return np.where(valid, x, 0).astype(np.int64), np.where(valid, y, 0).astype(np.int64), valid


# ---------------------------------------------------------------------------------------------------------------------
# mask votes
# ---------------------------------------------------------------------------------------------------------------------
def dilate_ref(mask, r):
    """mask [H,W] dilated by the (2r+1)^2 square, zero outside the image: the OR of the shifted copies, rows then columns"""
    m = np.asarray(mask) != 0
    H, W = m.shape
    rows = np.zeros_like(m)
    for d in range(-min(r, H), min(r, H) + 1):
        src = m[max(d, 0):H + min(d, 0)]
        rows[max(-d, 0):H + min(-d, 0)] |= src
    out = np.zeros_like(m)
    for d in range(-min(r, W), min(r, W) + 1):
        src = rows[:, max(d, 0):W + min(d, 0)]
        out[:, max(-d, 0):W + min(-d, 0)] |= src
    return out


def mask_votes_ref(verts, proj, masks, r):
    """(n_in_image, n_in_mask) int32 [V]"""
    n = len(np.asarray(verts).reshape(-1, 3))
    n_img, n_msk = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for P, m in zip(proj, masks):
        H, W = m.shape
        u, v, _, ok = project_ref(verts, P)
        col, row, inside = pixel_ref(u, v, ok, H, W)
        n_img += inside
        n_msk += inside & dilate_ref(m, r)[row, col]
    return n_img, n_msk


# ---------------------------------------------------------------------------------------------------------------------
# depth maps
# ---------------------------------------------------------------------------------------------------------------------
def depth_map_ref(verts, faces, P, H, W):
    """(depth [H,W] fp32, n_skipped) of one view: the loop over the faces"""
    u, v, w, ok = project_ref(verts, P)
    X, Y, valid = fixed_ref(u, v, ok)
    with np.errstate(all="ignore"):
        iw = 1.0 / w
    depth = np.full((H, W), np.inf, np.float32)
    skipped = 0
    for f in np.asarray(faces, np.int64).reshape(-1, 3):
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
        E = []
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            E.append((xs[c] - xs[b]) * (Yp - ys[b]) - (ys[c] - ys[b]) * (Xp - xs[b]))
        covered = ((E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)) | ((E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0))
        if not covered.any():
            continue
        bary = [e.astype(np.float64) / np.float64(area) for e in E]
        with np.errstate(all="ignore"):
            z = (1.0 / ((bary[0] * iw[f[0]] + bary[1] * iw[f[1]]) + bary[2] * iw[f[2]])).astype(np.float32)
        good = covered & np.isfinite(z) & (z > 0)
        box = depth[r0:r1 + 1, c0:c1 + 1]
        box[good] = np.minimum(box[good], z[good])
    return depth, skipped


def depth_maps_ref(verts, faces, proj, H, W):
    """(depth [n,H,W] fp32, n_skipped [n] int32)"""
    out = [depth_map_ref(verts, faces, P, H, W) for P in proj]
    depth = np.stack([d for d, _ in out]) if out else np.zeros((0, H, W), np.float32)
    return depth, np.asarray([s for _, s in out], np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# visibility votes, compaction, the whole
# ---------------------------------------------------------------------------------------------------------------------
def visible_ref(verts, P, depth, pad, tol):
    """bool [V]: in the image of this view and float32(w) <= max of depth over the clamped (2 pad + 1)^2 pixels + tol"""
    H, W = depth.shape
    u, v, w, ok = project_ref(verts, P)
    col, row, inside = pixel_ref(u, v, ok, H, W)
    m = np.full(len(w), -np.inf, np.float32)
    for dr in range(-pad, pad + 1):
        for dc in range(-pad, pad + 1):
            m = np.maximum(m, depth[np.clip(row + dr, 0, H - 1), np.clip(col + dc, 0, W - 1)])
    with np.errstate(all="ignore"):
        return inside & (w.astype(np.float32) <= m + np.float32(tol))


def visible_votes_ref(verts, proj, depth, pad=1, tol=0.0):
    n = np.zeros(len(np.asarray(verts).reshape(-1, 3)), np.int32)
    for P, d in zip(proj, depth):
        n += visible_ref(verts, P, d, pad, tol)
    return n


def keep_vertices_ref(verts, faces, normals, keep):
    """(verts, faces int32, normals or None): the faces whose three vertices are kept, the vertices they use"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    alive = np.asarray(keep, bool)[faces].all(1) if len(faces) else np.zeros(0, bool)
    used = np.zeros(len(verts), bool)
    used[faces[alive]] = True
    new_id = np.cumsum(used) - 1
    return (np.asarray(verts)[used], new_id[faces[alive]].astype(np.int32).reshape(-1, 3),
            None if normals is None else np.asarray(normals)[used])


def cull_ref(verts, faces, normals, views, masks, dilate, mask_rule="all", min_views=None, visibility=True, pad=1,
             tol=0.0):
    """((verts, faces, normals), stats dict) as evaluation.cull.cull_mesh composes the steps (without the component)"""
    H, W, proj = views["H"], views["W"], views["proj"]
    stats = {"n_verts": len(verts), "n_faces": len(faces), "kept_by_masks": None, "kept_by_visibility": None,
             "n_skipped": None}
    if masks is not None:
        n_img, n_msk = mask_votes_ref(verts, proj, masks, dilate)
        keep = n_msk == n_img if mask_rule == "all" else n_msk >= min_views
        stats["kept_by_masks"] = int(keep.sum())
        verts, faces, normals = keep_vertices_ref(verts, faces, normals, keep)
    if visibility:
        depth, skipped = depth_maps_ref(verts, faces, proj, H, W)
        keep = visible_votes_ref(verts, proj, depth, pad, tol) >= 1
        stats["kept_by_visibility"] = int(keep.sum())
        stats["n_skipped"] = tuple(int(s) for s in skipped)
        verts, faces, normals = keep_vertices_ref(verts, faces, normals, keep)
    stats["n_verts_out"], stats["n_faces_out"] = len(verts), len(faces)
    return (verts, faces, normals), stats


# ---------------------------------------------------------------------------------------------------------------------
# cached references of the scenes
# ---------------------------------------------------------------------------------------------------------------------
def views(which):
    return {"A": VIEWS_A, "B": VIEWS_B}[which]


@functools.lru_cache(maxsize=None)
def scene_depth(name, which):
    """(depth [n,H,W], n_skipped [n]) of a scene in a view set, read-only"""
    m, vw = scene(name), views(which)
    depth, skipped = depth_maps_ref(m["verts"], m["faces"], vw["proj"], vw["H"], vw["W"])
    depth.setflags(write=False)
    skipped.setflags(write=False)
    return depth, skipped


@functools.lru_cache(maxsize=None)
def shell_masks(which):
    """[n,H,W] bool: the silhouette of the nested scene (its shell) in every view, from its depth maps"""
    m = np.isfinite(scene_depth("nested", which)[0])
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def nested_cull_reference(which="A", dilate=1):
    m = scene("nested")
    return cull_ref(m["verts"], m["faces"], m["normals"], views(which), shell_masks(which), dilate)


def sphere_depth_analytic(view, k, radius=SPHERE_R):
    """depth [H,W] float64 along the camera's z of the sphere |x| = radius at every pixel centre of view k, inf off it"""
    H, W = view["H"], view["W"]
    K, pose = view["intrinsics"][k].astype(np.float64), view["pose"][k].astype(np.float64)
    col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d_cam = np.stack([(col - K[0, 2]) / K[0, 0], (row - K[1, 2]) / K[1, 1], np.ones_like(col)], -1)   # z = 1
    d = d_cam @ pose[:3, :3].T
    o = pose[:3, 3]
    a, b, c = (d * d).sum(-1), 2.0 * (d @ o), o @ o - radius * radius
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(disc)) / (2 * a)
    return np.where(disc >= 0, t, np.inf)


def special_vertices(view, k=0):
    """fp32 [., 3] vertices at chosen image positions of view k (u, v exact only up to the fp32 coordinates: the tests
    compare with the restatement, and test_mesh_cull_cpu checks which of them land where): half-pixel positions, the
    image border, behind the camera, w == 0, non-finite"""
    K, pose = view["intrinsics"][k].astype(np.float64), view["pose"][k].astype(np.float64)
    H, W = view["H"], view["W"]
    uv = [(2.5, 3.5), (3.5, 2.5), (-0.5, 10.0), (W - 0.5, 10.0), (10.0, -0.5), (10.0, H - 0.5), (0.0, 0.0),
          (W - 1.0, H - 1.0), (-0.51, 5.0), (W - 0.49, 5.0), (5.0, H - 0.49), (W / 2.0, H / 2.0), (-40.0, 7.0),
          (1e6, 3.0)]
    pts = []
    for u, v in uv:
        for depth in (2.0, 3.5):
            cam = np.array([(u - K[0, 2]) / K[0, 0] * depth, (v - K[1, 2]) / K[1, 1] * depth, depth])
            pts.append(pose[:3, :3] @ cam + pose[:3, 3])
    eye, fwd = pose[:3, 3], pose[:3, 2]
    pts += [eye - 2.0 * fwd, eye - 0.5 * fwd + 0.1 * pose[:3, 0], eye, eye + 0.25 * pose[:3, 0]]   # behind; w == 0
    pts = np.asarray(pts, np.float32)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]], np.float32)
    return np.concatenate([pts, bad])


def axis_view(H=48, W=64, focal=32.0):
    """one camera at the origin looking along +z with an identity rotation: a vertex (x, y, z) lands on
    u = focal x / z + cx, v = focal y / z + cy, exactly for power-of-two values - half-pixel and border cases are exact"""
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = focal
    K[0, 2], K[1, 2] = 8.0, 4.0
    pose = np.eye(4, dtype=np.float32)
    return {"H": H, "W": W, "pose": pose[None], "intrinsics": K[None], "proj": projections(K[None], pose[None]),
            "eyes": np.zeros((1, 3))}


def at_uv(view, u, v, z=1.0):
    """the fp32 vertex of axis_view that projects to (u, v) at depth z (exact for dyadic u, v and power-of-two z)"""
    K = view["intrinsics"][0].astype(np.float64)
    return [(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z]
