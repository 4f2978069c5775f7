"""The numpy restatement that serves as the reference of csrc/hm_mesh_texture.hip, ops.TextureAtlas and
evaluation/texture.py (numpy only; built on tests/mesh_cull_cases.py, mesh_color_cases.py and mesh_render_cases.py), in
float64 with one rounding per operation and the kernels' associations:

  layout_ref            who owns a block's texels and the texels' barycentric numerators (S, T)
  texel_points_ref      (points, normals, face) of every texel of a mesh's atlas
  texture_sample_ref    the colour of (face, weights) samples
  atlas_shape_ref, face_uvs_ref, atlas_image_ref   the 2-D image of the export
  bake_ref              mesh_color_cases.vertex_colors_ref over texel_points_ref: the bake
  texture_views_ref     render_mesh(texture=) / render_mesh(colors=) composed from the restatements

and the scenes of the plane property and of the quality order (pattern_*, coarse_sphere)."""
import functools
import math

import numpy as np

import mesh_color_cases as CC
import mesh_cull_cases as MC
import mesh_render_cases as MR


# ---------------------------------------------------------------------------------------------------------------------
# the atlas
# ---------------------------------------------------------------------------------------------------------------------
def block_shape(n):
    """(Hb, Wb) of a block at res n"""
    return n + 2, n + 3


def layout_ref(n):
    """(upper bool [Hb,Wb], S int64 [Hb,Wb], T int64 [Hb,Wb]): texel (i, j) = (column, row) belongs to the lower face
    iff i + j <= n + 1; an upper texel is point-mirrored, (i, j) -> (n + 2 - i, n + 1 - j), and then follows the lower
    rule: S = 2i, T = 2j inside (i + j <= n), else the nearest point of the hypotenuse, S = clamp(2i - 1, 0, 2n),
    T = 2n - S.  b1 = S / 2n, b2 = T / 2n, b0 = (2n - S - T) / 2n."""
    Hb, Wb = block_shape(n)
    j, i = np.meshgrid(np.arange(Hb, dtype=np.int64), np.arange(Wb, dtype=np.int64), indexing="ij")
    upper = i + j > n + 1
    i, j = np.where(upper, n + 2 - i, i), np.where(upper, n + 1 - j, j)
    inside = i + j <= n
    S = np.where(inside, 2 * i, np.clip(2 * i - 1, 0, 2 * n))
    T = np.where(inside, 2 * j, 2 * n - S)
    return upper, S, T


def _mix(b, corners):
    """float32(((b0 A) + (b1 B)) + (b2 C)) per component: b three float64 [K], corners three fp32 [K,3]"""
    a = [np.asarray(c, np.float32).astype(np.float64) for c in corners]
    with np.errstate(all="ignore"):
        return (((b[0][:, None] * a[0]) + (b[1][:, None] * a[1])) + (b[2][:, None] * a[2])).astype(np.float32)


def texel_points_ref(verts, faces, n, normals=None):
    """(points fp32 [T,3], normals fp32 [T,3] or None, face int32 [T]) in block-major order, t = (b Hb + j) Wb + i; a
    texel of the absent upper half of the last block has face -1 and NaN point and normal"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n_blocks = (len(faces) + 1) // 2
    upper, S, T = layout_ref(n)
    face = (2 * np.arange(n_blocks, dtype=np.int64)[:, None, None] + upper[None]).reshape(-1)
    S, T = np.broadcast_to(S, (n_blocks,) + S.shape).reshape(-1), np.broadcast_to(T, (n_blocks,) + T.shape).reshape(-1)
    d = np.float64(2 * n)
    b = [(2 * n - S - T).astype(np.float64) / d, S.astype(np.float64) / d, T.astype(np.float64) / d]
    there = face < len(faces)
    ids = faces[np.where(there, face, 0)]

    def mix(table):
        out = _mix(b, [np.asarray(table, np.float32).reshape(-1, 3)[ids[:, m]] for m in range(3)])
        out[~there] = np.nan
        return out

    return mix(verts), None if normals is None else mix(normals), np.where(there, face, -1).astype(np.int32)


def texture_sample_ref(texels, n, n_faces, face_id, weights, background=0.0):
    """fp32 [..., 3]: texels [n_blocks,Hb,Wb,3] fp32 at the samples face_id [...] int32, weights [..., 3] fp32.  face
    < 0 or a non-finite weight: the background.  Else s = w1 n, t = w2 n; the upper face mirrors them to (n + 2 - s,
    n + 1 - t); both are clamped to the block as doubles; taps floor and min(floor + 1, edge); along x, then along y,
    with (a (1 - f)) + (b f); one rounding to fp32."""
    Hb, Wb = block_shape(n)
    texels = np.asarray(texels, np.float32).reshape(-1, Hb, Wb, 3)
    face = np.asarray(face_id, np.int64)
    w = np.asarray(weights, np.float32).reshape(face.shape + (3,))
    out = np.empty(face.shape + (3,), np.float32)
    out[...] = np.broadcast_to(np.asarray(background, np.float32), (3,))
    on = (face >= 0) & np.isfinite(w).all(-1)
    assert (face[on] < n_faces).all(), "the kernel reports such a face"
    f, w = face[on], w[on].astype(np.float64)
    s, t = w[:, 1] * np.float64(n), w[:, 2] * np.float64(n)
    up = (f & 1) == 1
    px, py = np.where(up, np.float64(n + 2) - s, s), np.where(up, np.float64(n + 1) - t, t)
    px, py = np.minimum(np.maximum(px, 0.0), np.float64(Wb - 1)), np.minimum(np.maximum(py, 0.0), np.float64(Hb - 1))
    fx0, fy0 = np.floor(px), np.floor(py)
    fx, fy = (px - fx0)[:, None], (py - fy0)[:, None]
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, Wb - 1), np.minimum(y0 + 1, Hb - 1)
    b = f >> 1
    taa, tab, tba, tbb = (texels[b, y, x].astype(np.float64) for y, x in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    with np.errstate(all="ignore"):
        top = taa * (1.0 - fx) + tab * fx
        bot = tba * (1.0 - fx) + tbb * fx
        out[on] = (top * (1.0 - fy) + bot * fy).astype(np.float32)
    return out


def sample_taps_ref(n, upper, weights):
    """the four taps ((x, y), weight) of samples of one face half, as texture_sample_ref forms them: x, y int64 [K,4]
    and the bilinear weights float64 [K,4]"""
    Hb, Wb = block_shape(n)
    w = np.asarray(weights, np.float32).astype(np.float64)
    s, t = w[:, 1] * np.float64(n), w[:, 2] * np.float64(n)
    px, py = (np.float64(n + 2) - s, np.float64(n + 1) - t) if upper else (s, t)
    px, py = np.minimum(np.maximum(px, 0.0), np.float64(Wb - 1)), np.minimum(np.maximum(py, 0.0), np.float64(Hb - 1))
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    fx, fy = px - x0, py - y0
    x1, y1 = np.minimum(x0 + 1, Wb - 1), np.minimum(y0 + 1, Hb - 1)
    return (np.stack([x0, x1, x0, x1], 1), np.stack([y0, y0, y1, y1], 1),
            np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], 1))


# ---------------------------------------------------------------------------------------------------------------------
# the 2-D image of the export
# ---------------------------------------------------------------------------------------------------------------------
def atlas_shape_ref(n, n_blocks, blocks_per_row=None):
    """(bw, Ha, Wa): the default bw is, of the integers within one of sqrt(n_blocks Hb / Wb), the one whose atlas is
    nearest a square (the smallest |Wa - Ha|, of equals the smallest bw)"""
    Hb, Wb = block_shape(n)
    if blocks_per_row is None:
        k = math.isqrt(max(n_blocks, 1) * Hb // Wb)
        cand = [b for b in (k - 1, k, k + 1, k + 2) if b >= 1]
        blocks_per_row = min(cand, key=lambda b: (abs(b * Wb - -(-max(n_blocks, 1) // b) * Hb), b))
    bw = int(blocks_per_row)
    return bw, -(-max(n_blocks, 1) // bw) * Hb, bw * Wb


def face_corner_texels_ref(n, n_faces, blocks_per_row=None):
    """int64 [F,3,2]: the atlas pixel (x, y) of each face corner's texel centre"""
    Hb, Wb = block_shape(n)
    bw, _, _ = atlas_shape_ref(n, (n_faces + 1) // 2, blocks_per_row)
    f = np.arange(n_faces, dtype=np.int64)
    x0, y0 = ((f >> 1) % bw) * Wb, ((f >> 1) // bw) * Hb
    lower = np.array([[0, 0], [n, 0], [0, n]], np.int64)
    upper = np.array([[n + 2, n + 1], [2, n + 1], [n + 2, 1]], np.int64)
    return np.stack([x0, y0], 1)[:, None, :] + np.where(((f & 1) == 1)[:, None, None], upper[None], lower[None])


def face_uvs_ref(n, n_faces, blocks_per_row=None):
    """float64 [F,3,2]: vt = ((x + 0.5) / Wa, 1 - (y + 0.5) / Ha) of the corners' texel centres"""
    _, Ha, Wa = atlas_shape_ref(n, (n_faces + 1) // 2, blocks_per_row)
    xy = face_corner_texels_ref(n, n_faces, blocks_per_row).astype(np.float64)
    return np.stack([(xy[..., 0] + 0.5) / Wa, 1.0 - (xy[..., 1] + 0.5) / Ha], -1)


def atlas_image_ref(texels, n, blocks_per_row=None, fill=(0.0, 0.0, 0.0)):
    """fp32 [Ha,Wa,3]: the blocks laid out bw per row, the unused tail filled"""
    Hb, Wb = block_shape(n)
    texels = np.asarray(texels, np.float32).reshape(-1, Hb, Wb, 3)
    bw, Ha, Wa = atlas_shape_ref(n, len(texels), blocks_per_row)
    img = np.empty((Ha, Wa, 3), np.float32)
    img[...] = np.asarray(fill, np.float32)
    for b, blk in enumerate(texels):
        y0, x0 = (b // bw) * Hb, (b % bw) * Wb
        img[y0:y0 + Hb, x0:x0 + Wb] = blk
    return img


# ---------------------------------------------------------------------------------------------------------------------
# the bake and the textured views
# ---------------------------------------------------------------------------------------------------------------------
def bake_ref(verts, faces, normals, vw, images, n, masks=None, erode=1, pad=1, tol=0.0, min_cos=0.0, power=1,
             mode="blend", fill=(0.0, 0.0, 0.0), depth=None):
    """(texels fp32 [n_blocks,Hb,Wb,3], used bool [n_blocks,Hb,Wb], stats dict, (acc, n_used)) as
    evaluation.texture.texture_mesh composes the steps: the texels' points and normals coloured as vertices against
    the depth maps of the mesh itself"""
    Hb, Wb = block_shape(n)
    pts, nrm, face = texel_points_ref(verts, faces, n, normals)
    maps, skipped = MC.depth_maps_ref(verts, faces, vw["proj"], vw["H"], vw["W"]) if depth is None else depth
    acc, n_used = CC.vertex_colors_ref(pts, nrm, vw["proj"], CC.view_centers(vw), images, maps, masks, erode, pad, tol,
                                       min_cos, power, mode)
    texels = CC.colors_finish_ref(acc, n_used, mode, fill).reshape(-1, Hb, Wb, 3)
    stats = {"n_texels": int((face >= 0).sum()), "n_colored": int((n_used > 0).sum()),
             "n_skipped": tuple(int(s) for s in skipped)}
    return texels, (n_used > 0).reshape(-1, Hb, Wb), stats, (acc, n_used)


def to_unit(c):
    """the fp32 (c + 1) / 2 clamped to [0, 1] of render_mesh's colour shade"""
    return np.clip((np.asarray(c, np.float32) + np.float32(1.0)) / np.float32(2.0), np.float32(0.0), np.float32(1.0))


def texture_views_ref(verts, faces, vw, n, texels, background=1.0, render=None):
    """rgb fp32 [n_views,H,W,3] in [0,1] as render_mesh(texture=) composes it: the visibility buffer's face and
    weights, the sampler over (texels + 1) / 2 clamped, the background where nothing is drawn"""
    r = MR.renders_ref(verts, faces, vw["proj"], vw["H"], vw["W"]) if render is None else render
    rgb = texture_sample_ref(to_unit(texels), n, len(faces), r["face_id"], r["weights"], background)
    return np.clip(rgb, np.float32(0.0), np.float32(1.0))


def color_views_ref(verts, faces, vw, colors, background=1.0):
    """rgb fp32 [n_views,H,W,3] as render_mesh(colors=) composes it"""
    r = MR.renders_ref(verts, faces, vw["proj"], vw["H"], vw["W"], to_unit(colors), background)
    return np.clip(r["image"], np.float32(0.0), np.float32(1.0))


def psnr_ref(a, b, mask):
    """PSNR (data range 1) of two [H,W,3] images in [0,1] over the pixels of mask [H,W]"""
    d = (np.asarray(a, np.float64) - np.asarray(b, np.float64))[mask]
    return float(10.0 * np.log10(1.0 / np.mean(d * d)))


# ---------------------------------------------------------------------------------------------------------------------
# small meshes
# ---------------------------------------------------------------------------------------------------------------------
def fan_mesh(n_faces, seed=0):
    """(verts fp32 [V,3], faces int32 [F,3], normals fp32 [V,3]): n_faces random triangles over n_faces + 2 vertices"""
    rng = np.random.default_rng(100 + n_faces + seed)
    verts = rng.uniform(-1, 1, (n_faces + 2, 3)).astype(np.float32)
    faces = np.stack([rng.permutation(n_faces + 2)[:3] for _ in range(n_faces)]).astype(np.int32)
    normals = rng.normal(size=verts.shape).astype(np.float32)
    return verts, faces, normals


# ---------------------------------------------------------------------------------------------------------------------
# the plane property: one fronto-parallel quad, one view, a photograph affine in the pixel coordinates
# ---------------------------------------------------------------------------------------------------------------------
def plane_scene():
    """(verts, faces, normals, view set, images [1,H,W,3]): a quad at depth 1 of MC.axis_view covering the pixels
    [6, 40] x [5, 37], split along a diagonal; the photograph is a + b col + c row per channel, inside [-1, 1]"""
    vw = MC.axis_view()
    quad = np.asarray([MC.at_uv(vw, 6.0, 5.0), MC.at_uv(vw, 40.0, 5.0), MC.at_uv(vw, 6.0, 37.0),
                       MC.at_uv(vw, 40.0, 37.0)], np.float32)
    faces = np.asarray([[0, 1, 2], [3, 2, 1]], np.int32)
    normals = np.tile(np.asarray([[0.0, 0.0, -1.0]], np.float32), (4, 1))
    col, row = np.meshgrid(np.arange(vw["W"], dtype=np.float64), np.arange(vw["H"], dtype=np.float64))
    chan = [(-0.9, 0.02, 0.01), (0.8, -0.015, -0.012), (0.1, 0.01, -0.02)]
    image = np.stack([a + b * col + c * row for a, b, c in chan], -1).astype(np.float32)
    return quad, faces, normals, vw, image[None]


# ---------------------------------------------------------------------------------------------------------------------
# the quality order: a coarse sphere and photographs with an analytic surface pattern
# ---------------------------------------------------------------------------------------------------------------------
PATTERN_FREQ = 9.0


def pattern_color(points):
    """fp64 [...,3] in [-0.8, 0.8]: a smooth pattern in the position with about three periods across the sphere -
    finer than the coarse sphere's faces, coarser than two pixels"""
    p = np.asarray(points, np.float64)
    return 0.8 * np.stack([np.sin(PATTERN_FREQ * p[..., 0]), np.sin(PATTERN_FREQ * p[..., 1] + 1.0),
                           np.sin(PATTERN_FREQ * p[..., 2] + 2.0)], -1)


@functools.lru_cache(maxsize=None)
def pattern_images(which, radius=MC.SPHERE_R):
    """(images fp32 [n,H,W,3], masks bool [n,H,W]): mesh_color_cases.sphere_images with pattern_color for its colour"""
    vw = MC.views(which)
    H, W = vw["H"], vw["W"]
    images, masks = [], []
    for k in range(len(vw["proj"])):
        K, pose = vw["intrinsics"][k].astype(np.float64), vw["pose"][k].astype(np.float64)
        z = MC.sphere_depth_analytic(vw, k, radius)
        col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        d = np.stack([(col - K[0, 2]) / K[0, 0], (row - K[1, 2]) / K[1, 1], np.ones_like(col)], -1) @ pose[:3, :3].T
        hit = np.isfinite(z)
        x = pose[:3, 3] + np.where(hit, z, 0.0)[..., None] * d
        images.append(np.where(hit[..., None], pattern_color(x), 1.0).astype(np.float32))
        masks.append(hit)
    images, masks = np.stack(images), np.stack(masks)
    images.setflags(write=False)
    masks.setflags(write=False)
    return images, masks


COARSE_CELL = 0.3


@functools.lru_cache(maxsize=None)
def coarse_sphere_ref():
    """(verts fp32, faces int32, normals fp32): mesh_simplify_cases.simplify (the contract of ops.mesh_simplify) of the
    sphere scene with outward normals at a cell of COARSE_CELL - the mesh the CPU figures of the quality order are
    made on; the GPU test simplifies with ops.mesh_simplify itself"""
    import mesh_simplify_cases as MS
    m = MC.scene("sphere")
    r = MS.simplify(m["verts"], m["faces"], -m["normals"], COARSE_CELL)
    return (np.ascontiguousarray(r["verts"], np.float32), np.ascontiguousarray(r["faces"], np.int32),
            np.ascontiguousarray(r["normals"], np.float32))


class Dataset:
    """what texture_mesh_for_dataset and evaluate_mesh_views read of a SceneDataset, from numpy arrays"""

    def __init__(self, vw, images, masks):
        import torch
        self.img_res = [vw["H"], vw["W"]]
        self.intrinsics_all = [torch.from_numpy(k.copy()) for k in vw["intrinsics"]]
        self.pose_all = [torch.from_numpy(p.copy()) for p in vw["pose"]]
        self.rgb_images = [torch.from_numpy(im.reshape(-1, 3).copy()) for im in images]
        self.object_masks = [torch.from_numpy(mk.reshape(-1).copy()) for mk in masks]
