"""Baking a per-face texture atlas of an extracted mesh from the photographs it was trained on, on the device.  A
simplified mesh keeps one colour per vertex and loses the detail between them; the atlas keeps `res` texel steps along
every face edge instead, so the small mesh a user exports carries the photographs' detail.  The reference's eval.py has
no such step: it is an addition, off unless it is called.

texture_mesh: ops.mesh_texture_points gives every texel its point and normal on its face; then a texel is coloured
exactly as color_mesh colours a vertex - the same loop over chunks of views (color._blend_views), the same kernel
(ops.mesh_vertex_colors), the depth maps of the mesh itself; ops.mesh_colors_finish makes the texels.  DESIGN.md
"Texturing the mesh" states the contract."""
from collections import namedtuple

import torch

from .. import ops
from .color import _blend_views

TextureStats = namedtuple("TextureStats", ["n_texels", "n_colored", "n_skipped"])


def texture_mesh(mesh, intrinsics, pose, images, img_res, *, res=8, masks=None, erode=1, pad=1, tol=0.0, min_cos=0.0,
                 power=1, mode="blend", fill=(0.0, 0.0, 0.0), view_bytes=1 << 28, device=None):
    """(ops.TextureAtlas, TextureStats) of `mesh` seen by the input views, on the device.

    mesh, intrinsics, pose, images, img_res, masks, view_bytes and device are color_mesh's, and so are the rules erode,
    pad, tol, min_cos, power and mode (ops.mesh_vertex_colors states them): a texel is coloured as a vertex at the
    texel's point (ops.mesh_texture_points: `res` texel steps per face edge, two faces per block of (res + 2) x
    (res + 3) texels) with the texel's interpolated normal, against the depth maps of the mesh; the result does not
    depend on view_bytes.  A texel no view contributed to holds `fill`, and atlas.used tells which; the atlas'
    2-D image fills its unused tail with `fill` too.

    Memory: about 60 bytes per texel while baking (point, normal and face 28, accumulators 36) and 13 afterwards.  A
    mesh of 0.28 M faces at res 8 has 15.4 M texels: about 0.9 GB.

    TextureStats: n_texels the texels of the mesh's faces (those of the absent half of an odd last block do not
    count); n_colored the texels with at least one view; n_skipped per view (a tuple: the faces mesh_depth_maps could
    not draw).  Only counts come to the host.  render_mesh(texture=atlas) and evaluate_mesh_views(texture=atlas) draw
    the textured mesh; TriMesh(texture=, face_uvs=).export_obj writes it."""
    if not (isinstance(res, int) and not isinstance(res, bool) and 1 <= res <= ops.TEXTURE_MAX_RES):
        raise ValueError(f"hashmod texture_mesh: res must be an integer in [1, {ops.TEXTURE_MAX_RES}]")
    owner = []

    def texel_points(verts, faces, normals):
        points, point_normals, face = ops.mesh_texture_points(verts, faces, res, normals)
        owner.append(face)
        return points, point_normals

    _, faces, _, acc, n_used, skipped = _blend_views("texture_mesh", mesh, texel_points, intrinsics, pose, images,
                                                     img_res, masks, view_bytes, device, erode=erode, pad=pad, tol=tol,
                                                     min_cos=min_cos, power=power, mode=mode)
    n_faces = int(faces.shape[0])
    Hb, Wb = ops.texture_block_shape(res)
    texels = ops.mesh_colors_finish(acc, n_used, mode, fill).reshape(-1, Hb, Wb, 3)
    used = (n_used > 0).reshape(-1, Hb, Wb)
    n_texels, n_colored = torch.stack([(owner[0] >= 0).sum(), used.sum()]).tolist()
    return ops.TextureAtlas(res, n_faces, texels, used, fill), TextureStats(n_texels, n_colored, skipped)


def texture_mesh_for_dataset(mesh, dataset, **kw):
    """texture_mesh with intrinsics_all, pose_all, rgb_images, object_masks and img_res of a SceneDataset (images and
    masks are uploaded chunk by chunk to the mesh's device).  masks=None in `kw` bakes without the masks.  The mesh
    must be in the dataset's normalised frame: before apply_transform(scale_mat)."""
    device = kw.pop("device", None)
    if device is None and isinstance(mesh, (tuple, list)) and isinstance(mesh[0], torch.Tensor):
        device = mesh[0].device
    masks = kw.pop("masks", list(dataset.object_masks))
    return texture_mesh(mesh, torch.stack(list(dataset.intrinsics_all)), torch.stack(list(dataset.pose_all)),
                        list(dataset.rgb_images), dataset.img_res, masks=masks,
                        device="cuda" if device is None else device, **kw)
