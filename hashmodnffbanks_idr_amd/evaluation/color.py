"""Colouring an extracted mesh from the photographs it was trained on, on the device: per vertex, the views that see it
(in the image, in front of the mesh's own depth map, inside the eroded object mask, facing the camera) give a bilinear
sample each, blended by cos^power or taken from the best view.  The exported .ply then shows how the surface lines up
with the input images.  The reference's eval.py has no such step: it is an addition, off unless it is called.

color_mesh: per chunk of views the images are uploaded, the mesh's depth maps are drawn (ops.mesh_depth_maps) and
ops.mesh_vertex_colors continues its accumulators; ops.mesh_colors_finish makes the colours.  DESIGN.md "Mesh
colouring on the device" states the contract."""
from collections import namedtuple

import numpy as np
import torch

from .. import ops
from .cull import _device_mesh, view_projections

ColorStats = namedtuple("ColorStats", ["n_verts", "n_colored", "n_skipped"])


def _view_images(images, v0, v1, H, W, device, what="color_mesh"):
    """[v1 - v0, H, W, 3] contiguous fp32 on the device of the views [v0, v1) of a tensor or a list of per-view tensors
    (each view of a list goes straight into its place on the device: no stacked copy on the host)"""
    bad = ValueError(f"hashmod {what}: images must be fp32 [n, H, W, 3], [n, H*W, 3] or a list of [H*W, 3] with "
                     "img_res = (H, W)")
    if isinstance(images, torch.Tensor):
        part = images[v0:v1]
        if part.dtype != torch.float32 or part.numel() != (v1 - v0) * H * W * 3 or part.shape[-1] != 3:
            raise bad
        return part.to(device).reshape(v1 - v0, H, W, 3).contiguous()
    out = torch.empty((v1 - v0, H, W, 3), dtype=torch.float32, device=device)
    for k in range(v0, v1):
        im = torch.as_tensor(images[k])
        if im.dtype != torch.float32 or im.numel() != H * W * 3 or im.shape[-1] != 3:
            raise bad
        out[k - v0].copy_(im.reshape(H, W, 3))
    return out


def _blend_views(what, mesh, points_of, intrinsics, pose, images, img_res, masks, view_bytes, device, **rules):
    """(verts, faces, normals, acc, n_used, n_skipped) - the loop color_mesh and texture_mesh share: per chunk of
    `view_bytes` of views the images (and masks) are uploaded, the depth maps of the MESH are drawn
    (ops.mesh_depth_maps) and ops.mesh_vertex_colors continues the accumulators of the POINTS.  points_of(verts, faces,
    normals) gives the (points, normals) to colour; None colours the mesh's own vertices.  n_skipped: a tuple, per
    view the faces mesh_depth_maps could not draw."""
    if not (isinstance(view_bytes, int) and view_bytes > 0):
        raise ValueError(f"hashmod {what}: view_bytes must be a positive integer")
    if rules["mode"] not in ops.COLOR_MODES:
        raise ValueError(f"hashmod {what}: mode must be 'blend' or 'best'")
    H, W = int(img_res[0]), int(img_res[1])
    proj = view_projections(intrinsics, pose)
    n = len(proj)
    c2w = np.asarray(pose.cpu() if isinstance(pose, torch.Tensor) else pose, np.float64)
    centers = np.ascontiguousarray(c2w[:, :3, 3]) if n else np.zeros((0, 3))
    if len(images) != n or (masks is not None and len(masks) != n):
        raise ValueError(f"hashmod {what}: one image (and one mask) per view expected")
    if device is None:
        for t in (images, masks):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                device = t.device
    verts, faces, normals = _device_mesh(mesh, "cuda" if device is None else device)
    dev = verts.device
    points, point_normals = (verts, normals) if points_of is None else points_of(verts, faces, normals)
    n_points = int(points.shape[0])
    acc = torch.zeros((n_points, 4), dtype=torch.float64, device=dev)
    n_used = torch.zeros(n_points, dtype=torch.int32, device=dev)
    per = max(1, view_bytes // (4 * H * W + 12 * H * W + (4 * (H + 1) * (W + 1) if masks is not None else 0)))
    skipped = []
    for v0 in range(0, n, per):
        v1 = min(v0 + per, n)
        img = _view_images(images, v0, v1, H, W, dev, what)
        msk = None
        if masks is not None:
            msk = masks[v0:v1]
            if not isinstance(msk, torch.Tensor):
                msk = torch.stack([torch.as_tensor(m) for m in msk])
            if msk.numel() != (v1 - v0) * H * W:
                raise ValueError(f"hashmod {what}: masks must be [n, H, W] (or [n, H*W]) with img_res = (H, W)")
            msk = msk.to(dev).reshape(v1 - v0, H, W)
        depth, sk = ops.mesh_depth_maps(verts, faces, proj[v0:v1], H, W)
        ops.mesh_vertex_colors(points, point_normals, proj[v0:v1], centers[v0:v1], img, depth, masks=msk,
                               out=(acc, n_used), **rules)
        skipped.append(sk)
    n_skipped = tuple(torch.cat(skipped).tolist()) if skipped else ()
    return verts, faces, normals, acc, n_used, n_skipped


def color_mesh(mesh, intrinsics, pose, images, img_res, *, masks=None, erode=1, pad=1, tol=0.0, min_cos=0.0, power=1,
               mode="blend", fill=(0.0, 0.0, 0.0), view_bytes=1 << 28, device=None):
    """(colors [V,3] fp32 on the device, ColorStats) of `mesh` seen by the input views.

    `mesh` is as for cull_mesh: a (verts, faces[, normals]) tuple of device tensors, or a TriMesh, which is uploaded
    (to `device`, else to the device of a tensor among images and masks that is on one, else to the current one).  It
    must be in the cameras' normalised frame: BEFORE apply_transform(scale_mat).  intrinsics, pose [n,4,4] and
    img_res = (H, W) are a SceneDataset's; images fp32 [n,H,W,3] or [n,H*W,3], or a list of per-view [H*W,3] tensors as
    SceneDataset.rgb_images holds them, on the host or the device; masks [n,H,W] or [n,H*W] bool / uint8, a tensor or a
    list of per-view tensors, or None.

    The views are taken `view_bytes` at a time, counting a view's depth map, image and mask table: each chunk uploads
    its images (and masks), draws the mesh's depth maps (ops.mesh_depth_maps) and continues the accumulators of
    ops.mesh_vertex_colors, whose rules (pad, tol, erode, min_cos, power, mode) are stated there; the result does not
    depend on view_bytes.  Without normals every visible view weighs 1.  erode=1 keeps the four bilinear taps inside
    the mask.  ops.mesh_colors_finish gives `fill` to a vertex no view contributed to.

    ColorStats: n_verts; n_colored the vertices with at least one view; n_skipped per view (a tuple: the faces
    mesh_depth_maps could not draw).  Only counts come to the host.  colors_to_uint8 (utils.plots) turns the dataset's
    [-1, 1] range into the bytes TriMesh(vertex_colors=) exports."""
    verts, faces, normals, acc, n_used, skipped = _blend_views("color_mesh", mesh, None, intrinsics, pose, images,
                                                               img_res, masks, view_bytes, device, erode=erode, pad=pad,
                                                               tol=tol, min_cos=min_cos, power=power, mode=mode)
    colors = ops.mesh_colors_finish(acc, n_used, mode, fill)
    n_colored = (n_used > 0).sum()
    return colors, ColorStats(int(verts.shape[0]), int(n_colored), skipped)


def color_mesh_for_dataset(mesh, dataset, **kw):
    """color_mesh with intrinsics_all, pose_all, rgb_images, object_masks and img_res of a SceneDataset (images and
    masks are uploaded chunk by chunk to the mesh's device).  masks=None in `kw` colours without the masks.  The mesh
    must be in the dataset's normalised frame: before apply_transform(scale_mat)."""
    device = kw.pop("device", None)
    if device is None and isinstance(mesh, (tuple, list)) and isinstance(mesh[0], torch.Tensor):
        device = mesh[0].device
    masks = kw.pop("masks", list(dataset.object_masks))
    return color_mesh(mesh, torch.stack(list(dataset.intrinsics_all)), torch.stack(list(dataset.pose_all)),
                      list(dataset.rgb_images), dataset.img_res, masks=masks,
                      device="cuda" if device is None else device, **kw)
