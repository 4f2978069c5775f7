"""Culling an extracted mesh by what the cameras saw, on the device: the step mask-supervised IDR-style reconstructions
run between extraction and scoring.  Geometry that projects outside the (dilated) object masks - the blobs and skirts
the mask loss never saw from a training view - and geometry hidden from every camera - interior shells, the closed
underside, double walls - inflate the accuracy half of the Chamfer distance.  The reference's eval.py has no such
step: it is an addition, off unless it is called.

cull_mesh: per-vertex view votes against the masks (ops.mesh_mask_votes), depth maps of the mask-culled mesh
(ops.mesh_depth_maps), per-vertex visibility votes against them (ops.mesh_visible_votes), compaction
(ops.mesh_keep_vertices).  DESIGN.md "Mesh culling on the device" states the contracts and the limits."""
from collections import namedtuple

import numpy as np
import torch

from .. import ops
from ..utils.plots import TriMesh

CullStats = namedtuple("CullStats", ["n_verts", "n_faces", "kept_by_masks", "kept_by_visibility", "n_verts_out",
                                     "n_faces_out", "n_skipped"])


def view_projections(intrinsics, pose):
    """P [n,3,4] float64 = K[:3,:3] @ inv(pose)[:3,:4] of the fp32 intrinsics [n,4,4] and camera-to-world poses [n,4,4]
    a SceneDataset holds (tensors or arrays), the inverse and the product taken in numpy float64 on the host.  Pixel
    (col, row) has its centre at uv = (col, row), the dataset's convention."""
    K = np.asarray(intrinsics.cpu() if isinstance(intrinsics, torch.Tensor) else intrinsics, np.float64)
    c2w = np.asarray(pose.cpu() if isinstance(pose, torch.Tensor) else pose, np.float64)
    if K.ndim != 3 or K.shape[1:] != (4, 4) or c2w.shape != K.shape:
        raise ValueError("hashmod view_projections: intrinsics [n,4,4] and pose [n,4,4] expected")
    return np.ascontiguousarray(K[:, :3, :3] @ np.linalg.inv(c2w)[:, :3, :4]) if len(K) else np.zeros((0, 3, 4))


def _device_mesh(mesh, device):
    if isinstance(mesh, TriMesh):
        verts = torch.from_numpy(np.ascontiguousarray(mesh.vertices, np.float32)).to(device)
        faces = torch.from_numpy(np.ascontiguousarray(mesh.faces, np.int32)).to(device)
        normals = mesh._normals     # the normals it was given; none are made up for a mesh without them
        if normals is not None:
            normals = torch.from_numpy(np.ascontiguousarray(normals, np.float32)).to(device)
        return verts, faces, normals
    if isinstance(mesh, (tuple, list)) and len(mesh) in (2, 3):
        return mesh[0], mesh[1], (mesh[2] if len(mesh) == 3 else None)
    raise ValueError("hashmod cull_mesh: mesh must be a TriMesh or a (verts, faces[, normals]) tuple")


def cull_mesh(mesh, intrinsics, pose, masks, img_res, *, dilate, mask_rule="all", min_views=None, visibility=True,
              pad=1, tol=0.0, largest_component=False, depth_bytes=1 << 28, device=None):
    """((verts, faces, normals), CullStats) of `mesh` without what no camera could have constrained.

    `mesh` is as for mesh_chamfer: a (verts, faces[, normals]) tuple of device tensors, or a TriMesh, which is uploaded
    (to `device`, else to the masks' device, else to the current one).  It must be in the cameras' normalised frame -
    the frame the network is trained in, i.e. BEFORE apply_transform(scale_mat) takes it to world coordinates.
    intrinsics, pose [n,4,4] and img_res = (H, W) are a SceneDataset's; masks [n,H,W] or [n,H*W] bool / uint8.

    1. masks (skipped with masks=None): ops.mesh_mask_votes with the pixel radius `dilate` - required, because
       published scripts use different radii and none is canonical.  mask_rule="all" keeps a vertex iff
       n_in_mask == n_in_image (a view that does not have the vertex in its image does not vote), mask_rule="min" iff
       n_in_mask >= min_views.  ops.mesh_keep_vertices drops every face with a dropped vertex.
    2. visibility (visibility=True): the depth maps of the mask-culled mesh are drawn `depth_bytes` of views at a time
       (ops.mesh_depth_maps) and a vertex is kept iff ops.mesh_visible_votes(pad, tol) sees it in at least one view.
       pad=1 is conservative at the silhouette: it keeps back-facing vertices within a pixel of the rim.
    3. largest_component=True ends with ops.mesh_largest_component.

    CullStats: n_verts, n_faces of the input; kept_by_masks, kept_by_visibility the vertices each rule kept (of the
    input and of the mask-culled mesh; None for a stage that did not run); n_verts_out, n_faces_out; n_skipped per view
    (a tuple: the faces mesh_depth_maps could not draw, None without visibility).  Only counts come to the host."""
    if masks is not None and not isinstance(masks, torch.Tensor):
        raise ValueError("hashmod cull_mesh: masks must be a tensor or None")
    if mask_rule not in ("all", "min"):
        raise ValueError("hashmod cull_mesh: mask_rule must be 'all' or 'min'")
    if masks is not None and mask_rule == "min" and not (isinstance(min_views, int) and min_views >= 0):
        raise ValueError("hashmod cull_mesh: mask_rule='min' needs an integer min_views >= 0")
    if not (isinstance(depth_bytes, int) and depth_bytes > 0):
        raise ValueError("hashmod cull_mesh: depth_bytes must be a positive integer")
    H, W = int(img_res[0]), int(img_res[1])
    proj = view_projections(intrinsics, pose)
    if device is None and masks is not None:
        device = masks.device
    verts, faces, normals = _device_mesh(mesh, "cuda" if device is None else device)
    n_verts, n_faces = int(verts.shape[0]), int(faces.shape[0])
    kept_masks = kept_vis = n_skipped = None
    if masks is not None:
        if masks.dim() == 2 and masks.shape[1] == H * W:
            masks = masks.reshape(-1, H, W)
        if masks.dim() != 3 or tuple(masks.shape) != (len(proj), H, W):
            raise ValueError("hashmod cull_mesh: masks must be [n, H, W] (or [n, H*W]) with img_res = (H, W)")
        n_img, n_msk = ops.mesh_mask_votes(verts, proj, masks, dilate)
        keep = (n_msk == n_img) if mask_rule == "all" else (n_msk >= min_views)
        kept_masks = keep.sum()
        verts, faces, normals = ops.mesh_keep_vertices(verts, faces, normals, keep)
    if visibility:
        per = max(1, depth_bytes // (4 * H * W))
        n_vis = torch.zeros(int(verts.shape[0]), dtype=torch.int32, device=verts.device)
        skipped = []
        for v0 in range(0, len(proj), per):
            depth, sk = ops.mesh_depth_maps(verts, faces, proj[v0:v0 + per], H, W)
            ops.mesh_visible_votes(verts, proj[v0:v0 + per], depth, pad, tol, out=n_vis)
            skipped.append(sk)
        keep = n_vis >= 1
        kept_vis = keep.sum()
        n_skipped = tuple(torch.cat(skipped).tolist()) if skipped else ()
        verts, faces, normals = ops.mesh_keep_vertices(verts, faces, normals, keep)
    if largest_component:
        verts, faces, normals = ops.mesh_largest_component(verts, faces, normals)
    stats = CullStats(n_verts, n_faces, None if kept_masks is None else int(kept_masks),
                      None if kept_vis is None else int(kept_vis), int(verts.shape[0]), int(faces.shape[0]), n_skipped)
    return (verts, faces, normals), stats


def cull_mesh_for_dataset(mesh, dataset, **kw):
    """cull_mesh with intrinsics_all, pose_all, object_masks and img_res of a SceneDataset (the masks are uploaded to
    the mesh's device).  The mesh must be in the dataset's normalised frame: before apply_transform(scale_mat)."""
    device = kw.pop("device", None)
    if device is None and isinstance(mesh, (tuple, list)) and isinstance(mesh[0], torch.Tensor):
        device = mesh[0].device
    device = "cuda" if device is None else device
    masks = torch.stack([torch.as_tensor(m) for m in dataset.object_masks]).to(device)
    return cull_mesh(mesh, torch.stack(list(dataset.intrinsics_all)), torch.stack(list(dataset.pose_all)), masks,
                     dataset.img_res, device=device, **kw)
