"""Looking at an extracted mesh through the cameras, on the device: its vertex colours, its normals or its depth drawn
into every input view (ops.mesh_render: a visibility buffer and perspective-correct interpolation), and the coloured
mesh scored against the photographs it was coloured from with the PSNR and SSIM of the rendered views
(images.view_metrics).  The reference's eval.py draws its normal and depth plots by sphere-tracing the network; the
mesh is already on the device and is rasterised instead.  An addition, off unless it is called.  DESIGN.md "Rendering
the mesh" states the contract."""
import os
from collections import namedtuple

import numpy as np
import torch

from .. import ops
from ..utils.plots import TriMesh
from .cull import _device_mesh, view_projections
from .images import ViewScores, _write_csv, view_metrics

MeshViews = namedtuple("MeshViews", ["rgb", "coverage", "depth", "face_id", "n_skipped"])
SHADES = ("color", "normal", "depth")


def _vertex_attrs(mesh, verts, normals, colors, shade):
    """[V,3] fp32 in [0,1] on the device for shade "color" or "normal"; None for "depth" """
    dev, n_verts = verts.device, int(verts.shape[0])
    if shade == "depth":
        return None
    if shade == "normal":
        if normals is None and isinstance(mesh, TriMesh):
            normals = torch.from_numpy(np.ascontiguousarray(mesh.vertex_normals, np.float32)).to(dev)
        if normals is None:
            raise ValueError("hashmod render_mesh: shade='normal' needs the mesh's normals")
        return ((normals + 1.0) / 2.0).contiguous()
    if colors is not None:
        if (not isinstance(colors, torch.Tensor) or colors.dtype != torch.float32 or tuple(colors.shape) != (n_verts, 3)
                or colors.device != dev):
            raise ValueError("hashmod render_mesh: colors must be fp32 [V, 3] in [-1, 1] on the mesh's device")
        return ((colors + 1.0) / 2.0).clamp(0.0, 1.0).contiguous()
    if isinstance(mesh, TriMesh) and mesh.vertex_colors is not None:
        return (torch.from_numpy(np.ascontiguousarray(mesh.vertex_colors)).to(dev).float() / 255.0).contiguous()
    raise ValueError("hashmod render_mesh: shade='color' needs colors= or a TriMesh with vertex_colors")


def render_mesh(mesh, intrinsics, pose, img_res, *, colors=None, texture=None, shade="color", background=1.0,
                view_bytes=1 << 28, device=None):
    """MeshViews(rgb [n,H,W,3] fp32 in [0,1], coverage [n,H,W] bool, depth [n,H,W] fp32, face_id [n,H,W] int32,
    n_skipped [n] int32) of `mesh` seen by the cameras, on the device.

    `mesh` is as for color_mesh: a (verts, faces[, normals]) tuple of device tensors, or a TriMesh, which is uploaded
    (to `device`, else to the current one); it must be in the cameras' normalised frame, BEFORE
    apply_transform(scale_mat).  intrinsics, pose [n,4,4] and img_res = (H, W) are a SceneDataset's.  `shade`:
      "color"   the vertex colours: colors= fp32 [V,3] in the dataset's [-1, 1] range on the device (color_mesh's
                result), mapped by (c + 1) / 2 and clamped to [0, 1]; else a TriMesh's uint8 vertex_colors / 255;
                or texture= an ops.TextureAtlas of this mesh (texture_mesh's result) in the same range: its texels get
                the same map, and every pixel's colour is ops.mesh_texture_sample at the visibility buffer's face and
                perspective-correct weights (ops.mesh_render(return_weights=True)) instead of interpolated attributes
      "normal"  the world vertex normals mapped by (n + 1) / 2, the reference's normal-map convention
      "depth"   the depth along the camera's axis divided by the view's largest depth over its covered pixels, as grey
    interpolated perspective-correctly over the nearest face of every pixel (ops.mesh_render states the rules: no
    clipping, no anti-aliasing, no lighting); a pixel no face covers is `background` (a float or three).  The views are
    taken `view_bytes` at a time, counting a view's ids, depth, image and result (and, with a texture, its weights);
    the result does not depend on it."""
    chunks = list(_render_chunks(mesh, intrinsics, pose, img_res, colors, shade, background, view_bytes, device,
                                 texture))
    if not chunks:
        raise ValueError("hashmod render_mesh: no view to render")
    rgb, face_id, depth, n_skipped = (torch.cat([c[k] for c in chunks]) for k in range(4))
    return MeshViews(rgb, face_id >= 0, depth, face_id, n_skipped)


def _render_chunks(mesh, intrinsics, pose, img_res, colors, shade, background, view_bytes, device, texture=None):
    """render_mesh's work: yields (rgb, face_id, depth, n_skipped) of `view_bytes` of views at a time, in order"""
    if shade not in SHADES:
        raise ValueError("hashmod render_mesh: shade must be 'color', 'normal' or 'depth'")
    if not (isinstance(view_bytes, int) and view_bytes > 0):
        raise ValueError("hashmod render_mesh: view_bytes must be a positive integer")
    H, W = int(img_res[0]), int(img_res[1])
    proj = view_projections(intrinsics, pose)
    verts, faces, normals = _device_mesh(mesh, "cuda" if device is None else device)
    if texture is not None:
        if shade != "color" or colors is not None:
            raise ValueError("hashmod render_mesh: texture= goes with shade='color' and without colors=")
        if (not isinstance(texture, ops.TextureAtlas) or texture.n_faces != int(faces.shape[0])
                or texture.texels.device != verts.device):
            raise ValueError("hashmod render_mesh: texture must be an ops.TextureAtlas of this mesh on its device")
        texels = ((texture.texels + 1.0) / 2.0).clamp(0.0, 1.0).contiguous()
    attrs = None if texture is not None else _vertex_attrs(mesh, verts, normals, colors, shade)
    bg = torch.as_tensor(background, dtype=torch.float32).reshape(-1)
    if bg.numel() not in (1, 3):
        raise ValueError("hashmod render_mesh: background must be a float or three floats")
    bg = bg.expand(3).contiguous()
    per = max(1, view_bytes // ((33 if texture is None else 45) * H * W))
    for v0 in range(0, len(proj), per):
        r = ops.mesh_render(verts, faces, proj[v0:v0 + per], H, W, attrs=attrs,
                            background=0.0 if attrs is None else bg.tolist(), return_weights=texture is not None)
        if texture is not None:
            rgb = ops.mesh_texture_sample(texels, texture.res, texture.n_faces, r.face_id, r.weights,
                                          bg.tolist()).clamp_(0.0, 1.0)
        elif shade == "depth":
            on = r.face_id >= 0
            far = torch.where(on, r.depth, torch.zeros_like(r.depth)).amax(dim=(1, 2), keepdim=True)
            grey = (r.depth / far)[..., None].expand(-1, -1, -1, 3)
            rgb = torch.where(on[..., None], grey, bg.to(verts.device))
        else:
            rgb = r.image.clamp_(0.0, 1.0)
        yield rgb, r.face_id, r.depth, r.n_skipped


def evaluate_mesh_views(mesh, dataset, indices=None, out_dir=None, save_png=False, **kw):
    """ViewScores(indices, psnrs, ssims, psnr_mean, ssim_mean) of the coloured `mesh` drawn into the views `indices`
    (default: all) of a SceneDataset-like dataset (intrinsics_all, pose_all, rgb_images [H*W,3] in [-1,1], object_masks
    [H*W], img_res) against its photographs: render_mesh(shade="color") over white, then images.view_metrics per view
    in evaluate_views' convention - PSNR over the dataset's object mask, SSIM of the two images composited over white
    outside it; a pixel of the mask the mesh does not cover is white.  `kw` goes to render_mesh (colors= or texture=,
    view_bytes=, device=).  Each view's photograph and mask are uploaded, two scalars per view come to the host and nothing else
    does.  With out_dir, mesh_psnrs.csv and mesh_ssims.csv are written there in evaluate_views' layout, and with
    save_png also mesh_<index>.png, the rendered views.  The mesh must be in the dataset's normalised frame, as for
    color_mesh."""
    for k in kw:
        if k not in ("colors", "texture", "view_bytes", "device"):
            raise TypeError(f"hashmod evaluate_mesh_views: unexpected argument {k!r}")
    indices = list(range(len(dataset.rgb_images))) if indices is None else [int(i) for i in indices]
    if not indices:
        raise ValueError("hashmod evaluate_mesh_views: no view to evaluate")
    if save_png and out_dir is None:
        raise ValueError("hashmod evaluate_mesh_views: save_png needs out_dir")
    H, W = int(dataset.img_res[0]), int(dataset.img_res[1])
    device = kw.get("device")
    if device is None and isinstance(mesh, (tuple, list)) and isinstance(mesh[0], torch.Tensor):
        device = mesh[0].device
    K = torch.stack([torch.as_tensor(dataset.intrinsics_all[i]) for i in indices])
    pose = torch.stack([torch.as_tensor(dataset.pose_all[i]) for i in indices])
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    psnrs, ssims = [], []
    for rgb, _, _, _ in _render_chunks(mesh, K, pose, (H, W), kw.get("colors"), "color", 1.0,
                                       kw.get("view_bytes", 1 << 28), device, kw.get("texture")):
        for view in rgb:
            i = indices[len(psnrs)]
            gt = torch.as_tensor(dataset.rgb_images[i]).to(view.device)
            mask = torch.as_tensor(dataset.object_masks[i]).to(view.device)
            psnr, ssim = view_metrics(view.reshape(H * W, 3) * 2.0 - 1.0, gt, mask, (H, W))
            p, s = torch.stack([psnr, ssim]).tolist()
            psnrs.append(p)
            ssims.append(s)
            if save_png:
                from PIL import Image
                Image.fromarray((view * 255.0).round().to(torch.uint8).cpu().numpy()).save(
                    os.path.join(out_dir, f"mesh_{i}.png"))
    scores = ViewScores(indices, psnrs, ssims, sum(psnrs) / len(psnrs), sum(ssims) / len(ssims))
    if out_dir is not None:
        _write_csv(os.path.join(out_dir, "mesh_psnrs.csv"), psnrs, scores.psnr_mean)
        _write_csv(os.path.join(out_dir, "mesh_ssims.csv"), ssims, scores.ssim_mean)
    return scores
