"""The mesh on the tracer's own rays, on the device: cast_camera_rays casts the rays of ops.camera_rays - the rays the
network's sphere tracer marches, with unit directions - at a mesh (ops.MeshIndex.ray_cast, csrc/hm_mesh_ray.hip), so
that its t is the same quantity as the tracer's Euclidean `dists`; depth_agreement puts two such depths side by
side.  That comparison is the direct measure of what marching cubes, simplification and culling did to the surface
the renderer sees.  DESIGN.md "Rays against the mesh on the device" states the contract."""
import math
from collections import namedtuple

import torch

from .. import ops
from .._lib import HashmodArgumentError

DepthAgreement = namedtuple("DepthAgreement", "n n_both iou mean median max")


def _as_ray_index(what, mesh_or_index):
    """a MeshIndex as it is (its own pad: build it with ops.mesh_ray_pad), or a (verts, faces) pair indexed with the
    defaults of ops.mesh_ray_cast"""
    if isinstance(mesh_or_index, ops.MeshIndex):
        return mesh_or_index
    if isinstance(mesh_or_index, (tuple, list)) and len(mesh_or_index) in (2, 3):
        return ops.mesh_ray_index(mesh_or_index[0], mesh_or_index[1])
    raise ValueError(f"hashmod {what}: the mesh must be a MeshIndex or a (verts, faces) pair")


def cast_camera_rays(mesh_or_index, uv, pose, intrinsics, radius=None):
    """(t [B,N] fp32, face [B,N] int32, hit [B,N] bool): the first hit on the mesh - a MeshIndex built with a pad, or a
    (verts, faces) pair, indexed here as ops.mesh_ray_cast does - of the rays through the pixels uv [B,N,2] of the
    cameras pose, intrinsics [B,4,4]: the rays of ops.camera_rays, whose directions have unit length, so that t is the
    Euclidean distance from the camera centre, the tracer's `dists`.  With `radius` (> 0) the range of a ray is its
    interval inside the bounding sphere of that radius about the origin, and a ray that misses the sphere is a miss:
    the tracer's domain.  A miss has t = inf and face -1.  Not graph-capturable."""
    what = "cast_camera_rays"
    if radius is not None and not (isinstance(radius, (int, float)) and not isinstance(radius, bool)
                                   and math.isfinite(radius) and radius > 0):
        raise ValueError(f"hashmod {what}: radius must be a positive finite number (or None)")
    if not isinstance(uv, torch.Tensor) or uv.dim() != 3 or uv.shape[2] != 2:
        raise ValueError(f"hashmod {what}: uv must be a tensor [B,N,2]")
    for name, t in (("pose", pose), ("intrinsics", intrinsics)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (uv.shape[0], 4, 4):
            raise ValueError(f"hashmod {what}: {name} must be a tensor [B,4,4]")
    if not (isinstance(mesh_or_index, ops.MeshIndex) or (isinstance(mesh_or_index, (tuple, list))
                                                         and len(mesh_or_index) in (2, 3))):
        raise ValueError(f"hashmod {what}: the mesh must be a MeshIndex or a (verts, faces) pair")
    if not uv.is_cuda:
        raise HashmodArgumentError(f"hashmod {what}: the tensors must be on a GPU; there is no CPU path")
    index = _as_ray_index(what, mesh_or_index)
    Bn, N = int(uv.shape[0]), int(uv.shape[1])
    dirs, cam, t_sphere, in_sphere = ops.camera_rays(uv, pose, intrinsics, 1.0 if radius is None else radius)
    origins = cam[:, None, :].expand(Bn, N, 3).reshape(-1, 3).contiguous()
    if radius is None:
        t_min, t_max = 0.0, math.inf
    else:
        # an empty range (t_min > t_max) for a ray that misses the sphere
        inside = in_sphere.reshape(-1)
        t_min = torch.where(inside, t_sphere[..., 0].reshape(-1), torch.ones((), device=uv.device)).contiguous()
        t_max = torch.where(inside, t_sphere[..., 1].reshape(-1), torch.zeros((), device=uv.device)).contiguous()
    t, face = index.ray_cast(origins, dirs.reshape(-1, 3), t_min, t_max, return_uv=False)
    return t.view(Bn, N), face.view(Bn, N), (face >= 0).view(Bn, N)


def depth_agreement(t_a, hit_a, t_b, hit_b):
    """DepthAgreement(n, n_both, iou, mean, median, max) of two depths on the same rays - t_a, t_b fp32 of one shape
    with their bool hit masks, for instance cast_camera_rays' (t, hit) against the sphere tracer's (dists, mask), or
    two meshes against each other: n rays, n_both hit by both, the intersection over union of the two hit masks
    (nan when neither hits anything), and the mean, median (the lower of the two middle values for an even count) and
    maximum of |t_a - t_b| over the rays hit by both (nan when there are none).  The differences and the reductions
    are fp64 on the device; one host read."""
    what = "depth_agreement"
    tensors = (t_a, hit_a, t_b, hit_b)
    if not all(isinstance(t, torch.Tensor) for t in tensors):
        raise ValueError(f"hashmod {what}: tensors expected")
    if t_a.dtype != torch.float32 or t_b.dtype != torch.float32:
        raise ValueError(f"hashmod {what}: fp32 depths expected")
    if hit_a.dtype != torch.bool or hit_b.dtype != torch.bool:
        raise ValueError(f"hashmod {what}: bool hit masks expected")
    if not (t_a.shape == hit_a.shape == t_b.shape == hit_b.shape):
        raise ValueError(f"hashmod {what}: the four tensors must have one shape")
    if len({t.device for t in tensors}) != 1:
        raise ValueError(f"hashmod {what}: the tensors are on different devices")
    if not t_a.is_cuda:
        raise HashmodArgumentError(f"hashmod {what}: the tensors must be on a GPU; there is no CPU path")
    n = t_a.numel()
    both = hit_a & hit_b
    diff = (t_a.to(torch.float64) - t_b.to(torch.float64)).abs()[both]
    nan = torch.full((), math.nan, dtype=torch.float64, device=t_a.device)
    if diff.numel():                       # the shape of a masked selection is a host read already
        stats = [diff.mean(), diff.median(), diff.max()]
    else:
        stats = [nan, nan, nan]
    n_both, n_any, mean, median, mx = torch.stack([both.sum().to(torch.float64),
                                                   (hit_a | hit_b).sum().to(torch.float64)] + stats).tolist()
    return DepthAgreement(n, int(n_both), n_both / n_any if n_any else math.nan, mean, median, mx)
