"""The reference's DTU Chamfer evaluation (code/evaluation/dtu_eval) of a mesh against a point cloud, on the device:
upsample every triangle to a point density, nearest-neighbour distances both ways, means below a cut-off.

Not part of it (DESIGN.md "Chamfer evaluation on the device"): DTU's greedy radius down-sampling of the sampled cloud
and its observation-mask and ground-plane filters."""
import numpy as np
import torch

from .. import ops
from ..utils.plots import TriMesh


def _device_mesh(mesh, device):
    if isinstance(mesh, TriMesh):
        verts = torch.from_numpy(np.ascontiguousarray(mesh.vertices, np.float32)).to(device)
        faces = torch.from_numpy(np.ascontiguousarray(mesh.faces, np.int32)).to(device)
        return verts, faces
    if isinstance(mesh, (tuple, list)) and len(mesh) in (2, 3):
        return mesh[0], mesh[1]
    raise ValueError("hashmod mesh_chamfer: mesh must be a TriMesh or a (verts, faces[, normals]) tuple")


def mesh_chamfer(mesh, target_points, density, max_dist=None):
    """ops.ChamferResult (with n_cloud) of a mesh against target_points [T,3] fp32 on the GPU.  `mesh` is a
    (verts, faces[, normals]) tuple of device tensors as ops.marching_cubes or ops.mesh_largest_component return
    them, or a TriMesh, which is uploaded to the target's device.  The mesh's cloud is cat(verts,
    ops.mesh_sample_surface(verts, faces, density)) - the DTU order - and the result is ops.chamfer_distance(cloud,
    target_points, max_dist): mean_a2b is mesh -> target (accuracy), mean_b2a target -> mesh (completeness).  Only the
    scalars come back to the host."""
    if not isinstance(target_points, torch.Tensor):
        raise ValueError("hashmod mesh_chamfer: target_points must be a tensor")
    verts, faces = _device_mesh(mesh, target_points.device)
    cloud = torch.cat([verts, ops.mesh_sample_surface(verts, faces, density)])
    r = ops.chamfer_distance(cloud, target_points, max_dist)
    return ops.ChamferResult(r.mean_a2b, r.mean_b2a, r.n_a2b, r.n_b2a, int(cloud.shape[0]))
