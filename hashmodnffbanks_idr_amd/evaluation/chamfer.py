"""The reference's DTU Chamfer evaluation (code/evaluation/dtu_eval) of a mesh against a point cloud, on the device.

mesh_chamfer: upsample every triangle to a point density, nearest-neighbour distances both ways, means below a
cut-off; with surface=True the completeness side is the exact distance to the triangles.  mesh_to_mesh: the points of
each mesh against the triangles of the other (ops.mesh_closest_point), means and maxima.  dtu_chamfer: the whole DTU protocol - the sampled cloud is shuffled and thinned by the greedy radius rule
(ops.radius_downsample), cut to the scan's padded bounding box and observation mask (ops.dtu_point_flags), the scan is
cut at its ground plane, and accuracy and completeness are the one-sided means (ops.one_sided_distance) between what
is left.  load_dtu_scan reads a scan's mask and plane files.  DESIGN.md "Chamfer evaluation on the device" states the
contracts."""
import math
import os
from collections import namedtuple

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


def mesh_chamfer(mesh, target_points, density, max_dist=None, surface=False):
    """ops.ChamferResult (with n_cloud) of a mesh against target_points [T,3] fp32 on the GPU.  `mesh` is a
    (verts, faces[, normals]) tuple of device tensors as ops.marching_cubes or ops.mesh_largest_component return
    them, or a TriMesh, which is uploaded to the target's device.  The mesh's cloud is cat(verts,
    ops.mesh_sample_surface(verts, faces, density)) - the DTU order - and the result is ops.chamfer_distance(cloud,
    target_points, max_dist): mean_a2b is mesh -> target (accuracy), mean_b2a target -> mesh (completeness).  With
    surface=True the completeness side is ops.point_mesh_distance(target_points, mesh, max_dist): the exact distance
    to the triangles instead of the distance to the sampled cloud, which cannot see below the sampling density; the
    accuracy side is the same bits (ops.one_sided_distance).  Only the scalars come back to the host."""
    if not isinstance(target_points, torch.Tensor):
        raise ValueError("hashmod mesh_chamfer: target_points must be a tensor")
    if not isinstance(surface, bool):
        raise ValueError("hashmod mesh_chamfer: surface must be a bool")
    verts, faces = _device_mesh(mesh, target_points.device)
    cloud = torch.cat([verts, ops.mesh_sample_surface(verts, faces, density)])
    if not surface:
        r = ops.chamfer_distance(cloud, target_points, max_dist)
        return ops.ChamferResult(r.mean_a2b, r.mean_b2a, r.n_a2b, r.n_b2a, int(cloud.shape[0]))
    ops._check_cloud("mesh_chamfer", "target_points", target_points, cloud)
    if cloud.shape[0] < 1 or target_points.shape[0] < 1:
        raise ValueError("hashmod mesh_chamfer: the mesh's cloud and the target need at least one point")
    acc, n_acc = ops.one_sided_distance(cloud, target_points, max_dist)
    comp, n_comp = ops.point_mesh_distance(target_points, (verts, faces), max_dist)
    return ops.ChamferResult(acc, comp, n_acc, n_comp, int(cloud.shape[0]))


MeshToMeshResult = namedtuple("MeshToMeshResult", ["mean_a2b", "mean_b2a", "max_a2b", "max_b2a", "n_a2b", "n_b2a"])


def mesh_to_mesh(mesh_a, mesh_b, density, max_dist=None):
    """MeshToMeshResult of two meshes (each as for mesh_chamfer; device tensors of one GPU, or TriMeshes with
    device tensors on the other side): the points of each mesh - cat(verts, ops.mesh_sample_surface(verts, faces,
    density)) - against the TRIANGLES of the other (ops.mesh_closest_point).  mean_a2b is the mean exact distance from
    a's points to b's surface over the distances < max_dist (strict; all for None), max_a2b the largest of them (a
    sampled one-sided Hausdorff distance), n_a2b their number; the b2a fields the other way.  The distances are the
    fp64 square roots of the exact fp32 d2, so that - unlike a distance between two sampled clouds - the figures do
    not stop at the sampling density of the side measured against.  No distance below max_dist gives nan and count 0.
    Only the scalars come to the host."""
    if not (isinstance(density, (int, float)) and math.isfinite(density) and density > 0):
        raise ValueError("hashmod mesh_to_mesh: density must be a positive finite number")
    if max_dist is not None and not (isinstance(max_dist, (int, float)) and max_dist > 0):
        raise ValueError("hashmod mesh_to_mesh: max_dist must be a positive number (or None)")
    dev = next((t.device for m in (mesh_a, mesh_b) if isinstance(m, (tuple, list)) for t in m[:1]
                if isinstance(t, torch.Tensor)), None)
    if dev is None:
        raise ValueError("hashmod mesh_to_mesh: at least one mesh must be a tuple of device tensors")
    sides = []
    for mesh in (mesh_a, mesh_b):
        verts, faces = _device_mesh(mesh, dev)
        sides.append((torch.cat([verts, ops.mesh_sample_surface(verts, faces, density)]),
                      ops.mesh_index(verts, faces)))
    (pa, ia), (pb, ib) = sides
    sa, ca, ma, sb, cb, mb = torch.cat([ops._point_mesh_sums(pa, ib, max_dist)[0],
                                        ops._point_mesh_sums(pb, ia, max_dist)[0]]).tolist()
    return MeshToMeshResult(sa / ca if ca else math.nan, sb / cb if cb else math.nan, ma if ca else math.nan,
                            mb if cb else math.nan, int(ca), int(cb))


DtuChamferResult = namedtuple("DtuChamferResult", ["accuracy", "completeness", "overall", "n_cloud", "n_down", "n_in",
                                                   "n_in_obs", "n_stl_above", "n_d2s", "n_s2d"])


def dtu_chamfer(mesh, stl_points, *, obs_mask, bb, res, plane, density=0.2, patch=60, max_dist=20, shuffle_seed=1,
                order=None):
    """DtuChamferResult of a mesh against a DTU scan's cloud stl_points [T,3] fp32 on the GPU, as the reference's
    evaluation/dtu_eval computes it (`mesh` as for mesh_chamfer; obs_mask [X,Y,Z] uint8 on the GPU, bb [2,3], res and
    plane [4] as load_dtu_scan returns them):
        data      = cat(verts, ops.mesh_sample_surface(verts, faces, density))[order]              n_cloud
        data_down = data[ops.radius_downsample(data, density)]                                      n_down
        data_in   = data_down inside [bb[0] - patch, bb[1] + 2*patch)                               n_in
        in_obs    = data_in whose voxel around((p - bb[0])/res) is set in obs_mask                  n_in_obs
        accuracy     = mean of the distances in_obs -> stl_points that are < max_dist               n_d2s
        stl_above = stl_points with ((P0*x + P1*y) + P2*z) + P3 > 0                                 n_stl_above
        completeness = mean of the distances stl_above -> data_in that are < max_dist               n_s2d
        overall   = (accuracy + completeness)/2
    `order` is a permutation of the cloud as an int64 device tensor; without it the cloud is shuffled by
    torch.randperm of a device generator seeded with shuffle_seed (the reference shuffles with numpy's seeded
    generator: another, equally arbitrary, order).  A mean over no distance is nan.  Only scalars come to the host."""
    if not isinstance(stl_points, torch.Tensor):
        raise ValueError("hashmod dtu_chamfer: stl_points must be a tensor")
    for name, v in (("density", density), ("max_dist", max_dist)):
        if not (isinstance(v, (int, float)) and math.isfinite(v) and v > 0):
            raise ValueError(f"hashmod dtu_chamfer: {name} must be a positive finite number")
    ops._check_cloud("dtu_chamfer", "stl_points", stl_points)
    ops._dtu_params("dtu_chamfer", obs_mask, bb, res, patch, plane)
    dev = stl_points.device
    verts, faces = _device_mesh(mesh, dev)
    cloud = torch.cat([verts, ops.mesh_sample_surface(verts, faces, density)])
    n_cloud = int(cloud.shape[0])
    if order is None:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(shuffle_seed))
        order = torch.randperm(n_cloud, generator=gen, device=dev)
    elif (not isinstance(order, torch.Tensor) or order.dtype != torch.int64 or order.shape != (n_cloud,)
          or order.device != dev):
        raise ValueError(f"hashmod dtu_chamfer: order must be an int64 permutation [{n_cloud}] on the cloud's device")
    data = cloud[order]
    data_down = data[ops.radius_downsample(data, density)]
    flags = ops.dtu_point_flags(data_down, obs_mask, bb, res, patch, plane)
    data_in = data_down[(flags & ops.DTU_INBOUND) != 0]
    both = ops.DTU_INBOUND | ops.DTU_IN_MASK
    in_obs = data_down[(flags & both) == both]
    above = (ops.dtu_point_flags(stl_points, obs_mask, bb, res, patch, plane) & ops.DTU_ABOVE_PLANE) != 0
    stl_above = stl_points[above]
    acc, n_d2s = ops.one_sided_distance(in_obs, stl_points, max_dist)
    comp, n_s2d = ops.one_sided_distance(stl_above, data_in, max_dist)
    return DtuChamferResult(acc, comp, 0.5 * (acc + comp), n_cloud, int(data_down.shape[0]), int(data_in.shape[0]),
                            int(in_obs.shape[0]), int(stl_above.shape[0]), n_d2s, n_s2d)


def load_dtu_scan(dataset_dir, scan):
    """dict(obs_mask uint8 [X,Y,Z] numpy, bb float64 [2,3], res float, plane float64 [4]) of a DTU scan: the ObsMask,
    BB and Res of ObsMask{scan}_10.mat and the P of Plane{scan}.mat, looked for in dataset_dir/ObsMask and then in
    dataset_dir itself.  Upload obs_mask with torch.from_numpy(...).to(device) for dtu_chamfer."""
    from scipy.io import loadmat
    found = {}
    for name in (f"ObsMask{scan}_10.mat", f"Plane{scan}.mat"):
        for folder in (os.path.join(dataset_dir, "ObsMask"), dataset_dir):
            if os.path.isfile(os.path.join(folder, name)):
                found[name] = loadmat(os.path.join(folder, name))
                break
        else:
            raise FileNotFoundError(f"hashmod load_dtu_scan: {name} is neither in {dataset_dir}/ObsMask nor in "
                                    f"{dataset_dir}")
    obs, plane = found[f"ObsMask{scan}_10.mat"], found[f"Plane{scan}.mat"]
    out = {"obs_mask": np.ascontiguousarray(obs["ObsMask"] != 0, np.uint8),
           "bb": np.ascontiguousarray(obs["BB"], np.float64).reshape(2, 3),
           "res": float(np.asarray(obs["Res"], np.float64).reshape(-1)[0]),
           "plane": np.ascontiguousarray(plane["P"], np.float64).reshape(4)}
    if out["obs_mask"].ndim != 3:
        raise ValueError("hashmod load_dtu_scan: ObsMask is not a volume")
    return out
