"""The mesh as a signed distance function, on the device: sdf_agreement puts a network's f(x) beside the signed
distance to the surface it produced (ops.mesh_signed_distance, csrc/hm_mesh_topo.hip) - the eikonal term only
encourages the two to agree - and volume_iou measures how much of space two reconstructions disagree on, through
ops.mesh_contains on a lattice.  DESIGN.md "Signed distance to the mesh on the device" states the contract."""
import math
from collections import namedtuple

import torch

from .. import ops
from .._lib import HashmodArgumentError

SdfAgreement = namedtuple("SdfAgreement", "n n_used sign_agreement mean median max")


def sdf_agreement(values, sd, band=None):
    """SdfAgreement(n, n_used, sign_agreement, mean, median, max) of two signed distances at the same points - values,
    sd [m] fp32, for instance a network's f(x) and ops.mesh_signed_distance's sd: n points, n_used of them with a
    finite sd (not cut by max_dist) and, with `band` (> 0), |sd| <= band; over those the share of equal signs (zero
    counts as positive), and the mean, median (the lower of the two middle values for an even count) and maximum of
    |values - sd|; nan when none is used.  The differences and the reductions are fp64 on the device; one host read."""
    what = "sdf_agreement"
    if not isinstance(values, torch.Tensor) or not isinstance(sd, torch.Tensor):
        raise ValueError(f"hashmod {what}: tensors expected")
    if values.dtype != torch.float32 or sd.dtype != torch.float32:
        raise ValueError(f"hashmod {what}: fp32 tensors expected")
    if values.dim() != 1 or values.shape != sd.shape:
        raise ValueError(f"hashmod {what}: values and sd must both have the shape [m]")
    if band is not None and not (isinstance(band, (int, float)) and not isinstance(band, bool) and band > 0):
        raise ValueError(f"hashmod {what}: band must be a positive number (or None)")
    if values.device != sd.device:
        raise ValueError(f"hashmod {what}: the tensors are on different devices")
    if not values.is_cuda:
        raise HashmodArgumentError(f"hashmod {what}: the tensors must be on a GPU; there is no CPU path")
    n = values.numel()
    s64 = sd.to(torch.float64)
    used = torch.isfinite(sd)
    if band is not None:
        used = used & (s64.abs() <= float(band))
    diff = (values.to(torch.float64) - s64).abs()[used]
    same = ((values >= 0) == (sd >= 0))[used]
    nan = torch.full((), math.nan, dtype=torch.float64, device=values.device)
    if diff.numel():                       # the shape of a masked selection is a host read already
        stats = [diff.mean(), diff.median(), diff.max()]
    else:
        stats = [nan, nan, nan]
    n_used, n_same, mean, median, mx = torch.stack([used.sum().to(torch.float64),
                                                    same.sum().to(torch.float64)] + stats).tolist()
    return SdfAgreement(n, int(n_used), n_same / n_used if n_used else math.nan, mean, median, mx)


def mesh_sdf_agreement(model_or_fn, mesh, points, band=None, chunk=1 << 18):
    """sdf_agreement of a callable's values against the mesh's signed distance at points [m,3] fp32: model_or_fn maps
    [k,3] points to k values ([k] or [k,1]; a network's f(x)) and is evaluated in chunks of `chunk` points under
    no_grad; `mesh` is a (MeshIndex, MeshTopology) or a (verts, faces) pair."""
    what = "mesh_sdf_agreement"
    if not callable(model_or_fn):
        raise ValueError(f"hashmod {what}: a callable is expected")
    if not (isinstance(chunk, int) and not isinstance(chunk, bool) and chunk >= 1):
        raise ValueError(f"hashmod {what}: chunk must be an integer >= 1")
    if (not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() != 2
            or points.shape[1] != 3 or not points.is_contiguous()):
        raise ValueError(f"hashmod {what}: contiguous fp32 points [m, 3] expected")
    if not points.is_cuda:
        raise HashmodArgumentError(f"hashmod {what}: the tensors must be on a GPU; there is no CPU path")
    index, topology = ops._as_signed_mesh(what, mesh)
    m = int(points.shape[0])
    with torch.no_grad():
        parts = [model_or_fn(points[s:s + chunk]).reshape(-1) for s in range(0, m, chunk)]
    values = (torch.cat(parts) if parts else points.new_empty(0)).to(torch.float32).contiguous()
    if values.numel() != m:
        raise ValueError(f"hashmod {what}: the callable must return one value per point")
    return sdf_agreement(values, index.signed_distance(points, topology), band)


def _lattice_centres(lo, hi, res, device):
    """the res^3 cell centres [res^3, 3] fp32 of the box, x slowest, and the fp64 volume of a cell"""
    axes = []
    for a in range(3):
        step = (hi[a] - lo[a]) / res
        axes.append(lo[a] + (torch.arange(res, dtype=torch.float64, device=device) + 0.5) * step)
    grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    return grid.to(torch.float32).contiguous(), math.prod((hi[a] - lo[a]) / res for a in range(3))


def volume_iou(mesh_a, mesh_b, res=128, box=None, allow_open=False):
    """(iou, vol_a, vol_b, vol_both): the volumetric intersection over union of two closed meshes - each a (MeshIndex,
    MeshTopology) or a (verts, faces) pair - and the three volumes, from the occupancy of both (ops.mesh_contains) at
    the res^3 cell centres of `box` = ((x0, y0, z0), (x1, y1, z1)), by default the joint bounding box of the two
    vertex sets; a volume is a cell count times the cell volume, the iou the ratio of two counts (nan when both are
    empty).  The sign means inside only for a closed, consistently wound mesh: one that is not (MeshTopology.closed)
    raises ValueError unless allow_open is set.  Host floats; not graph-capturable."""
    what = "volume_iou"
    if not (isinstance(res, int) and not isinstance(res, bool) and 1 <= res <= 1024):
        raise ValueError(f"hashmod {what}: res must be an integer in [1, 1024]")
    if not isinstance(allow_open, bool):
        raise ValueError(f"hashmod {what}: allow_open must be a bool")
    (ia, ta), (ib, tb) = ops._as_signed_mesh(what, mesh_a), ops._as_signed_mesh(what, mesh_b)
    if ia.device != ib.device:
        raise ValueError(f"hashmod {what}: the meshes are on different devices")
    for name, t in (("mesh_a", ta), ("mesh_b", tb)):
        if not t.closed and not allow_open:
            raise ValueError(f"hashmod {what}: {name} is not closed ({t.boundary_edges} boundary, "
                             f"{t.nonmanifold_edges} non-manifold, {t.flipped_edges} flipped edges): its sign is not "
                             "an inside; pass allow_open=True to count it anyway")
    if box is None:
        ends = torch.stack([torch.minimum(ta.verts.amin(0), tb.verts.amin(0)),
                            torch.maximum(ta.verts.amax(0), tb.verts.amax(0))]).tolist()
        lo, hi = ends
    else:
        try:
            lo, hi = [float(v) for v in box[0]], [float(v) for v in box[1]]
        except (TypeError, ValueError, IndexError):
            raise ValueError(f"hashmod {what}: box must be ((x0, y0, z0), (x1, y1, z1))") from None
        if len(lo) != 3 or len(hi) != 3:
            raise ValueError(f"hashmod {what}: box must be ((x0, y0, z0), (x1, y1, z1))")
    if not all(math.isfinite(a) and math.isfinite(b) and b > a for a, b in zip(lo, hi)):
        raise ValueError(f"hashmod {what}: the box must be finite with a positive extent on every axis")
    centres, cell = _lattice_centres(lo, hi, res, ia.device)
    counts = []
    step = 1 << 21                          # queries per launch: the lattice in slabs, the counts summed on the device
    for s in range(0, centres.shape[0], step):
        q = centres[s:s + step]
        in_a, in_b = ops.mesh_contains(q, (ia, ta)), ops.mesh_contains(q, (ib, tb))
        counts.append(torch.stack([in_a.sum(), in_b.sum(), (in_a & in_b).sum(), (in_a | in_b).sum()]))
    n_a, n_b, n_both, n_any = torch.stack(counts).sum(0).tolist()
    return (n_both / n_any if n_any else math.nan), n_a * cell, n_b * cell, n_both * cell
