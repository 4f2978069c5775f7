"""The device signed point-to-mesh distance (csrc/hm_mesh_topo.hip) against its numpy restatement
(tests/mesh_sign_cases.topology_ref / sign_ref): the edge table and the counts bit for bit, the vertex table up to the
device's atan2, the sign and the signed distance bit for bit from the device's own tables over every grid and big-face
setting, analytic signs on a sphere, independence of batching, order and face numbering, the errors, and the
evaluation entry points built on it."""
import functools
import math

import numpy as np
import pytest
import torch

import mc_ref
import mesh_dist_cases as MC
import mesh_sign_cases as SC
import nn_cases as NC
from hashmodnffbanks_idr_amd import ops
from hashmodnffbanks_idr_amd._lib import HashmodError
from hashmodnffbanks_idr_amd.evaluation import mesh_sdf, mesh_sdf_agreement, sdf_agreement, volume_iou

pytestmark = pytest.mark.gpu

CELL_IDS = ["default", "one_cell", "fine"]


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # a copy: the shared inputs are read-only


def _big(big_face):
    return ops.MESH_DIST_BIG_FACE if big_face is None else big_face


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """(verts, faces, topology) of the case on the device, and the topology's tables on the host"""
    v, f, _ = SC.case(name)
    vd, fd = _dev(v), _dev(f)
    topo = ops.mesh_topology(vd, fd)
    return vd, fd, topo, topo.vertex_normals.cpu().numpy(), topo.edge_normals.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _want(name, max_dist2=np.inf):
    """sign_ref of the case's brute-force closest points with the DEVICE's tables: (sd, sign)"""
    v, f, q = SC.case(name)
    _, _, _, VN, EN = _mesh(name)
    return SC.sign_ref(q, v, f, SC.reference(name, max_dist2), VN, EN)


def _check(got, want, what=""):
    sd, sign = got
    assert sd.dtype == torch.float32 and sign.dtype == torch.int32
    assert torch.equal(sign.cpu(), torch.from_numpy(want[1].copy())), f"sign differs from the rule {what}"
    assert torch.equal(sd.cpu(), torch.from_numpy(want[0].copy())), f"sd differs from the rule {what}"


# ---- the tables ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.CASES)
def test_tables_and_counts(name):
    v, f, _ = SC.case(name)
    _, _, topo, VN, EN = _mesh(name)
    VN_ref, EN_ref, counts = SC.topology(name)
    assert topo.vertex_normals.dtype == torch.float64 and topo.vertex_normals.shape == (len(v), 3)
    assert topo.edge_normals.dtype == torch.float64 and topo.edge_normals.shape == (len(f), 3, 3)
    assert (topo.boundary_edges, topo.nonmanifold_edges, topo.flipped_edges) == counts
    assert topo.closed == (counts == (0, 0, 0)) and topo.closed == (name in SC.CLOSED)
    assert torch.equal(torch.from_numpy(EN), torch.from_numpy(EN_ref.copy())), "edge_normals differ"
    # the vertex table within 1e-12 of the vector's norm: device atan2 is not numpy's; four orders above the fp64
    # rounding of a dozen terms, eight below anything that moves a sign here
    norm = np.sqrt((VN_ref * VN_ref).sum(1))
    err = np.sqrt(((VN - VN_ref) ** 2).sum(1))
    rel = err[norm > 0] / norm[norm > 0]
    print(f"{name}: max |VN - VN_ref| / |VN_ref| = {rel.max() if len(rel) else 0.0:.3e}")
    assert (err <= 1e-12 * norm).all()
    again = ops.mesh_topology(*_mesh(name)[:2])
    assert torch.equal(again.vertex_normals, topo.vertex_normals) and torch.equal(again.edge_normals, topo.edge_normals)


def test_unreferenced_vertices_are_zero():
    v, f, _ = SC.case("icosphere1")
    extra = np.concatenate([np.full((3, 3), 7.0, np.float32), v, np.full((5, 3), -2.0, np.float32)])
    topo = ops.mesh_topology(_dev(extra), _dev(f + 3))
    assert torch.equal(topo.vertex_normals[3:-5], _mesh("icosphere1")[2].vertex_normals)
    assert not topo.vertex_normals[:3].any() and not topo.vertex_normals[-5:].any()
    assert torch.equal(topo.edge_normals, _mesh("icosphere1")[2].edge_normals) and topo.closed


# ---- sign and signed distance, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("which", range(3), ids=CELL_IDS)
@pytest.mark.parametrize("name", SC.CASES)
def test_signed_distance_equals_the_rule(name, which):
    v, f, q = SC.case(name)
    vd, fd, topo, _, _ = _mesh(name)
    qd = _dev(q)
    cell = MC.cells(v)[which]
    want = _want(name)
    for big_face in MC.BIG_FACES:
        index = ops.mesh_index(vd, fd, cell=cell, big_face=_big(big_face))
        _check(index.signed_distance(qd, topo, return_sign=True), want, f"(cell {cell}, big_face {big_face})")
    if which == 0:
        padded = ops.mesh_index(vd, fd, pad=ops.mesh_ray_pad(vd))
        _check(padded.signed_distance(qd, topo, return_sign=True), want, "(padded index)")
        assert torch.equal(ops.mesh_contains(qd, (padded, topo)).cpu(), torch.from_numpy(want[1] < 0))
        assert torch.equal(ops.mesh_contains(qd, (vd, fd)).cpu(), torch.from_numpy(want[1] < 0))
        _check(ops.mesh_signed_distance(qd, vd, fd, return_sign=True), want, "(one call)")


def test_magnitude_is_the_closest_point_distance_and_outputs_are_optional():
    v, f, q = SC.case("displaced3")
    vd, fd, topo, _, _ = _mesh("displaced3")
    qd = _dev(q)
    index = ops.mesh_index(vd, fd)
    d2, face, point = ops.mesh_closest_point(qd, vd, fd)
    sd = index.signed_distance(qd, topo)
    assert isinstance(sd, torch.Tensor) and torch.equal(sd.abs(), torch.sqrt(d2))
    sd2, sign, face2, point2 = index.signed_distance(qd, topo, return_sign=True, return_face=True, return_point=True)
    assert torch.equal(sd2, sd) and torch.equal(face2, face) and torch.equal(point2, point)
    assert torch.equal(sign, torch.where(sd < 0, -1, 1).to(torch.int32))
    sd3, point3 = ops.mesh_signed_distance(qd, vd, fd, return_point=True)
    assert torch.equal(sd3, sd) and torch.equal(point3, point)
    assert 0.1 < (sign < 0).float().mean().item() < 0.9


def test_cut_queries_get_inf_and_sign_zero():
    v, f, q = SC.case("clusters")
    vd, fd, topo, _, _ = _mesh("clusters")
    md2 = float(np.float32(MC.CLUSTERS_MAX_DIST) ** 2)
    want = _want("clusters", md2)
    cut = want[1] == 0
    assert 0 < cut.sum() < len(q) and np.isposinf(want[0][cut]).all()
    for which in range(3):
        index = ops.mesh_index(vd, fd, cell=MC.cells(v)[which])
        got = index.signed_distance(_dev(q), topo, max_dist=MC.CLUSTERS_MAX_DIST, return_sign=True)
        _check(got, want, f"(cell {which})")
    _check(ops.mesh_signed_distance(_dev(q), vd, fd, max_dist=MC.CLUSTERS_MAX_DIST, return_sign=True), want)


def test_empty_queries_give_empty_outputs():
    vd, fd, topo, _, _ = _mesh("icosphere1")
    index = ops.mesh_index(vd, fd)
    empty = torch.zeros((0, 3), device="cuda")
    sd, sign, face, point = index.signed_distance(empty, topo, return_sign=True, return_face=True, return_point=True)
    assert sd.shape == (0,) and sign.shape == (0,) and face.shape == (0,) and point.shape == (0, 3)
    assert sd.dtype == torch.float32 and sign.dtype == torch.int32
    assert ops.mesh_signed_distance(empty, vd, fd).shape == (0,)
    inside = ops.mesh_contains(empty, (vd, fd))
    assert inside.shape == (0,) and inside.dtype == torch.bool


# ---- analytic signs -----------------------------------------------------------------------------------------
def test_analytic_signs_on_a_sphere():
    v, f = NC.icosphere(5)
    rng = np.random.default_rng(41)
    q = NC._f4(np.concatenate([(rng.random((100000, 3)) * 2 - 1) * 1.3, NC.sphere_clouds()[0][:100000]]))
    assert len(f) == 20480 and len(q) == 200000
    tri = v.astype(np.float64)[f]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    inner_radius = ((n / np.linalg.norm(n, axis=1, keepdims=True)) * tri[:, 0]).sum(1).min()
    assert 0.99 < inner_radius < 1.0
    vd, fd = _dev(v), _dev(f)
    topo = ops.mesh_topology(vd, fd)
    assert topo.closed
    sd, sign = ops.mesh_index(vd, fd).signed_distance(_dev(q), topo, return_sign=True)
    sign = sign.cpu().numpy()
    r = np.sqrt((q.astype(np.float64) ** 2).sum(1))
    inside, outside = r < inner_radius, r > 1.0
    print(f"inner radius {inner_radius:.6f}: {inside.sum()} queries inside it, {outside.sum()} beyond 1")
    assert inside.sum() > 50000 and outside.sum() > 50000
    assert (sign[inside] == -1).all() and (sign[outside] == 1).all()
    # the distance to a convex inscribed polyhedron from outside is at least |q| - 1
    got = sd.cpu().numpy().astype(np.float64)
    assert (got[outside] >= (r[outside] - 1.0) - 1e-6).all() and (-got[inside] <= 1.0 - r[inside] + 1e-6).all()


# ---- independence -------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_batching_or_order():
    v, f, q = SC.case("queries_1000")
    vd, fd, topo, _, _ = _mesh("queries_1000")
    index = ops.mesh_index(vd, fd)
    qd = _dev(q)
    first = index.signed_distance(qd, topo, return_sign=True)
    _check(first, _want("queries_1000"))
    again = index.signed_distance(qd, topo, return_sign=True)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for k in (1, 63, 65, 257):
        part = index.signed_distance(qd[:k].contiguous(), topo, return_sign=True)
        assert all(torch.equal(a, b[:k]) for a, b in zip(part, first)), k
    perm = torch.from_numpy(np.random.default_rng(8).permutation(len(q))).cuda()
    shuffled = index.signed_distance(qd[perm].contiguous(), topo, return_sign=True)
    assert all(torch.equal(a, b[perm]) for a, b in zip(shuffled, first))


@pytest.mark.parametrize("name", ["icosphere2", "displaced3", "mc_sphere", "planar", "fan_300"])
def test_permuting_the_faces_keeps_magnitude_and_far_signs(name):
    v, f, q = SC.case(name)
    want_sd, want_sign = _want(name)
    perm = np.random.default_rng(12).permutation(len(f))
    sd, sign = ops.mesh_signed_distance(_dev(q), _dev(v), _dev(f[perm]), return_sign=True)
    sd, sign = sd.cpu().numpy(), sign.cpu().numpy()
    assert np.array_equal(np.abs(sd), np.abs(want_sd))
    if name in SC.CLOSED:
        far = np.abs(want_sd) > 1e-6 * SC.extent(v)
        assert far.sum() > len(q) // 2 and np.array_equal(sign[far], want_sign[far])
    # and bit for bit the rule on the permuted mesh, with the permuted mesh's own tables
    topo = ops.mesh_topology(_dev(v), _dev(f[perm]))
    rule = SC.sign_ref(q, v, f[perm], MC.closest_ref(q, v, f[perm]), topo.vertex_normals.cpu().numpy(),
                       topo.edge_normals.cpu().numpy())
    assert np.array_equal(sd, rule[0]) and np.array_equal(sign, rule[1])


# ---- errors -------------------------------------------------------------------------------------------------
def test_bad_inputs_raise_and_leave_the_library_usable():
    v, f, q = SC.case("icosphere1")
    vd, fd, topo, _, _ = _mesh("icosphere1")
    index = ops.mesh_index(vd, fd)
    other = _mesh("icosphere2")
    with pytest.raises(ValueError, match="topology"):
        index.signed_distance(_dev(q), other[2])
    with pytest.raises(ValueError, match="topology"):
        index.signed_distance(_dev(q), (vd, fd))
    with pytest.raises(ValueError, match="topology"):
        ops.mesh_contains(_dev(q), (ops.mesh_index(other[0], other[1]), topo))
    for bad in (np.nan, np.inf):
        vb = np.array(v)
        vb[int(f[7, 1]), 2] = bad
        with pytest.raises(HashmodError, match="non-finite"):
            ops.mesh_topology(_dev(vb), fd)
    for bad in (-1, len(v)):
        fb = np.array(f)
        fb[11, 2] = bad
        with pytest.raises(HashmodError, match="face index"):
            ops.mesh_topology(vd, _dev(fb))
    qb = np.array(q)
    qb[5, 1] = np.nan
    with pytest.raises(HashmodError, match="non-finite"):
        index.signed_distance(_dev(qb), topo)
    with pytest.raises(ValueError, match="GPU|devices"):
        index.signed_distance(torch.from_numpy(np.array(q)), topo)
    with pytest.raises(ValueError, match="GPU"):
        ops.mesh_topology(torch.from_numpy(np.array(v)), fd.cpu())
    with pytest.raises(ValueError, match="GPU"):
        sdf_agreement(torch.zeros(4), torch.zeros(4))
    vp, fp = _mesh("planar")[:2]
    with pytest.raises(ValueError, match="not closed"):
        volume_iou((vd, fd), (vp, fp))
    with pytest.raises(ValueError, match="not closed"):
        volume_iou((vp, fp), (vd, fd), res=4)
    vf, ff = _mesh("flipped1")[:2]
    with pytest.raises(ValueError, match="3 flipped"):
        volume_iou((vf, ff), (vd, fd), res=4)
    with pytest.raises(ValueError, match="box"):
        volume_iou((vd, fd), (vd, fd), res=4, box=((0, 0, 0), (1, 1, 0)))
    iou, va, vb_, vboth = volume_iou((vd, fd), (vp, fp), res=8, allow_open=True)
    assert va > 0 and vboth <= va
    _check(index.signed_distance(_dev(q), topo, return_sign=True), _want("icosphere1"))


# ---- evaluation ---------------------------------------------------------------------------------------------
def test_volume_iou_of_a_mesh_with_itself_is_one():
    v, f = NC.icosphere(3)
    vd, fd = _dev(v), _dev(f)
    iou, vol_a, vol_b, vol_both = volume_iou((vd, fd), (vd, fd), res=32)
    assert iou == 1.0 and vol_a == vol_b == vol_both
    # the volume of the inscribed polyhedron, to the lattice's resolution
    assert vol_a == pytest.approx(abs(mc_ref.signed_volume(v, f)), rel=0.02)
    pair = (ops.mesh_index(vd, fd, cell=0.5), ops.mesh_topology(vd, fd))
    assert volume_iou(pair, (vd, fd), res=32) == (iou, vol_a, vol_b, vol_both)


def test_volume_iou_against_winding_number_occupancy():
    v, f = NC.icosphere(3)
    half = NC._f4(v * np.float32(0.5))
    res = 48
    vd, fd, hd = _dev(v), _dev(f), _dev(half)
    iou, vol_a, vol_b, vol_both = volume_iou((vd, fd), (hd, fd), res=res)
    lo, hi = v.min(0).astype(np.float64).tolist(), v.max(0).astype(np.float64).tolist()
    centres, cell = mesh_sdf._lattice_centres(lo, hi, res, vd.device)
    assert centres.shape == (res ** 3, 3) and centres.dtype == torch.float32
    c = centres.cpu().numpy()
    # the reference occupancy: winding numbers, for the half-size copy only where its bounding box reaches
    in_a = SC.winding_ref(c, v, f) > 0.5
    in_b = np.zeros(len(c), bool)
    near_b = (np.abs(c) <= np.abs(half).max(0) * 1.01).all(1)
    in_b[near_b] = SC.winding_ref(c[near_b], half, f) > 0.5
    sd_a = ops.mesh_signed_distance(centres, vd, fd).cpu().numpy()
    sd_b = ops.mesh_signed_distance(centres, hd, fd).cpu().numpy()
    tol = 1e-6 * SC.extent(v)
    far = (np.abs(sd_a) > tol) & (np.abs(sd_b) > tol)
    got_a = ops.mesh_contains(centres, (vd, fd)).cpu().numpy()
    got_b = ops.mesh_contains(centres, (hd, fd)).cpu().numpy()
    assert np.array_equal(got_a[far], in_a[far]) and np.array_equal(got_b[far], in_b[far])
    n_near = int((~far).sum())
    print(f"{n_near} of {res ** 3} cell centres within 1e-6 extent of a surface; cells inside a / b / both "
          f"{in_a.sum()} / {in_b.sum()} / {(in_a & in_b).sum()}")
    # the counts volume_iou reports are those of mesh_contains, and the reference's up to the near cells
    assert vol_a == got_a.sum() * cell and vol_b == got_b.sum() * cell and vol_both == (got_a & got_b).sum() * cell
    assert iou == (got_a & got_b).sum() / (got_a | got_b).sum()
    assert abs(int(got_a.sum()) - int(in_a.sum())) <= n_near
    assert abs(int((got_a & got_b).sum()) - int((in_a & in_b).sum())) <= n_near
    if n_near == 0:                                                   # equal counts: the ratio up to its two roundings
        assert vol_both / vol_a == pytest.approx((in_a & in_b).sum() / in_a.sum(), rel=2.0 ** -50, abs=0)
    assert vol_both == vol_b and vol_both / vol_a == pytest.approx(0.125, rel=0.05)


def test_sdf_agreement_against_numpy():
    rng = np.random.default_rng(3)
    sd = (rng.standard_normal(1001) * 0.3).astype(np.float32)
    values = (sd + rng.standard_normal(1001) * 0.05).astype(np.float32)
    sd[::50] = np.inf                                                 # cut queries
    values[7], sd[9] = 0.0, 0.0                                       # zero counts as positive
    for band in (None, 0.2):
        got = sdf_agreement(_dev(values), _dev(sd), band)
        used = np.isfinite(sd) & (True if band is None else np.abs(sd.astype(np.float64)) <= band)
        diff = np.abs(values.astype(np.float64) - sd.astype(np.float64))[used]
        same = ((values >= 0) == (sd >= 0))[used]
        assert got.n == 1001 and got.n_used == int(used.sum()) and got.sign_agreement == same.sum() / used.sum()
        assert 0.5 < got.sign_agreement < 1.0
        assert got.mean == pytest.approx(diff.mean(), rel=1e-12, abs=0)
        assert got.median == np.sort(diff)[(len(diff) - 1) // 2] and got.max == diff.max()
    none = sdf_agreement(_dev(values), torch.full((1001,), math.inf, device="cuda"))
    assert none.n == 1001 and none.n_used == 0 and all(math.isnan(x) for x in none[2:])


def test_mesh_sdf_agreement_of_the_analytic_sphere():
    v, f = NC.icosphere(3)
    vd, fd = _dev(v), _dev(f)
    q = _dev(NC._f4((np.random.default_rng(17).random((5000, 3)) * 2 - 1) * 1.2))

    def sphere(x):
        assert not torch.is_grad_enabled() and x.shape[0] <= 1024
        return x.norm(dim=1, keepdim=True) - 1.0

    got = mesh_sdf_agreement(sphere, (vd, fd), q, chunk=1024)
    sd = ops.mesh_signed_distance(q, vd, fd)
    with torch.no_grad():
        values = torch.cat([sphere(q[s:s + 1024]).reshape(-1) for s in range(0, 5000, 1024)])
    assert got == sdf_agreement(values, sd)
    # the polyhedron is inscribed: it lies within the sagitta of its longest edge of the sphere
    assert got.n == got.n_used == 5000 and got.sign_agreement > 0.98 and 0.0 < got.max < 0.02
    banded = mesh_sdf_agreement(sphere, (ops.mesh_index(vd, fd), ops.mesh_topology(vd, fd)), q, band=0.1, chunk=1024)
    assert 0 < banded.n_used < 5000 and banded.max <= got.max
