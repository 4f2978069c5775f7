"""The numpy restatement of the signed point-to-mesh distance (tests/mesh_sign_cases.topology_ref / sign_ref, the
reference of csrc/hm_mesh_topo.hip) against generalised winding numbers, the counts and signs the cases are built to
have, and the argument checks that need no GPU."""
import functools

import numpy as np
import pytest
import torch

import mesh_dist_cases as MC
import mesh_sign_cases as SC
import nn_cases as NC

N_BOX, N_CEN, N_VERT = 5000, 2500, 2500          # 12 500 queries per mesh


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name in ("icosphere1", "icosphere2"):
        return NC.icosphere(int(name[-1]))
    return SC.displaced_icosphere(3) if name == "displaced3" else SC.mc_sphere()


# ---- the rule against winding numbers -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mc_sphere", "icosphere1", "icosphere2", "displaced3"])
def test_sign_rule_equals_winding_number(name):
    """on EVERY query farther than 1e-6 x the largest extent from the surface the sign of the rule, evaluated on the
    fp32 closest point of closest_ref, is the inside / outside of the fp64 winding number"""
    v, f = _mesh(name)
    rng = np.random.default_rng(sum(map(ord, name)) + 5)
    q = SC.query_mix(v, f, rng, N_BOX, N_CEN, N_VERT)
    assert len(q) == 12500
    closest = MC.closest_ref(q, v, f)
    VN, EN, counts = SC.topology_ref(v, f)
    assert counts == (0, 0, 0)
    sd, sign, branch = SC.sign_ref(q, v, f, closest, VN, EN, return_branch=True)
    w = SC.winding_ref(q, v, f)
    far = np.sqrt(closest[0].astype(np.float64)) > 1e-6 * SC.extent(v)
    share = np.bincount(branch, minlength=3) / len(q)
    print(f"{name}: {far.sum()} of {len(q)} queries beyond 1e-6 extent; face / edge / vertex branch "
          f"{share[0]:.3f} / {share[1]:.3f} / {share[2]:.3f}; inside {(sign < 0).mean():.3f}")
    bad = np.nonzero(far & ((sign < 0) != (w > 0.5)))[0]
    assert len(bad) == 0, [(q[i].tolist(), int(branch[i]), float(w[i]), float(sd[i])) for i in bad[:10]]
    assert far.sum() > 12000 and np.abs(w[far] - np.round(w[far])).max() < 1e-3
    assert share.min() > 0.01                                         # all three branches are exercised
    assert 0.05 < (sign < 0).mean() < 0.95
    assert np.array_equal(np.abs(sd), np.sqrt(closest[0]))


# ---- topology counts ----------------------------------------------------------------------------------------
def test_topology_counts():
    for name in ("icosphere1", "icosphere2", "displaced3", "mc_sphere"):
        assert SC.topology(name)[2] == (0, 0, 0), name
    assert SC.topology("planar")[2] == (20, 0, 0)
    for n in MC.SOUP_F:
        assert SC.topology(f"soup_{n}")[2] == (3 * n, 0, 0)
    assert SC.topology("three_on_edge")[2] == (6, 1, 0)
    assert SC.topology("flipped1")[2] == (0, 0, 3)
    for n in SC.FANS:
        assert SC.topology(f"fan_{n}")[2] == (n, 0, 0)


def test_tables_of_simple_meshes():
    # planar: every face's unit normal is +z, so an inner edge sums two of them, a rim edge has its own, and an inner
    # vertex sums its six corner angles, 2 pi
    v, f, _ = SC.case("planar")
    VN, EN, _ = SC.topology("planar")
    assert np.array_equal(EN[..., :2], np.zeros((50, 3, 2))) and set(np.unique(EN[..., 2])) == {1.0, 2.0}
    assert (EN[..., 2] == 1.0).sum() == 20
    inner = 2 * 6 + 3
    assert VN[inner, 2] == pytest.approx(2 * np.pi, rel=1e-14) and VN[0, 2] == pytest.approx(np.pi / 2, rel=1e-14)
    # the book of three pages: every half-edge of the shared edge stores the sum of all three normals
    _, EN3, _ = SC.topology("three_on_edge")
    _, nu, _ = SC.face_quantities(*SC.case("three_on_edge")[:2])
    want = (nu[0] + nu[1]) + nu[2]
    assert all(np.array_equal(EN3[face, 0], want) for face in range(3))
    assert np.array_equal(EN3[0, 1], nu[0])
    # a face with a repeated vertex has nu = 0 and still takes part in the runs; an unreferenced vertex stays zero
    vo, fo, _ = SC.case("odd_faces")
    VNo, ENo, counts = SC.topology("odd_faces")
    _, nuo, _ = SC.face_quantities(vo, fo)
    assert np.array_equal(nuo[0], np.zeros(3)) and np.array_equal(nuo[1], np.zeros(3))
    assert counts == (12, 1, 0)                 # (9,10) is in face 1 (twice) and in face 4; (9,9) is a run of its own
    assert np.array_equal(ENo[4, 0], nuo[4]) and np.array_equal(ENo[1, 1], nuo[4])
    assert np.isfinite(VNo).all() and np.isfinite(ENo).all()


# ---- planar signs -------------------------------------------------------------------------------------------
def test_planar_signs():
    v, f, q = SC.case("planar")
    VN, EN, _ = SC.topology("planar")
    closest = SC.reference("planar")
    sd, sign = SC.sign_ref(q, v, f, closest, VN, EN)
    assert sign.tolist() == list(SC.PLANAR_SIGNS)
    want = np.asarray([d for _, d, _ in MC.PLANAR_QUERIES], np.float32)
    assert np.array_equal(sd, np.asarray(SC.PLANAR_SIGNS, np.float32) * np.sqrt(want))
    # mirrored queries: below is -, except where s == 0 (in the plane, on a vertex)
    qm = q * np.asarray([1, 1, -1], np.float32)
    sign_m = SC.sign_ref(qm, v, f, MC.closest_ref(qm, v, f), VN, EN)[1]
    assert sign_m.tolist() == [-s if p[2] != 0 else 1 for s, (p, _, _) in zip(SC.PLANAR_SIGNS, MC.PLANAR_QUERIES)]


def test_cut_queries_have_no_sign():
    v, f, q = SC.case("clusters")
    md2 = float(np.float32(MC.CLUSTERS_MAX_DIST) ** 2)
    closest = SC.reference("clusters", md2)
    VN, EN, _ = SC.topology("clusters")
    sd, sign = SC.sign_ref(q, v, f, closest, VN, EN)
    cut = closest[1] < 0
    assert 0 < cut.sum() < len(q)
    assert np.isposinf(sd[cut]).all() and (sign[cut] == 0).all() and (np.abs(sign[~cut]) == 1).all()


# ---- argument checks ----------------------------------------------------------------------------------------
def test_argument_checks():
    """ValueError before the library is touched: there is no GPU here, and no call below reaches one"""
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd._lib import HashmodError
    from hashmodnffbanks_idr_amd.evaluation import mesh_sdf_agreement, sdf_agreement, volume_iou
    v, f, q = (torch.from_numpy(np.array(a)) for a in MC.case("single"))
    meta = dict(device="meta")
    vm, fm, qm = torch.zeros(3, 3, **meta), torch.zeros(1, 3, dtype=torch.int32, **meta), torch.zeros(5, 3, **meta)
    for bad in (v.double(), torch.zeros(3, 4), torch.zeros(3, 8).t(), torch.zeros(8), None):
        with pytest.raises(ValueError):
            ops.mesh_topology(bad, f)
        with pytest.raises(ValueError):
            ops.mesh_signed_distance(bad, v, f)
        with pytest.raises(ValueError):
            ops.mesh_signed_distance(q, bad, f)
        with pytest.raises(ValueError):
            ops.mesh_contains(bad, (v, f))
    for bad in (f.long(), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32).t(), None):
        with pytest.raises(ValueError):
            ops.mesh_topology(v, bad)
        with pytest.raises(ValueError):
            ops.mesh_signed_distance(q, v, bad)
    # a CPU tensor of the right dtype and shape: an argument error and a HashmodError
    for call in (lambda: ops.mesh_topology(v, f), lambda: ops.mesh_signed_distance(q, v, f),
                 lambda: ops.mesh_contains(q, (v, f)), lambda: volume_iou((v, f), (v, f)),
                 lambda: sdf_agreement(torch.zeros(4), torch.zeros(4)),
                 lambda: mesh_sdf_agreement(lambda x: x[:, 0], (v, f), q)):
        with pytest.raises(ValueError, match="GPU"):
            call()
        with pytest.raises(HashmodError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="at least one face"):
        ops.mesh_topology(vm, torch.zeros(0, 3, dtype=torch.int32, **meta))
    for md in (-1.0, float("nan"), "1"):
        with pytest.raises(ValueError, match="max_dist"):
            ops.mesh_signed_distance(qm, vm, fm, max_dist=md)
    for flag in (1, None, "yes"):
        for name in ("return_sign", "return_face", "return_point"):
            with pytest.raises(ValueError, match=name):
                ops.mesh_signed_distance(qm, vm, fm, **{name: flag})
    for cell in (0, -1.0, float("nan"), "1", True):
        with pytest.raises(ValueError, match="cell"):
            ops.mesh_signed_distance(qm, vm, fm, cell=cell)
    for mesh in ("mesh.ply", (vm,), (vm, fm, qm), None):
        with pytest.raises(ValueError, match="mesh"):
            ops.mesh_contains(qm, mesh)
        with pytest.raises(ValueError, match="mesh"):
            volume_iou(mesh, (vm, fm))
    for res in (0, -3, 2.5, "8", True, 4096):
        with pytest.raises(ValueError, match="res"):
            volume_iou((vm, fm), (vm, fm), res=res)
    with pytest.raises(ValueError, match="allow_open"):
        volume_iou((vm, fm), (vm, fm), allow_open=1)
    for a, b in ((torch.zeros(4), torch.zeros(5)), (torch.zeros(4, 1), torch.zeros(4, 1)),
                 (torch.zeros(4).double(), torch.zeros(4)), (torch.zeros(4), None)):
        with pytest.raises(ValueError):
            sdf_agreement(a, b)
    for band in (0, -1.0, float("nan"), "1", True):
        with pytest.raises(ValueError, match="band"):
            sdf_agreement(torch.zeros(4, **meta), torch.zeros(4, **meta), band=band)
    with pytest.raises(ValueError, match="callable"):
        mesh_sdf_agreement(None, (vm, fm), qm)
    for chunk in (0, 1.5, True):
        with pytest.raises(ValueError, match="chunk"):
            mesh_sdf_agreement(lambda x: x[:, 0], (vm, fm), qm, chunk=chunk)
