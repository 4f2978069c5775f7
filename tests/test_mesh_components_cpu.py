"""The inputs of the mesh-component tests have the properties the GPU tests rely on, and the numpy restatement they
use as reference is TriMesh.split (runs anywhere)."""
import inspect

import numpy as np
import pytest

import mesh_cc_cases as CC
from hashmodnffbanks_idr_amd.utils.plots import TriMesh, get_surface_high_res_mesh

WITH_FACES = [n for n in CC.NAMES if n not in ("empty", "lone_vertex")]


def test_case_properties():
    ref = CC.reference("three")
    assert len(ref["ids"]) == 3
    assert np.allclose(np.sort(ref["area"])[::-1], [2.003, 1.411, 0.495], atol=1e-3)

    m, ref = CC.case("noise"), CC.reference("noise")
    top = np.sort(ref["area"])[::-1]
    assert len(m["faces"]) == 178788 and len(ref["ids"]) == 562 and top[0] > 1300 * top[1]

    m, ref = CC.case("noise_many"), CC.reference("noise_many")
    top = np.sort(ref["area"])[::-1]
    assert len(m["faces"]) == 33148 and len(ref["ids"]) == 1776
    assert np.allclose(top[:2], [41.79, 38.58], atol=5e-3)

    m, ref = CC.case("strip"), CC.reference("strip")
    assert len(m["faces"]) == 100000 and len(ref["ids"]) == 1 and np.all(ref["label"] == 0)
    assert not np.array_equal(np.sort(m["faces"][:, 0]), m["faces"][:, 0])            # shuffled
    for nv in CC.BLOCK_EDGES:
        m, ref = CC.case(f"strip_{nv}"), CC.reference(f"strip_{nv}")
        assert len(m["verts"]) == nv and len(m["faces"]) == nv - 2 and len(ref["ids"]) == 1

    assert len(CC.case("empty")["faces"]) == 0 and len(CC.case("one_face")["faces"]) == 1
    assert CC.case("lone_vertex")["verts"].shape == (1, 3) and len(CC.case("lone_vertex")["faces"]) == 0
    assert np.array_equal(CC.reference("lone_vertex")["label"], [0])

    m, ref, base = CC.case("unused"), CC.reference("unused"), CC.case("three")
    free = np.setdiff1d(np.arange(len(m["verts"])), m["faces"])
    assert len(free) == 100 and len(m["verts"]) == len(base["verts"]) + 100
    assert free.min() < m["faces"].max() and np.array_equal(ref["label"][free], free)
    assert np.array_equal(ref["area"], CC.reference("three")["area"])

    m, ref = CC.case("repeated"), CC.reference("repeated")
    assert any(len(set(f)) == 2 for f in m["faces"].tolist())
    assert ref["ids"].tolist() == [0, 3] and ref["count"].tolist() == [1, 2] and ref["label"][7] == 7

    ref = CC.reference(CC.TIE)
    assert len(ref["ids"]) == 2 and ref["area"][0] == ref["area"][1] and ref["count"][0] == ref["count"][1]


@pytest.mark.parametrize("name", [n for n in WITH_FACES if n != CC.TIE])
def test_argmax_does_not_hinge_on_rounding(name):
    area = np.sort(CC.reference(name)["area"])[::-1]
    assert len(area) == 1 or area[0] - area[1] > 1e-6 * area[0]


@pytest.mark.parametrize("name", WITH_FACES)
def test_restatement_is_trimesh_split(name):
    m, ref = CC.case(name), CC.reference(name)
    mesh = TriMesh(m["verts"], m["faces"], m["normals"])
    parts = mesh.split(only_watertight=False)
    assert len(parts) == len(ref["ids"])
    for part, cid, area, count in zip(parts, ref["ids"], ref["area"], ref["count"]):
        v, f, n = CC.submesh(m["verts"], m["faces"], m["normals"], ref["label"], cid)
        assert np.array_equal(part.vertices, v.astype(np.float64)) and np.array_equal(part.faces, f)
        assert np.array_equal(part.vertex_normals, n.astype(np.float64))
        assert part.vertices.shape[0] > 0 and ref["label"][cid] == cid
        # two summation orders of at most 2e5 positive fp64 terms: 2e5 * 2^-53 ~ 2e-11 at worst
        assert len(part.faces) == count and part.area == pytest.approx(area, rel=1e-10)
    best = parts[int(np.argmax([p.area for p in parts]))]
    v, f, n = CC.largest(name)
    assert np.array_equal(best.vertices, v.astype(np.float64)) and np.array_equal(best.faces, f)


def test_empty_meshes_split_into_nothing():
    for name in ("empty", "lone_vertex"):
        m = CC.case(name)
        assert TriMesh(m["verts"], m["faces"], m["normals"]).split() == []
        assert len(CC.reference(name)["ids"]) == 0
        assert np.array_equal(CC.reference(name)["label"], np.arange(len(m["verts"])))


def test_high_res_mesh_takes_largest_component_flag():
    p = inspect.signature(get_surface_high_res_mesh).parameters
    assert p["largest_component"].default is False and p["sparse"].default is False
    assert list(p)[:4] == ["sdf", "resolution", "device", "sparse"]
