"""Mesh extraction on the host: the generated marching-cubes table (scripts/gen_mc_table.py vs the checked-in
csrc/hm_mc_table.h), its face rule and loop structure on all 256 cases, the topology of the numpy reference's meshes
(tests/mc_ref.py, driven by the same table), TriMesh (utils/plots.py) and the C ABI's argument checks."""
import ctypes
import os

import numpy as np
import pytest

import mc_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gen = M.gen


def test_generated_table_equals_checked_in_header():
    assert open(gen.HEADER).read() == gen.render()


def _expected_face_segments(case):
    """undirected segments per face from the signs alone: 2 crossing edges are joined; with 4, the two edges of every
    inside corner are joined (each inside corner cut off on its own)"""
    out = {}
    for a in range(3):
        for s in (0, 1):
            corners = [c for c in range(8) if (c >> a) & 1 == s]
            edges = [e for e in range(12) if gen.EDGE_AXIS[e] != a and (gen.EDGE_CORNER[e] >> a) & 1 == s]
            ends = {e: (gen.EDGE_CORNER[e], gen.EDGE_CORNER[e] | 1 << gen.EDGE_AXIS[e]) for e in edges}
            cross = [e for e in edges if ((case >> ends[e][0]) & 1) != ((case >> ends[e][1]) & 1)]
            if len(cross) == 2:
                segs = {frozenset(cross)}
            elif len(cross) == 4:
                segs = {frozenset(e for e in edges if c in ends[e]) for c in corners if (case >> c) & 1}
            else:
                segs = set()
            out[(a, s)] = segs
    return out


def _face_of(e1, e2):
    f = set()
    for a in range(3):
        for s in (0, 1):
            if all(gen.EDGE_AXIS[e] != a and (gen.EDGE_CORNER[e] >> a) & 1 == s for e in (e1, e2)):
                f.add((a, s))
    return f


@pytest.mark.parametrize("case", range(256))
def test_case_boundary_is_the_face_rule_and_interior_edges_pair_up(case):
    tris = gen.generate()[case]
    assert len(tris) <= 5
    directed = [(t[m], t[(m + 1) % 3]) for t in tris for m in range(3)]
    assert len(set(directed)) == len(directed)          # no directed edge twice inside a cell
    und = {}
    for e in directed:
        und.setdefault(frozenset(e), []).append(e)
    boundary = {k for k, v in und.items() if len(v) == 1}
    for k, v in und.items():
        assert len(v) in (1, 2)
        if len(v) == 2:                                  # interior: once in each direction, never within a cube face
            assert v[0] == v[1][::-1]
            assert not _face_of(*k), (case, k)
    got = {}
    for k in boundary:
        faces = _face_of(*k)
        assert len(faces) == 1, (case, k)
        got.setdefault(faces.pop(), set()).add(k)
    exp = _expected_face_segments(case)
    for f, segs in exp.items():
        assert got.get(f, set()) == segs, (case, f)


def _noise(seed, shape):
    rng = np.random.default_rng(seed)
    v = np.ones(shape, np.float32)
    v[1:-1, 1:-1, 1:-1] = rng.standard_normal([s - 2 for s in shape]).astype(np.float32)
    return v


@pytest.mark.parametrize("seed", range(6))
def test_reference_noise_meshes_are_closed_and_oriented(seed):
    shape = [(24, 24, 24), (17, 33, 9), (12, 40, 15)][seed % 3]
    verts, faces, normals = M.marching_cubes(_noise(seed, shape), level=0.25 * (seed % 2))
    assert len(faces) > 1000
    assert M.edge_check(faces) == (True, True)
    assert len(np.unique(faces)) == len(verts)          # every vertex is used
    assert M.signed_volume(verts, faces) > 0


def _lattice(n):
    x = np.linspace(-1.0, 1.0, n)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    return X, Y, Z, x[1] - x[0]


def test_reference_sphere_and_torus_128():
    X, Y, Z, h = _lattice(128)
    r = 0.7
    sphere = (np.sqrt(X ** 2 + Y ** 2 + Z ** 2) - r).astype(np.float32)
    R, rr = 0.55, 0.25
    torus = (np.sqrt((np.sqrt(X ** 2 + Y ** 2) - R) ** 2 + Z ** 2) - rr).astype(np.float32)
    for vol, chi, exact in ((sphere, 2, 4.0 / 3.0 * np.pi * r ** 3), (torus, 0, 2.0 * np.pi ** 2 * R * rr ** 2)):
        verts, faces, normals = M.marching_cubes(vol, 0.0, (h, h, h))
        assert M.edge_check(faces) == (True, True)
        assert M.euler(verts, faces) == chi
        vol_mesh = M.signed_volume(verts, faces)
        assert vol_mesh > 0 and abs(vol_mesh / exact - 1.0) < 0.01
        c = verts - 1.0                                  # lattice coordinates -> centred
        radial = c if chi == 2 else c - R * np.concatenate([c[:, :2] / np.linalg.norm(c[:, :2], axis=1,
                                                                                    keepdims=True), 0 * c[:, 2:]], 1)
        cosang = np.einsum("ij,ij->i", normals, radial / np.linalg.norm(radial, axis=1, keepdims=True))
        assert cosang.min() > 0.99                       # normals point toward increasing values (outward)


def _two_boxes():
    """two unit tetrahedra far apart, the second scaled by 2 (areas differ)"""
    tv = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    tf = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64)
    verts = np.concatenate([tv, 2 * tv + 5])
    faces = np.concatenate([tf + 4, tf])     # the larger one's faces first
    return verts, faces


def test_trimesh_split_area_transform_and_ply_round_trip(tmp_path):
    from hashmodnffbanks_idr_amd.utils.plots import TriMesh
    verts, faces = _two_boxes()
    mesh = TriMesh(verts, faces)
    small = 1.5 + np.sqrt(3) / 2
    assert mesh.area == pytest.approx(5 * small)
    assert mesh.is_watertight
    parts = mesh.split(only_watertight=False)
    assert [len(p.vertices) for p in parts] == [4, 4]
    assert [p.area for p in parts] == pytest.approx([small, 4 * small])
    assert np.array_equal(parts[1].vertices, 2 * verts[:4] + 5)
    for p in parts:
        assert M.edge_check(p.faces) == (True, True) and M.signed_volume(p.vertices, p.faces) > 0
    open_part = TriMesh(verts[:4], faces[4:7] - 4)
    assert not open_part.is_watertight
    with_open = TriMesh(np.concatenate([verts, verts[:4] + 20]), np.concatenate([faces, faces[4:7] + 8]))
    assert len(with_open.split(only_watertight=False)) == 3
    assert [p.area for p in with_open.split(only_watertight=True)] == pytest.approx([small, 4 * small])

    # rotation + translation keeps the area; a reflection reverses the winding so the volume stays positive
    th = 0.3
    T = np.eye(4)
    T[:3, :3] = [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]
    T[:3, 3] = [1, 2, 3]
    m2 = TriMesh(verts, faces).apply_transform(T)
    assert m2.area == pytest.approx(mesh.area)
    assert np.allclose(m2.vertices, verts @ T[:3, :3].T + T[:3, 3])
    S = np.diag([-2.0, 1.0, 1.0, 1.0])
    m3 = TriMesh(verts, faces).apply_transform(S)
    assert M.signed_volume(m3.vertices, m3.faces) == pytest.approx(2 * M.signed_volume(verts, faces))
    assert np.allclose(np.linalg.norm(m3.vertex_normals, axis=1), 1.0)

    path = tmp_path / "m.ply"
    mesh.export(str(path))
    v, n, f = M.read_ply(str(path))
    assert np.array_equal(v, verts.astype(np.float32)) and np.array_equal(f, faces.astype(np.int32))
    assert np.array_equal(n, mesh.vertex_normals.astype(np.float32))
    assert mesh.export() == path.read_bytes()


def test_abi_rejects_bad_volumes_with_a_status():
    from hashmodnffbanks_idr_amd import build, _lib
    build.build(verbose=False)
    L = _lib.lib()
    assert L.hm_mc_workspace_bytes(1, 4, 4) == -1 and b"dimensions" in L.hm_last_error()
    assert L.hm_mc_workspace_bytes(2048, 1024, 1024) == -1
    assert 6 * 64 ** 3 <= L.hm_mc_workspace_bytes(64, 64, 64) <= 8 * 64 ** 3
    fake = ctypes.c_void_p(256)
    cnt = ctypes.c_void_p(512)
    rc = L.hm_mc_count(fake, 4, 1, 4, 4, 4, 1, 0.0, fake, 1 << 20, cnt, None)
    assert rc == -1 and b">= 2" in L.hm_last_error()
    rc = L.hm_mc_count(fake, 2048, 1024, 1024, 1 << 20, 1024, 1, 0.0, fake, 1 << 40, cnt, None)
    assert rc == -1 and b"2^31" in L.hm_last_error()
    rc = L.hm_mc_count(fake, 4, 4, 4, 16, 4, 1, 0.0, fake, 16, cnt, None)
    assert rc == -1 and b"workspace too small" in L.hm_last_error()
    sp = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    rc = L.hm_mc_emit(fake, 4, 4, 4, 16, 4, 1, 0.0, sp, fake, 1 << 20, 1 << 31, 10, fake, fake, fake, None)
    assert rc == -1 and b"int32" in L.hm_last_error()
    with pytest.raises(ValueError, match="int32"):
        _lib.check(rc)


_WS_N = [0, 1, 255, 256, 257, 4096, 4097, 1 << 20]
# the sizes the library reported before its workspace layouts were written once over HmCarve (csrc/hm_common.h): a
# buffer sized by an older build must still fit, and a part dropped from or added to a layout shows here
_WS_BYTES = {
    "hm_sort_workspace_bytes": [1024, 1792, 4096, 4096, 4864, 50176, 51968, 12845056],
    "hm_nn_workspace_bytes": [1024, 2560, 8192, 8192, 9728, 115712, 118272, 29622272],
    "hm_nn_radius_workspace_bytes": [0, 1024, 2560, 2560, 3328, 37120, 37888, 9453568],
    "hm_mesh_cc_sums_workspace_bytes": [1024, 2560, 8192, 8192, 9728, 115712, 118272, 29622272],
    "hm_mesh_moments_workspace_bytes": [256, 256, 256, 256, 256, 256, 256, 20480],
}


def test_workspace_sizes_are_the_recorded_ones():
    from hashmodnffbanks_idr_amd import build, _lib
    build.build(verbose=False)
    L = _lib.lib()
    for name, want in _WS_BYTES.items():
        assert [getattr(L, name)(n) for n in _WS_N] == want, name
    dims = [(2, 2, 2), (16, 16, 16), (17, 16, 16), (64, 64, 64)]
    assert [L.hm_mc_workspace_bytes(*d) for d in dims] == [1024, 25088, 26624, 1574656]
    assert [L.hm_mcs_workspace_bytes(n) for n in (1, 8, 9)] == [3584, 25088, 28160]
