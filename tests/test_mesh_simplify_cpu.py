"""Properties of the numpy restatement of ops.mesh_simplify (tests/mesh_simplify_cases.py) alone, so that the GPU
tests, which compare the kernels with it, cannot pass vacuously."""
import numpy as np
import pytest

import mesh_simplify_cases as S

# a normal is compared on every cluster whose unit normals do not cancel: tests/test_mesh_simplify_gpu.py
MIN_NORMAL_RATIO = 1e-3


def _cases():
    return [(name, placement) for name in S.NAMES for placement in S.PLACEMENTS]


def test_noise_exercises_repeats_drops_and_clamps():
    ref = S.reference("noise@1.7")
    print("repeats", ref["n_repeats"], "dropped clusters", ref["n_dropped"], "clamped", int(ref["clamped"].sum()))
    assert ref["n_repeats"] >= 1 and ref["n_dropped"] >= 1 and ref["clamped"].sum() >= 1
    assert not S.reference("noise@1.7", "mean")["clamped"].any()


def test_long_run_and_empty():
    ref = S.reference("one_cell")
    assert ref["verts"].shape == (0, 3) and ref["faces"].shape == (0, 3) and np.all(ref["vertex_map"] == -1)
    assert ref["n_dropped"] == 1
    ref = S.reference("empty")
    assert ref["verts"].shape == (0, 3) and ref["faces"].shape == (0, 3) and ref["normals"].shape == (0, 3)
    assert np.all(ref["vertex_map"] == -1) and len(ref["vertex_map"]) == 5


def test_rotations_repeat_and_flips_do_not():
    # the four vertices are clusters 0, 2, 1, 3 by cell key
    ref = S.reference("rotated_repeat")
    assert ref["vertex_map"].tolist() == [0, 2, 1, 3]
    assert ref["faces"].tolist() == [[0, 2, 1], [0, 1, 3]] and ref["n_repeats"] == 1
    ref = S.reference("flipped_pair")
    assert ref["faces"].tolist() == [[0, 2, 1], [0, 1, 2], [1, 3, 2]] and ref["n_repeats"] == 0


def test_one_face_is_the_identity_up_to_order():
    m, ref = S.case("one_face"), S.reference("one_face", "mean")
    assert np.array_equal(ref["verts"][ref["vertex_map"]], m["verts"])
    want = ref["vertex_map"][m["faces"][0]]
    assert ref["faces"].tolist() == [np.roll(want, -int(np.argmin(want))).tolist()]
    assert sorted(ref["vertex_map"].tolist()) == [0, 1, 2]


def test_cell_faces_put_lattice_vertices_in_their_own_cells():
    m, ref = S.case("cell_faces"), S.reference("cell_faces", "mean")
    lattice = np.all(np.round(m["verts"] * 4) == m["verts"] * 4, 1)
    assert lattice.sum() >= 125
    # the lattice vertex at lo + i h is in cell i: two of them never share a cluster
    ids = ref["vertex_map"][lattice & (ref["vertex_map"] >= 0)]
    cells = np.round((m["verts"][lattice & (ref["vertex_map"] >= 0)] + 0.5) * 4).astype(int)
    assert len(np.unique(ids)) == len(np.unique(cells, axis=0))


def test_unused_vertices_map_to_nothing():
    m, ref = S.case("unused"), S.reference("unused")
    free = np.setdiff1d(np.arange(len(m["verts"])), m["faces"])
    assert len(free) == 100 and np.all(ref["vertex_map"][free] == -1)


@pytest.mark.parametrize("name,placement", _cases())
def test_reference_properties(name, placement):
    m, ref = S.case(name), S.reference(name, placement)
    n_out = len(ref["verts"])
    assert ref["verts"].dtype == np.float32 and ref["normals"].shape == (n_out, 3) and len(ref["members"]) == n_out
    # every compared cluster has a normal to compare
    if n_out:
        print(name, placement, "clusters", n_out, "faces", len(ref["faces"]), "smallest |sum n^| / k",
              ref["normal_ratio"].min())
        assert ref["normal_ratio"].min() >= MIN_NORMAL_RATIO
    # every member lies within the cell's diagonal (and the rounding of the coordinates) of its representative
    bound = np.sqrt(3.0) * ref["h"] + 2.0 ** -20 * (np.abs(m["verts"]).max() if len(m["verts"]) else 0.0)
    for c, members in enumerate(ref["members"]):
        assert len(members) >= 1 and np.all(np.diff(members) > 0) and np.all(ref["vertex_map"][members] == c)
        dist = np.linalg.norm(m["verts"][members].astype(np.float64) - ref["verts"][c].astype(np.float64), axis=1)
        assert dist.max() <= bound
    assert sum(len(x) for x in ref["members"]) == int((ref["vertex_map"] >= 0).sum())
    # no output face is degenerate or repeated (up to rotation), every output vertex is used, ids are in range
    f = ref["faces"]
    if len(f):
        assert f.min() == 0 and f.max() == n_out - 1 and len(np.unique(f)) == n_out
        assert np.all((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2]))
        assert np.all(f[:, 0] < f[:, 1]) and np.all(f[:, 0] < f[:, 2])
        assert len(np.unique(f, axis=0)) == len(f)
    else:
        assert n_out == 0


def test_placements_share_the_connectivity():
    for name in ("three@1.7", "noise@3.0"):
        a, b = S.reference(name, "quadric"), S.reference(name, "mean")
        assert np.array_equal(a["faces"], b["faces"]) and np.array_equal(a["vertex_map"], b["vertex_map"])
        assert np.array_equal(a["normals"], b["normals"]) and not np.array_equal(a["verts"], b["verts"])
    b, c = S.reference("three@1.7", "mean"), S.reference("three@1.7", "mean", with_normals=False)
    assert c["normals"] is None and np.array_equal(c["faces"], b["faces"]) and np.array_equal(c["verts"], b["verts"])
