"""Shared inputs of the mesh-component tests (numpy only): meshes from tests/mc_ref.marching_cubes or built by hand,
and the numpy restatement of TriMesh.split that serves as the reference of the HIP kernels (csrc/hm_mesh_cc.hip) -
label = smallest vertex id of the component (scipy connected_components), submesh through np.unique.

case(name) -> {"verts" [V,3] f4, "faces" [F,3] i8, "normals" [V,3] f4}; reference(name) -> labels, the ids of the
components that own faces (ascending), their fp64 areas and face counts.  Both are computed once and read-only."""
import functools

import numpy as np

import mc_ref as M

BLOCK_EDGES = (4095, 4096, 4097)
NAMES = ("three", "noise", "noise_many", "strip") + tuple(f"strip_{v}" for v in BLOCK_EDGES) + (
    "empty", "one_face", "lone_vertex", "unused", "repeated", "tie")
TIE = "tie"


def _frozen(**arrays):
    for a in arrays.values():
        a.setflags(write=False)
    return arrays


def _mesh(verts, faces, normals):
    return _frozen(verts=np.ascontiguousarray(verts, np.float32), faces=np.ascontiguousarray(faces, np.int64).reshape(-1, 3),
                   normals=np.ascontiguousarray(normals, np.float32))


def _from_volume(vol, spacing, level):
    v, f, n = M.marching_cubes(vol, level, spacing)
    return _mesh(v, f, n)


def _three():
    shape = (48, 40, 56)
    axes = [np.linspace(-1.0, 1.0, n) for n in shape]
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    s1 = np.sqrt((X + 0.45) ** 2 + (Y - 0.1) ** 2 + Z ** 2) - 0.4
    s2 = np.sqrt((X - 0.6) ** 2 + (Y + 0.5) ** 2 + (Z - 0.5) ** 2) - 0.2
    ring = np.sqrt((X - 0.45) ** 2 + (Y - 0.35) ** 2) - 0.3
    torus = np.sqrt(ring ** 2 + (Z + 0.55) ** 2) - 0.12
    vol = np.minimum(np.minimum(s1, s2), torus).astype(np.float32)
    return _from_volume(vol, tuple(a[1] - a[0] for a in axes), 0.0)


def _noise(border, level):
    v = np.full((40, 40, 40), border, np.float32)
    v[1:-1, 1:-1, 1:-1] = np.random.default_rng(1).standard_normal((38, 38, 38)).astype(np.float32)
    return _from_volume(v, (1.0, 1.0, 1.0), level)


def _strip(n_verts, seed):
    """a triangle strip (i, i+1, i+2) over a zigzag of points, vertex ids permuted and faces shuffled"""
    rng = np.random.default_rng(seed)
    i = np.arange(n_verts)
    pos = np.stack([0.5 * i, (i % 2).astype(np.float64), 0.25 * (i % 3)], 1)
    faces = np.stack([i[:-2], i[1:-1], i[2:]], 1)
    new_id = rng.permutation(n_verts)
    verts = np.empty_like(pos)
    verts[new_id] = pos
    faces = new_id[faces][rng.permutation(len(faces))]
    normals = rng.standard_normal((n_verts, 3))
    return _mesh(verts, faces, normals)


def _component(mesh, label, cid):
    return submesh(mesh["verts"], mesh["faces"], mesh["normals"], label, cid)


def _unused():
    """`three` with 100 vertices that no face uses inserted between the used ones"""
    m = case("three")
    rng = np.random.default_rng(3)
    n_old = len(m["verts"])
    n_new = n_old + 100
    extra = np.sort(rng.choice(n_new, 100, replace=False))
    keep = np.setdiff1d(np.arange(n_new), extra)           # new id of old vertex i, ascending
    verts = rng.standard_normal((n_new, 3)).astype(np.float32)
    normals = rng.standard_normal((n_new, 3)).astype(np.float32)
    verts[keep] = m["verts"]
    normals[keep] = m["normals"]
    return _mesh(verts, keep[m["faces"]], normals)


def _tie():
    """the small sphere of `three` on a 2^-12 grid, and its copy moved by multiples of 2^-12: every coordinate and
    every edge vector is exact in fp32, so the two components have the same face areas in the same order"""
    m = case("three")
    ref = reference("three")
    small = int(ref["ids"][np.argmin(ref["area"])])
    v, f, n = _component(m, ref["label"], small)
    v = np.round(v.astype(np.float64) * 4096.0) / 4096.0
    shift = np.array([-0.75, 0.5, -0.25])
    verts = np.concatenate([v, v + shift])
    assert np.array_equal(verts.astype(np.float32).astype(np.float64), verts)
    return _mesh(verts, np.concatenate([f, f + len(v)]), np.concatenate([n, n]))


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(11)
    if name == "three":
        return _three()
    if name == "noise":
        return _noise(1.0, 0.0)
    if name == "noise_many":
        return _noise(-3.0, 1.5)
    if name == "strip":
        return _strip(100002, 7)
    if name.startswith("strip_"):
        return _strip(int(name[6:]), 7)
    if name == "empty":
        return _mesh(rng.standard_normal((5, 3)), np.zeros((0, 3)), rng.standard_normal((5, 3)))
    if name == "one_face":
        return _mesh(rng.standard_normal((3, 3)), [[2, 0, 1]], rng.standard_normal((3, 3)))
    if name == "lone_vertex":
        return _mesh(rng.standard_normal((1, 3)), np.zeros((0, 3)), rng.standard_normal((1, 3)))
    if name == "unused":
        return _unused()
    if name == "repeated":
        # (3, 3, 4) has no area but joins 3 to 4; vertex 7 is in no face
        verts = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2], [3, 2, 2], [3, 4, 2], [3, 4, 5], [9, 9, 9]]
        return _mesh(verts, [[4, 5, 6], [0, 1, 2], [3, 3, 4]], rng.standard_normal((8, 3)))
    if name == "tie":
        return _tie()
    raise KeyError(name)


# ---- the reference: TriMesh.split restated -----------------------------------------------------------------
def labels(faces, n_verts):
    """label [V] int64: the smallest vertex id of the component of v (vertices joined by the faces' edges)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    rows = np.concatenate([f[:, 0], f[:, 1]])
    cols = np.concatenate([f[:, 1], f[:, 2]])
    graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n_verts, n_verts))
    _, comp = connected_components(graph, directed=False)
    lowest = np.full(int(comp.max()) + 1 if n_verts else 0, n_verts, np.int64)
    np.minimum.at(lowest, comp, np.arange(n_verts))
    return lowest[comp]


def submesh(verts, faces, normals, label, cid):
    """(verts, faces, normals) of the component with label cid, as TriMesh.split builds it"""
    ff = faces[label[faces[:, 0]] == cid]
    used, inv = np.unique(ff, return_inverse=True)
    return verts[used], inv.reshape(-1, 3), normals[used]


def face_areas(verts, faces):
    v = np.asarray(verts, np.float64)[faces]
    return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)


@functools.lru_cache(maxsize=None)
def reference(name):
    m = case(name)
    f = m["faces"]
    label = labels(f, len(m["verts"]))
    ids = np.unique(label[np.unique(f)]) if len(f) else np.zeros(0, np.int64)
    rank = np.searchsorted(ids, label[f[:, 0]])
    area = np.bincount(rank, weights=face_areas(m["verts"], f), minlength=len(ids)).astype(np.float64)
    count = np.bincount(rank, minlength=len(ids)).astype(np.int64)
    return _frozen(label=label, ids=ids.astype(np.int64), area=area, count=count)


def largest(name):
    """(verts, faces, normals) of the component numpy's argmax picks; the mesh itself without faces"""
    m, ref = case(name), reference(name)
    if len(m["faces"]) == 0:
        return m["verts"], m["faces"], m["normals"]
    return _component(m, ref["label"], int(ref["ids"][np.argmax(ref["area"])]))
