"""Shared inputs and the reference of the mesh-simplification tests (numpy only): the contract of ops.mesh_simplify
(DESIGN.md "Mesh simplification", csrc/hm_mesh_simplify.hip) restated with np.unique, np.bincount in fp64 and
np.linalg.solve.

case(name) -> {"verts" [V,3] f4, "faces" [F,3] i8, "normals" [V,3] f4, "cell" float};
reference(name, placement) -> the four outputs plus what the CPU tests look at (see simplify).  Both are computed once
and read-only."""
import functools
import math

import numpy as np

import mesh_cc_cases as CC

REG = 0.05
PLACEMENTS = ("quadric", "mean")
THREE_SPACING = 2.0 / 47.0        # the x spacing of mesh_cc_cases' `three` lattice (48 samples over [-1, 1])
MULTIPLES = (0.5, 1.7, 3.0)
NAMES = (tuple(f"three@{k}" for k in MULTIPLES) + tuple(f"noise@{k}" for k in MULTIPLES)
         + tuple(f"strip_{v}" for v in CC.BLOCK_EDGES) + tuple(f"strip_{v}@0.8" for v in CC.BLOCK_EDGES)
         + ("one_cell", "rotated_repeat", "flipped_pair", "cell_faces", "unused", "one_face", "empty"))


def _frozen(**values):
    for a in values.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return values


def _mesh(verts, faces, normals, cell):
    return _frozen(verts=np.ascontiguousarray(verts, np.float32),
                   faces=np.ascontiguousarray(faces, np.int64).reshape(-1, 3),
                   normals=np.ascontiguousarray(normals, np.float32), cell=float(cell))


def _of(name, cell):
    m = CC.case(name)
    return _mesh(m["verts"], m["faces"], m["normals"], cell)


def _one_cell():
    """5 000 vertices, all used, inside one cell: one run longer than a wave, and no face survives"""
    rng = np.random.default_rng(21)
    verts = 0.5 + 0.25 * rng.random((5000, 3))
    i = np.arange(4998)
    faces = np.concatenate([np.stack([i, i + 1, i + 2], 1), rng.integers(0, 5000, (200, 3))])
    return _mesh(verts, faces, rng.standard_normal((5000, 3)), 10.0)


def _quad(faces):
    """four vertices more than a cell apart, each a cluster of its own"""
    rng = np.random.default_rng(22)
    verts = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 1]]
    return _mesh(verts, faces, rng.standard_normal((4, 3)), 0.25)


def _cell_faces():
    """vertices exactly at lo + i h, h = 2^-2, i = 0..4 on every axis (hi included), and a few between them"""
    rng = np.random.default_rng(23)
    i = np.arange(5)
    lattice = np.stack(np.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3) * 0.25 - 0.5
    between = lattice[rng.choice(125, 40, replace=False)] + rng.choice([-2.0 ** -20, 2.0 ** -20, 0.125], (40, 3))
    verts = np.clip(np.concatenate([lattice, between]), -0.5, 0.5)
    order = rng.permutation(len(verts))
    verts = verts[order]
    assert np.array_equal(verts.astype(np.float32).astype(np.float64), verts)
    faces = np.concatenate([rng.permutation(len(verts))[:165].reshape(-1, 3) for _ in range(8)])
    return _mesh(verts, faces, rng.standard_normal((len(verts), 3)), 0.25)


def _with_odd_normals(m):
    """a zero, an infinite and a NaN normal among the first vertices"""
    n = m["normals"].copy()
    n[0] = 0.0
    n[1, 1] = np.inf
    n[2, 0] = np.nan
    return _mesh(m["verts"], m["faces"], n, m["cell"])


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("three@"):
        return _of("three", float(name[6:]) * THREE_SPACING)
    if name.startswith("noise@"):
        m = _of("noise", float(name[6:]))
        assert len(m["verts"]) == 84530
        return _with_odd_normals(m) if name == "noise@1.7" else m
    if name.startswith("strip_"):
        # at h = 1.3 every face of the zigzag has two corners in one cell and none survives: the vertex sort's block
        # edges show in nothing but an empty result, so the same strips are also clustered at 0.8, where faces survive
        base, _, cell = name.partition("@")
        return _of(base, float(cell or 1.3))
    if name == "one_cell":
        return _one_cell()
    if name == "rotated_repeat":
        return _quad([[0, 1, 2], [1, 2, 0], [0, 2, 3]])
    if name == "flipped_pair":
        return _quad([[0, 1, 2], [0, 2, 1], [3, 1, 2]])
    if name == "cell_faces":
        return _cell_faces()
    if name == "unused":
        return _of("unused", 1.7 * THREE_SPACING)
    if name == "one_face":
        return _of("one_face", 0.01)
    if name == "empty":
        return _of("empty", 0.5)
    raise KeyError(name)


# ---- the reference ---------------------------------------------------------------------------------------------
def grid(verts, cell):
    """(lo [3] f4, h f4, g [3] int) of the clustering grid over all rows of verts; ValueError beyond the limits"""
    lo, hi = verts.min(0), verts.max(0)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise RuntimeError("a vertex has a non-finite coordinate")
    h = np.float32(cell)
    g = [int(math.floor(max(float(hi[a]) - float(lo[a]), 0.0) / float(h))) + 1 for a in range(3)]
    if max(g) > 1 << 30 or g[0] * g[1] * g[2] >= 1 << 31:
        raise ValueError(f"a grid of {g} cells is beyond the limit")
    return lo, h, g


def _sums(index, weights, n):
    """[n, ...] fp64: np.bincount of every column of weights [len(index), ...]"""
    w = weights.reshape(len(index), -1)
    out = np.stack([np.bincount(index, weights=w[:, c], minlength=n) for c in range(w.shape[1])], 1)
    return out.reshape((n,) + weights.shape[1:])


def simplify(verts, faces, normals, cell, placement="quadric", reg=REG):
    """The contract of ops.mesh_simplify.  Returns a dict: verts [C,3] f4, faces [G,3] i8, normals [C,3] f4 or None,
    vertex_map [V] i8, and about the OUTPUT clusters: members (list of vertex-id arrays), normal_ratio [C]
    (|sum n^| / k, None without normals), clamped [C] bool; n_repeats (faces removed as repeats), n_dropped (clusters
    no surviving face uses), h."""
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n_verts = len(verts)
    assert placement in PLACEMENTS and (placement == "mean" or normals is not None)
    empty = dict(verts=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int64),
                 normals=None if normals is None else np.zeros((0, 3), np.float32),
                 vertex_map=np.full(n_verts, -1, np.int64), members=[], normal_ratio=None if normals is None else
                 np.zeros(0), clamped=np.zeros(0, bool), n_repeats=0, n_dropped=0, h=float(np.float32(cell)))
    if n_verts == 0 or len(faces) == 0:
        return _frozen(**empty)
    assert faces.min() >= 0 and faces.max() < n_verts
    # 1. grid
    lo, h, g = grid(verts, cell)
    with np.errstate(all="ignore"):
        c = np.floor((verts - lo) / h)                    # float32 throughout
    assert c.dtype == np.float32
    c = np.clip(c, 0, np.asarray(g, np.float32) - 1).astype(np.int64)
    key = (c[:, 0] * g[1] + c[:, 1]) * g[2] + c[:, 2]
    # 2. members
    used = np.zeros(n_verts, bool)
    used[faces.reshape(-1)] = True
    uid = np.nonzero(used)[0]
    ukey, inv = np.unique(key[uid], return_inverse=True)
    inv = inv.reshape(-1)
    n_clusters = len(ukey)
    cluster_of = np.full(n_verts, -1, np.int64)
    cluster_of[uid] = inv
    # 3. representatives
    k = np.bincount(inv, minlength=n_clusters).astype(np.float64)
    p = verts[uid].astype(np.float64)
    m = _sums(inv, p, n_clusters) / k[:, None]
    x = m.copy()
    out_normals = ratio = None
    clamped = np.zeros(n_clusters, bool)
    if normals is not None:
        n = np.asarray(normals, np.float32)[uid].astype(np.float64)
        with np.errstate(all="ignore"):
            length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
            ok = np.isfinite(length) & (length > 0)
            nh = np.where(ok[:, None], n / np.where(ok, length, 1.0)[:, None], 0.0)
        s = _sums(inv, nh, n_clusters)
        sl = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        out_normals = np.where((sl > 0)[:, None], s / np.where(sl > 0, sl, 1.0)[:, None], 0.0)
        ratio = sl / k
    if placement == "quadric":
        d = (nh * (p - m[inv])).sum(1)
        b = _sums(inv, nh * d[:, None], n_clusters)
        A = _sums(inv, nh[:, :, None] * nh[:, None, :], n_clusters) + (reg * k)[:, None, None] * np.eye(3)
        x = m + np.linalg.solve(A, b[:, :, None])[:, :, 0]
        cells = np.stack([ukey // g[2] // g[1], ukey // g[2] % g[1], ukey % g[2]], 1)
        blo = lo.astype(np.float64) + cells * float(h)
        bhi = blo + float(h)
        xc = np.clip(x, np.minimum(blo, m), np.maximum(bhi, m))
        clamped = np.any(xc != x, 1)
        x = xc
    # 4. faces
    fc = cluster_of[faces]
    t = fc[(fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])]
    r = np.argmin(t, 1) if len(t) else np.zeros(0, np.int64)
    t = t[np.arange(len(t))[:, None], (r[:, None] + np.arange(3)) % 3]
    first = np.sort(np.unique(t, axis=0, return_index=True)[1]) if len(t) else np.zeros(0, np.int64)
    n_repeats = len(t) - len(first)
    t = t[first]
    # 5. compaction
    cu = np.unique(t)
    new_id = np.full(n_clusters, -1, np.int64)
    new_id[cu] = np.arange(len(cu))
    order = np.argsort(inv, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(k.astype(np.int64))])
    return _frozen(verts=x[cu].astype(np.float32), faces=new_id[t].reshape(-1, 3),
                   normals=None if out_normals is None else out_normals[cu].astype(np.float32),
                   vertex_map=np.where(cluster_of >= 0, new_id[np.maximum(cluster_of, 0)], -1),
                   members=[uid[order[bounds[c]:bounds[c + 1]]] for c in cu],
                   normal_ratio=None if ratio is None else ratio[cu], clamped=clamped[cu], n_repeats=n_repeats,
                   n_dropped=n_clusters - len(cu), h=float(h))


@functools.lru_cache(maxsize=None)
def reference(name, placement="quadric", with_normals=True):
    m = case(name)
    return simplify(m["verts"], m["faces"], m["normals"] if with_normals else None, m["cell"], placement)
