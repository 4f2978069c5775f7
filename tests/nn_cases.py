"""Shared inputs of the Chamfer-evaluation tests (numpy only) and the numpy restatements that serve as the references
of the HIP kernels (csrc/hm_nn.hip, csrc/hm_mesh_sample.hip):

  nn_ref(query, points, max_dist2)     brute force in fp32 with the kernel's expression, numpy's first minimum
  sample_ref(verts, faces, density)    the DTU upsampling rule as include/hashmod.h states it, in fp64
  chamfer_ref(a, b, max_dist)          the metric in fp64 from cKDTree distances

cloud(name) -> (points [n,3] f4, query [m,3] f4); everything is computed once and read-only."""
import functools

import numpy as np

UNIFORM = ((1, 1), (1, 257), (63, 64), (64, 65), (65, 63), (4097, 1000))
CLOUDS = tuple(f"uniform_{n}_{m}" for n, m in UNIFORM) + ("clusters", "identical", "plane", "lattice", "outside")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _f4(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


# ---- the references ----------------------------------------------------------------------------------------
def nn_ref(query, points, max_dist2=np.inf):
    """(d2 [m] f4, index [m] i4): argmin over all points of the fp32 value (dx*dx + dy*dy) + dz*dz, every operation
    rounded once, the lowest index among equal values; (inf, -1) where the minimum is > max_dist2"""
    q, p = _f4(query), _f4(points)
    d2 = np.empty(len(q), np.float32)
    idx = np.empty(len(q), np.int32)
    step = max(1, (1 << 22) // max(len(p), 1))
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(0, len(q), step):
            d = q[s:s + step, None, :] - p[None, :, :]
            d *= d
            v = (d[..., 0] + d[..., 1]) + d[..., 2]
            assert v.dtype == np.float32
            k = np.argmin(v, axis=1)
            idx[s:s + step] = k
            d2[s:s + step] = v[np.arange(len(k)), k]
    far = ~(d2 <= np.float32(max_dist2))
    d2[far] = np.inf
    idx[far] = -1
    return d2, idx


def sample_counts(verts, faces, density):
    """(n1 [F], n2 [F]) as float64, 0 for a face without samples, and (a, v1, v2)"""
    v = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64).reshape(-1, 3)]
    a, v1, v2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]

    def norm(w):
        return np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])

    l1, l2 = norm(v1), norm(v2)
    cr = np.stack([v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1], v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2],
                   v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]], 1)
    A2 = norm(cr)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        thr = np.float64(density) * np.sqrt(l1 * l2 / A2)
        n1, n2 = np.floor(l1 / thr), np.floor(l2 / thr)
    ok = (A2 > 0) & (n1 >= 1) & (n2 >= 1)
    return np.where(ok, n1, 0.0), np.where(ok, n2, 0.0), (a, v1, v2)


def sample_ref(verts, faces, density):
    """(samples [S,3] f4, face_of [S] i4): faces ascending, i outer, j inner"""
    n1, n2, (a, v1, v2) = sample_counts(verts, faces, density)
    pts, owner = [np.zeros((0, 3), np.float32)], [np.zeros(0, np.int32)]
    for f in np.nonzero(n1)[0]:
        u = (np.arange(int(n1[f]) + 1, dtype=np.float64) + 0.5) / n1[f]
        w = (np.arange(int(n2[f]) + 1, dtype=np.float64) + 0.5) / n2[f]
        U, W = np.meshgrid(u, w, indexing="ij")
        keep = U + W < 1.0
        U, W = U[keep][:, None], W[keep][:, None]
        pts.append(((v1[f] * U + v2[f] * W) + a[f]).astype(np.float32))
        owner.append(np.full(len(U), f, np.int32))
    return np.concatenate(pts), np.concatenate(owner)


def one_sided_ref(src, dst):
    """fp64 nearest-neighbour distances src -> dst of the fp32 clouds"""
    from scipy.spatial import cKDTree
    return cKDTree(np.asarray(dst, np.float64)).query(np.asarray(src, np.float64), workers=16)[0]


def chamfer_ref(a, b, max_dist=None):
    """(mean_a2b, mean_b2a, overall, n_a2b, n_b2a, d_ab, d_ba)"""
    d_ab, d_ba = one_sided_ref(a, b), one_sided_ref(b, a)
    ka = d_ab < max_dist if max_dist is not None else np.ones(len(d_ab), bool)
    kb = d_ba < max_dist if max_dist is not None else np.ones(len(d_ba), bool)
    ma = d_ab[ka].mean() if ka.any() else np.nan
    mb = d_ba[kb].mean() if kb.any() else np.nan
    return ma, mb, 0.5 * (ma + mb), int(ka.sum()), int(kb.sum()), d_ab, d_ba


# ---- the clouds ----------------------------------------------------------------------------------------------
def lattice():
    g = np.arange(8, dtype=np.float32)
    return _f4(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1))


@functools.lru_cache(maxsize=None)
def cloud(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("uniform_"):
        n, m = map(int, name.split("_")[1:])
        return _frozen(_f4(rng.random((n, 3))), _f4(rng.random((m, 3)) * 1.2 - 0.1))
    if name == "clusters":
        # two clusters of extent ~1, 100 extents apart along x; queries on the way between them
        a = rng.random((200, 3))
        b = rng.random((200, 3)) + [100.0, 0.0, 0.0]
        q = rng.random((130, 3))
        q[:, 0] = np.linspace(-3.0, 104.0, 130)
        return _frozen(_f4(np.concatenate([a, b])), _f4(q))
    if name == "identical":
        return _frozen(_f4(np.tile([[0.25, -1.5, 3.0]], (100, 1))), _f4(rng.standard_normal((70, 3)) * 2))
    if name == "plane":
        p = rng.random((500, 3))
        p[:, 2] = 0.0
        return _frozen(_f4(p), _f4(rng.random((200, 3)) * [1.2, 1.2, 2.0] - [0.1, 0.1, 1.0]))
    if name == "lattice":
        p = lattice()
        h = np.arange(7, dtype=np.float32) + 0.5
        half = _f4(np.stack(np.meshgrid(h, h, h, indexing="ij"), -1))      # 8 minimisers each
        edge = _f4(rng.integers(0, 7, (100, 3)) + rng.integers(0, 2, (100, 3)) * 0.5)   # 1, 2, 4 or 8 minimisers
        return _frozen(p, _f4(np.concatenate([half, edge, p])))
    if name == "outside":
        p = rng.random((1000, 3))
        q = []
        for axis in range(3):
            for sign in (-1.0, 1.0):
                far = rng.random((20, 3))
                far[:, axis] = 0.5 + sign * (0.5 + np.geomspace(1e-3, 100.0, 20))
                q.append(far)
        q.append((rng.random((30, 3)) - 0.5) * 200.0)                       # beyond edges and corners
        return _frozen(_f4(p), _f4(np.concatenate(q)))
    raise KeyError(name)


def cells(points):
    """the `cell` arguments every cloud is searched with: the default, one cell, 1/64 of the extent (mostly empty)"""
    ext = float((points.max(0) - points.min(0)).max())
    return [None, 4.0 * ext if ext > 0 else 1.0, ext / 64 if ext > 0 else 1.0 / 64]


@functools.lru_cache(maxsize=None)
def reference(name, max_dist2=np.inf):
    p, q = cloud(name)
    return _frozen(*nn_ref(q, p, max_dist2))


def n_minimisers(query, points):
    """how many points attain the fp32 minimum of each query"""
    q, p = _f4(query), _f4(points)
    d = q[:, None, :] - p[None, :, :]
    d *= d
    v = (d[..., 0] + d[..., 1]) + d[..., 2]
    return (v == v.min(1, keepdims=True)).sum(1)


@functools.lru_cache(maxsize=None)
def sphere_clouds(n=200000):
    """(points, query): noisy points of the unit sphere and points on it"""
    rng = np.random.default_rng(5)
    p = rng.standard_normal((n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    q = rng.standard_normal((n, 3))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return _frozen(_f4(p + 0.01 * rng.standard_normal((n, 3))), _f4(q))


# ---- meshes ---------------------------------------------------------------------------------------------------
RIGHT = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
RIGHT_COUNTS = {0.6: 0, 0.3: 3, 0.1: 45, 0.01: 4950}


def sphere_volume(n=32):
    ax = np.linspace(-1.0, 1.0, n)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (np.sqrt(X * X + Y * Y + Z * Z) - 0.7).astype(np.float32), (ax[1] - ax[0],) * 3


@functools.lru_cache(maxsize=None)
def icosphere(level=2):
    """(verts f4, faces i4) of a subdivided icosahedron on the unit sphere: near-equilateral faces"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
         [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10],
         [8, 6, 7], [9, 8, 1]]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                w = v[i] + v[j]
                v.append(w / np.linalg.norm(w))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return _frozen(np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32))


@functools.lru_cache(maxsize=None)
def big_among_small():
    """one triangle with n1 ~ 300 at density 0.01 among 1000 small ones, shuffled"""
    rng = np.random.default_rng(9)
    base = rng.random((1000, 1, 3)) * 4.0
    small = base + rng.random((1000, 3, 3)) * 0.05
    big = np.array([[[0.0, 0.0, 5.0], [3.0, 0.1, 5.0], [0.2, 2.8, 5.15]]])
    tris = np.concatenate([small, big])[rng.permutation(1001)]
    return _frozen(_f4(tris), np.arange(3003, dtype=np.int32).reshape(-1, 3))


@functools.lru_cache(maxsize=None)
def odd_faces():
    """a zero-area face, a face with a repeated vertex, a sliver, a triangle smaller than the density 0.05, and one
    ordinary face"""
    verts = _f4([[0, 0, 0], [1, 1, 1], [2, 2, 2],            # collinear: no area
                 [0, 0, 0], [10, 0, 0], [5, 0.01, 0],        # sliver
                 [3, 3, 3], [3.01, 3, 3], [3, 3.01, 3],      # smaller than the density
                 [0, 0, 1], [1, 0, 1], [0, 1, 1]])
    faces = np.array([[0, 1, 2], [9, 9, 10], [3, 4, 5], [6, 7, 8], [9, 10, 11]], np.int32)
    return _frozen(verts, faces)


def perturbed_target(verts, n, sigma, seed=21):
    """n points: seeded vertices of the mesh moved by sigma-scaled noise"""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(verts), n)
    return _f4(np.asarray(verts, np.float64)[pick] + sigma * rng.standard_normal((n, 3)))
