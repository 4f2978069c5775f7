"""Shared inputs of the point-to-mesh distance tests (numpy only) and the numpy restatement that is the reference of
the HIP kernels (csrc/hm_mesh_dist.hip):

  closest_ref(query, verts, faces, max_dist2, dtype)   the definition of include/hashmod.h over all faces, numpy's
                                                       first minimum; (d2, face, point, feature)
  closest_ref_near(query, verts, faces)                the same rule in fp64 over the faces that can hold the minimum
                                                       (a proved superset found with a k-d tree), for sizes at which
                                                       all pairs are too many

case(name) -> (verts [V,3] f4, faces [F,3] i4, query [m,3] f4); everything is computed once and read-only."""
import functools
import itertools

import numpy as np

import nn_cases as NC

SOUP_F = (63, 64, 65, 255, 256, 257)
QUERY_M = (1, 63, 64, 65, 1000)
CASES = (("icosphere1", "icosphere2", "odd_faces", "big_among_small", "planar", "clusters", "single", "outside")
         + tuple(f"soup_{f}" for f in SOUP_F) + tuple(f"queries_{m}" for m in QUERY_M))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- the reference -------------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def face_values(q, a, b, c):
    """(d2, point, feature) of the faces (a, b, c) for the queries q, all broadcast against each other along the
    leading axes ([k,1,3] against [1,F,3] or [k,K,3]); in the dtype of the inputs, every operation rounded once"""
    T = a.dtype
    zero, one = T.type(0), T.type(1)
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)

    def value(p):
        p = np.fmin(np.fmax(p, lo), hi)           # fmax / fmin: the other operand for a NaN, as fmaxf / fminf
        w = q - p
        return _dot(w, w), p

    with np.errstate(all="ignore"):
        n = _cross(b - a, c - a)
        nn = _dot(n, n)
        wa, wb, wc = a - q, b - q, c - q
        inside = ((nn > 0) & (_dot(n, _cross(wa, wb)) >= 0) & (_dot(n, _cross(wb, wc)) >= 0)
                  & (_dot(n, _cross(wc, wa)) >= 0))
        d2, point = value(q + (_dot(wa, n) / nn)[..., None] * n)
        d2 = np.where(inside, d2, T.type(np.inf))
        feature = np.zeros(d2.shape, np.int8)
        for k, (p0, p1) in enumerate(((a, b), (b, c), (c, a)), 1):
            e = p1 - p0
            ee = _dot(e, e)
            t = np.where(ee > 0, _dot(q - p0, e) / np.where(ee > 0, ee, one), zero)
            t = np.fmin(np.fmax(t, zero), one)
            d, p = value(p0 + t[..., None] * e)
            better = d < d2                        # strict: the first minimum in candidate order
            d2 = np.where(better, d, d2)
            point = np.where(better[..., None], p, point)
            feature = np.where(better, np.int8(k), feature)
    assert d2.dtype == T and point.dtype == T
    return d2, point, feature


def closest_ref(query, verts, faces, max_dist2=np.inf, dtype=np.float32):
    """(d2 [m], face [m] i4, point [m,3], feature [m] i4) in `dtype`: the brute force over all faces of the fp32
    vertices, the lowest face among equal d2; (inf, -1, nan, -1) where the minimum is > max_dist2"""
    T = np.dtype(dtype)
    q = np.ascontiguousarray(query, np.float32).reshape(-1, 3).astype(T)
    tri = np.asarray(verts, np.float32).astype(T)[np.asarray(faces, np.int64).reshape(-1, 3)]
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    m = len(q)
    d2, face = np.empty(m, T), np.empty(m, np.int32)
    point, feature = np.empty((m, 3), T), np.empty(m, np.int32)
    step = max(1, (1 << 18) // max(len(tri), 1))
    for s in range(0, m, step):
        d, p, f = face_values(q[s:s + step, None, :], a, b, c)
        k = np.argmin(d, axis=1)
        r = np.arange(len(k))
        face[s:s + step], d2[s:s + step], point[s:s + step], feature[s:s + step] = k, d[r, k], p[r, k], f[r, k]
    far = ~(d2 <= T.type(max_dist2))
    d2[far], face[far], point[far], feature[far] = np.inf, -1, np.nan, -1
    return d2, face, point, feature


def closest_ref_near(query, verts, faces):
    """d2 [m] f8 of the fp64 rule, from the faces that can hold the minimum.  The rule's value for the face with the
    nearest centroid is an upper bound u^2 of the minimum; a face with a point within u of q has its centroid within
    u + R, R the largest centroid-to-vertex distance of any face.  Those faces (found with a k-d tree over the
    centroids, the radius widened by 1e-9 relative for the tree's and the bound's own rounding) are a superset of the
    minimisers."""
    from scipy.spatial import cKDTree
    q = np.asarray(query, np.float32).astype(np.float64).reshape(-1, 3)
    tri = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64)]
    cen = tri.mean(1)
    R = np.sqrt(((tri - cen[:, None, :]) ** 2).sum(-1)).max()
    tree = cKDTree(cen)
    first = tri[tree.query(q, workers=16)[1]]
    u = np.sqrt(face_values(q, first[:, 0], first[:, 1], first[:, 2])[0])
    near = tree.query_ball_point(q, (u + R) * (1 + 1e-9) + 1e-300, workers=16)
    # the ragged (query, face) pairs laid end to end; every query has at least the face of its nearest centroid
    count = np.fromiter(map(len, near), np.int64, len(q))
    assert count.min() >= 1
    face = np.fromiter(itertools.chain.from_iterable(near), np.int64, int(count.sum()))
    t = tri[face]
    d = face_values(np.repeat(q, count, axis=0), t[:, 0], t[:, 1], t[:, 2])[0]
    return np.minimum.reduceat(d, np.cumsum(count) - count)


def n_minimisers(query, verts, faces):
    """how many faces attain the fp32 minimum of each query"""
    q = np.asarray(query, np.float32).reshape(-1, 3)
    tri = np.asarray(verts, np.float32)[np.asarray(faces, np.int64)]
    d = face_values(q[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])[0]
    return (d == d.min(1, keepdims=True)).sum(1)


def unit(query, verts, d2):
    """the unit of the fp32-against-fp64 bound per query: 2^-24 * max(M, d), M the largest coordinate magnitude of
    the mesh and the queries"""
    M = max(float(np.abs(verts).max()), float(np.abs(query).max()))
    return 2.0 ** -24 * np.maximum(M, np.sqrt(np.asarray(d2, np.float64)))


# ---- the cases -----------------------------------------------------------------------------------------------
def box_queries(verts, n, rng, scale=1.4):
    """n queries uniform in the mesh's bounding box scaled by `scale` about its centre"""
    lo, hi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3) * scale
    return mid + (rng.random((n, 3)) * 2 - 1) * half


def centroid_queries(verts, faces, n, rng, off=1e-4):
    """n queries `off` away from seeded face centroids"""
    tri = verts.astype(np.float64)[faces[rng.integers(0, len(faces), n)]]
    return tri.mean(1) + off * rng.standard_normal((n, 3))


def planar():
    """a 5x5 grid of unit squares in z = 0, each split along its (x, y) -> (x+1, y+1) diagonal"""
    g = np.arange(6, dtype=np.float32)
    X, Y = np.meshgrid(g, g, indexing="ij")
    verts = np.stack([X.ravel(), Y.ravel(), np.zeros(36, np.float32)], 1)
    faces = []
    for i in range(5):
        for j in range(5):
            v = i * 6 + j
            faces += [[v, v + 6, v + 7], [v, v + 7, v + 1]]
    return NC._f4(verts), np.asarray(faces, np.int32)


# planar's queries and the exact d2 each must have: one unit above an inner vertex (6 faces tie), above an inner edge
# midpoint (2), above a face interior (1), half a unit above a vertex, two units outside the rim in the plane, one out
# and one up from a rim edge, diagonally off the corner, ON a vertex, and below a rim vertex
PLANAR_QUERIES = (((2, 2, 1), 1.0, 6), ((2.5, 2, 1), 1.0, 2), ((2.25, 2.5, 1), 1.0, 1), ((3, 3, 0.5), 0.25, 6),
                  ((-2, 2.5, 0), 4.0, 1), ((2.5, 7, 0), 4.0, 1), ((-1, 2.5, 1), 2.0, 1), ((6, 6, 0), 2.0, 2),
                  ((2, 3, 0), 0.0, 6), ((5, 2, -1), 1.0, 3))


def _soup(rng, n):
    base = rng.random((n, 1, 3)) * 2.0
    return NC._f4(base + (rng.random((n, 3, 3)) - 0.5) * 0.4), np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(sum(map(ord, name)) + 77)

    def mixed(v, f, n_box, n_cen):
        return np.concatenate([box_queries(v, n_box, rng), centroid_queries(v, f, n_cen, rng)])

    if name in ("icosphere1", "icosphere2"):
        v, f = NC.icosphere(int(name[-1]))
        # the vertices and the edge midpoints themselves, and points straight above them: ties by construction
        on = np.concatenate([v[:20], (v[f[:20, 0]] + v[f[:20, 1]]) / 2, v[:20] * 1.5])
        return _frozen(v, f, NC._f4(np.concatenate([mixed(v, f, 200, 60), on])))
    if name == "odd_faces":
        v, f = NC.odd_faces()
        return _frozen(v, f, NC._f4(np.concatenate([mixed(v, f, 200, 60), v])))
    if name == "big_among_small":
        v, f = NC.big_among_small()
        above_big = np.stack([rng.random(40) * 2, rng.random(40) * 2, 5.0 + rng.random(40)], 1)
        return _frozen(v, f, NC._f4(np.concatenate([mixed(v, f, 200, 60), above_big])))
    if name == "planar":
        v, f = planar()
        return _frozen(v, f, NC._f4([p for p, _, _ in PLANAR_QUERIES]))
    if name == "clusters":
        # two clusters of small faces, each of extent ~1, 100 extents apart along x; queries on the way between them
        va, fa = _soup(rng, 60)
        vb, fb = _soup(rng, 60)
        q = rng.random((130, 3))
        q[:, 0] = np.linspace(-3.0, 106.0, 130)
        return _frozen(NC._f4(np.concatenate([va * 0.5, vb * 0.5 + [100.0, 0.0, 0.0]])),
                       np.concatenate([fa, fb + len(va)]).astype(np.int32), NC._f4(q))
    if name == "single":
        v = NC._f4([[0.0, 0.0, 0.0], [1.0, 0.25, 0.0], [0.25, 1.0, 0.5]])
        f = np.array([[0, 1, 2]], np.int32)
        return _frozen(v, f, NC._f4(mixed(v, f, 100, 30)))
    if name == "outside":
        v, f = _soup(rng, 300)
        q = []
        for axis in range(3):
            for sign in (-1.0, 1.0):
                far = rng.random((20, 3)) * 2
                far[:, axis] = 1.0 + sign * (1.2 + np.geomspace(1e-3, 100.0, 20))
                q.append(far)
        q.append((rng.random((30, 3)) - 0.5) * 400.0)                       # beyond edges and corners
        return _frozen(v, f, NC._f4(np.concatenate(q)))
    if name.startswith("soup_"):
        n = int(name.split("_")[1])
        v, f = _soup(np.random.default_rng(31), max(SOUP_F))                # prefixes of ONE soup
        return _frozen(v[:3 * n].copy(), f[:n].copy(), NC._f4(box_queries(v, 130, rng, 1.2)))
    if name.startswith("queries_"):
        m = int(name.split("_")[1])
        v, f = NC.icosphere(2)
        return _frozen(v, f, NC._f4(box_queries(v, m, rng)))
    raise KeyError(name)


def cells(verts):
    """the `cell` arguments every mesh is indexed with: the default, one cell, 1/64 of the extent"""
    return NC.cells(verts)


BIG_FACES = (None, 1, 1 << 40)      # the default; every multi-cell face is big; none is


@functools.lru_cache(maxsize=None)
def reference(name, max_dist2=np.inf):
    v, f, q = case(name)
    return _frozen(*closest_ref(q, v, f, max_dist2))


CLUSTERS_MAX_DIST = 10.0
