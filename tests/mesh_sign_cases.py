"""Shared inputs of the signed point-to-mesh distance tests (numpy only) and the numpy restatement that is the reference
of the HIP kernels (csrc/hm_mesh_topo.hip), by the definition of include/hashmod.h:

  topology_ref(verts, faces)                           (VN [V,3] f8, EN [F,3,3] f8, (boundary, nonmanifold, flipped)):
                                                       the pseudo-normal tables and the counts, every sum in the stated
                                                       order (ascending face, then corner / half-edge, from 0)
  sign_ref(query, verts, faces, closest, VN, EN)       (sd [m] f4, sign [m] i4) of a closest-point result
                                                       (d2, face, point, feature) and the two tables
  winding_ref(query, verts, faces)                     the generalised winding number, an fp64 solid-angle sum: an
                                                       independent inside / outside of a closed mesh

case(name) -> (verts [V,3] f4, faces [F,3] i4, query [m,3] f4); everything is computed once and read-only."""
import functools
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import mc_ref
import mesh_dist_cases as MC
import nn_cases as NC

FANS = (65, 257, 300)
NEW_CASES = (("displaced3", "mc_sphere") + tuple(f"fan_{n}" for n in FANS) + ("three_on_edge", "flipped1"))
CASES = MC.CASES + NEW_CASES
CLOSED = ("icosphere1", "icosphere2", "displaced3", "mc_sphere") + tuple(f"queries_{m}" for m in MC.QUERY_M)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


# ---- the reference -------------------------------------------------------------------------------------------
def face_quantities(verts, faces):
    """(n [F,3], nu [F,3], angle [F,3]) in fp64 from the fp32 vertices, every operation rounded once"""
    tri = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64).reshape(-1, 3)]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    n = _cross(b - a, c - a)
    nn = _dot(n, n)
    with np.errstate(all="ignore"):
        nu = np.where((nn != 0)[:, None], n / np.sqrt(nn)[:, None], 0.0)
    angle = np.empty((len(tri), 3))
    for k, (p, p1, p2) in enumerate(((a, b, c), (b, c, a), (c, a, b))):
        e1, e2 = p1 - p, p2 - p
        x = _cross(e1, e2)
        angle[:, k] = np.arctan2(np.sqrt(_dot(x, x)), _dot(e1, e2))
    return n, nu, angle


def topology_ref(verts, faces):
    """the two tables and the counts by the definition; the sums are plain loops in the stated order"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    _, nu, angle = face_quantities(verts, f)
    VN = np.zeros((len(verts), 3))
    for face in range(len(f)):
        for k in range(3):
            VN[f[face, k]] = VN[f[face, k]] + angle[face, k] * nu[face]
    runs = {}
    for face in range(len(f)):
        for k in range(3):
            v0, v1 = int(f[face, k]), int(f[face, (k + 1) % 3])
            runs.setdefault((min(v0, v1), max(v0, v1)), []).append((face, k, v0 > v1))
    EN = np.zeros((len(f), 3, 3))
    boundary = nonmanifold = flipped = 0
    for members in runs.values():                       # a run's members are in ascending (face, k) order
        s = np.zeros(3)
        for face, _, _ in members:
            s = s + nu[face]
        for face, k, _ in members:
            EN[face, k] = s
        boundary += len(members) == 1
        nonmanifold += len(members) > 2
        flipped += len(members) == 2 and members[0][2] == members[1][2]
    return VN, EN, (int(boundary), int(nonmanifold), int(flipped))


def sign_ref(query, verts, faces, closest, VN, EN, return_branch=False):
    """(sd [m] f4, sign [m] i4) of the closest-point result closest = (d2, face, point, feature) and the tables; with
    return_branch also the branch each query took (0 face, 1 edge, 2 vertex, -1 cut)"""
    q = np.ascontiguousarray(query, np.float32).reshape(-1, 3)
    v = np.asarray(verts, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    d2, face, point, feature = closest
    cut = np.asarray(face) < 0
    fc = np.where(cut, 0, face).astype(np.int64)
    ft = np.where(cut, 0, feature).astype(np.int64)
    ids = f[fc]
    a, b, c = v[ids[:, 0]], v[ids[:, 1]], v[ids[:, 2]]
    a64, b64, c64 = a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)
    n = _cross(b64 - a64, c64 - a64)
    rows = np.arange(len(q))
    k = np.maximum(ft - 1, 0)
    i0, i1 = ids[rows, k], ids[rows, (k + 1) % 3]
    p0, p1 = v[i0], v[i1]
    with np.errstate(all="ignore"):
        e = p1 - p0
        ee = _dot(e, e)
        t = np.where(ee > 0, _dot(q - p0, e) / np.where(ee > 0, ee, np.float32(1)), np.float32(0))
        assert t.dtype == np.float32
        N_edge = np.where((t <= 0)[:, None], VN[i0], np.where((t >= 1)[:, None], VN[i1], EN[fc, k]))
        interior = (ft == 0)[:, None]
        N = np.where(interior, n, N_edge)
        w = np.where(interior, q - a, q - np.asarray(point, np.float32)).astype(np.float64)
        s = _dot(w, N)
        sign = np.where(s < 0, -1, 1).astype(np.int32)
        sd = (sign * np.sqrt(np.asarray(d2, np.float32))).astype(np.float32)
    sign[cut], sd[cut] = 0, np.inf
    if return_branch:
        branch = np.where(ft == 0, 0, np.where((t <= 0) | (t >= 1), 2, 1))
        return sd, sign, np.where(cut, -1, branch)
    return sd, sign


def winding_ref(query, verts, faces):
    """w [m] f8: the sum over the faces of the signed solid angle (Van Oosterom and Strackee) over 4 pi - 1 inside a
    closed outward-wound mesh, 0 outside, meaningless on the surface"""
    q = np.asarray(query, np.float32).astype(np.float64).reshape(-1, 3)
    tri = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64).reshape(-1, 3)]
    corner = [[np.ascontiguousarray(tri[:, m, x])[None, :] for x in range(3)] for m in range(3)]
    out = np.empty(len(q))
    step = max(1, (1 << 16) // max(len(tri), 1))        # [step, F] temporaries that stay in the cache

    def chunk(s):
        p = q[s:s + step]
        (ax, ay, az), (bx, by, bz), (cx, cy, cz) = ([corner[m][x] - p[:, x, None] for x in range(3)] for m in range(3))
        la, lb, lc = np.sqrt(ax * ax + ay * ay + az * az), np.sqrt(bx * bx + by * by + bz * bz), \
            np.sqrt(cx * cx + cy * cy + cz * cz)
        num = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)
        den = (la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la
               + (cx * ax + cy * ay + cz * az) * lb)
        out[s:s + step] = np.arctan2(num, den).sum(1) / (2.0 * math.pi)

    starts = range(0, len(q), step)
    if len(q) * len(tri) < 1 << 22:
        for s in starts:
            chunk(s)
    else:                                               # numpy releases the lock: the chunks of a large job in threads
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            list(pool.map(chunk, starts))
    return out


# ---- the cases -----------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def displaced_icosphere(level=3):
    """the icosphere moved radially to r = 1 + 0.3 sin 5x sin(4y+1) cos 3z: closed and not convex"""
    v, f = NC.icosphere(level)
    x, y, z = v.astype(np.float64).T
    r = 1.0 + 0.3 * np.sin(5 * x) * np.sin(4 * y + 1) * np.cos(3 * z)
    return _frozen(NC._f4(v.astype(np.float64) * r[:, None]), f)


@functools.lru_cache(maxsize=None)
def mc_sphere(n=20):
    """marching cubes of a bumpy sphere on an n^3 lattice over [-1, 1]^3, wound outward"""
    ax = np.linspace(-1.0, 1.0, n)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    r = np.sqrt(X * X + Y * Y + Z * Z)
    vol = (r - (0.62 + 0.12 * np.sin(4 * X + 0.3) * np.cos(3 * Y) * np.sin(5 * Z + 1))).astype(np.float32)
    v, f, _ = mc_ref.marching_cubes(vol, 0.0, (ax[1] - ax[0],) * 3)
    v = NC._f4(v.astype(np.float64) - 1.0)
    f = np.ascontiguousarray(f, np.int32)
    if mc_ref.signed_volume(v, f) < 0:
        f = np.ascontiguousarray(f[:, ::-1])
    return _frozen(v, f)


def fan(n):
    """n faces around one apex above a regular n-gon: vertex 0 has a run of n corners, every rim vertex one of two"""
    ang = 2.0 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], 1)
    v = NC._f4(np.concatenate([[[0.0, 0.0, 0.5]], rim]))
    i = np.arange(n)
    return v, np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], 1).astype(np.int32)


def three_on_edge():
    """three faces on the edge (0, 1): a book of three pages"""
    v = NC._f4([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -0.5, 1], [0.5, -0.5, -1]])
    return v, np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]], np.int32)


def flipped_icosphere():
    """icosphere(1) with the winding of face 5 reversed"""
    v, f = NC.icosphere(1)
    f = np.array(f)
    f[5] = f[5, ::-1]
    return v, f


def query_mix(verts, faces, rng, n_box, n_cen, n_vert):
    """box queries, queries 1e-2 and 1e-4 from centroids, queries 1e-5 .. 0.3 off vertices"""
    v64 = verts.astype(np.float64)
    pick = rng.integers(0, len(verts), n_vert)
    d = rng.standard_normal((n_vert, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    off = np.geomspace(1e-5, 0.3, n_vert)[:, None]
    box = MC.box_queries(verts, n_box, rng)
    near, nearer = (MC.centroid_queries(verts, faces, n_cen, rng, o) for o in (1e-2, 1e-4))
    return NC._f4(np.concatenate([box, near, nearer, v64[pick] + off * d]))


@functools.lru_cache(maxsize=None)
def case(name):
    if name in MC.CASES:
        return MC.case(name)
    rng = np.random.default_rng(sum(map(ord, name)) + 177)
    if name == "displaced3":
        v, f = displaced_icosphere(3)
    elif name == "mc_sphere":
        v, f = mc_sphere()
    elif name.startswith("fan_"):
        v, f = fan(int(name.split("_")[1]))
    elif name == "three_on_edge":
        v, f = three_on_edge()
    elif name == "flipped1":
        v, f = flipped_icosphere()
    else:
        raise KeyError(name)
    return _frozen(np.ascontiguousarray(v), np.ascontiguousarray(f), query_mix(v, f, rng, 150, 50, 100))


@functools.lru_cache(maxsize=None)
def reference(name, max_dist2=np.inf):
    """closest_ref of the case: (d2, face, point, feature)"""
    if name in MC.CASES:
        return MC.reference(name, max_dist2)
    v, f, q = case(name)
    return _frozen(*MC.closest_ref(q, v, f, max_dist2))


@functools.lru_cache(maxsize=None)
def topology(name):
    v, f, _ = case(name)
    VN, EN, counts = topology_ref(v, f)
    return _frozen(VN, EN) + (counts,)


def extent(verts):
    return float((verts.max(0) - verts.min(0)).max())


# what the definition gives for mesh_dist_cases.PLANAR_QUERIES, in order: above is +, below is -, in the plane beyond
# the rim is + (s == 0), on a vertex is + (d2 == 0)
PLANAR_SIGNS = (1, 1, 1, 1, 1, 1, 1, 1, 1, -1)
