"""Shared inputs of the mesh ray-casting tests (numpy only) and the numpy restatements that are the reference of the
HIP kernel (csrc/hm_mesh_ray.hip):

  face_values(o, d, a, b, c, pad, t_min, t_max)   the definition of include/hashmod.h per (ray, face), broadcast
  ray_ref(origins, dirs, verts, faces, pad, ...)  the brute force over all faces: (t, face, uv, point)
  walk_ref(origins, dirs, index, ...)             the kernel's slab walk over a dict-of-cells index (grid_index)
  n_hitters(...)                                  how many faces attain the winning t of each ray

case(name) -> (verts [V,3] f4, faces [F,3] i4, origins [m,3] f4, dirs [m,3] f4, t_min [m] f4, t_max [m] f4);
everything is computed once and read-only.  The meshes are those of mesh_dist_cases."""
import functools
import math

import numpy as np

import mesh_dist_cases as MC
import nn_cases as NC

RAYS_M = (1, 63, 64, 65, 1000)
MESHES = (("icosphere1", "icosphere2", "odd_faces", "big_among_small", "planar", "clusters", "single")
          + tuple(f"soup_{f}" for f in MC.SOUP_F))
CASES = MESHES + tuple(f"rays_{m}" for m in RAYS_M)
BIG_FACE = 64           # ops.MESH_DIST_BIG_FACE
FLT_MAX = np.float32(np.finfo(np.float32).max)

_frozen = MC._frozen
_dot, _cross = MC._dot, MC._cross


# ---- the reference -------------------------------------------------------------------------------------------
def face_values(o, d, a, b, c, pad, t_min, t_max, dtype=np.float32):
    """(t, u, v, p, hit) of the faces (a, b, c) for the rays (o, d, t_min, t_max), all broadcast against each other
    along the leading axes ([k,1,3] against [1,F,3]; t_min, t_max [k,1]); in `dtype`, every operation rounded once.
    t is inf where the face is not hit."""
    T = np.dtype(dtype)
    o, d, a, b, c = (np.asarray(x, T) for x in (o, d, a, b, c))
    pad, t_min, t_max = T.type(pad), np.asarray(t_min, T), np.asarray(t_max, T)
    with np.errstate(all="ignore"):
        lo = np.minimum(np.minimum(a, b), c) - pad
        hi = np.maximum(np.maximum(a, b), c) + pad
        e1, e2 = b - a, c - a
        pv = _cross(d, e2)
        det = _dot(e1, pv)
        tv = o - a
        u = _dot(tv, pv) / det
        qv = _cross(tv, e1)
        v = _dot(d, qv) / det
        t = _dot(e2, qv) / det
        p = o + t[..., None] * d
        hit = ((det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= t_min) & (t <= t_max)
               & ((p >= lo) & (p <= hi)).all(-1))
    assert t.dtype == T and p.dtype == T and u.dtype == T
    return np.where(hit, t, T.type(np.inf)), u, v, p, hit


def _bounds(m, t_min, t_max, T):
    return (np.broadcast_to(np.asarray(t_min, np.float32), (m,)).astype(T),
            np.broadcast_to(np.asarray(t_max, np.float32), (m,)).astype(T))


def ray_ref(origins, dirs, verts, faces, pad, t_min=0.0, t_max=np.inf, dtype=np.float32):
    """(t [m], face [m] i4, uv [m,2], point [m,3]) in `dtype`: the brute force over all faces of the fp32 mesh and
    rays, the smallest t and the lowest face among equal t; (inf, -1, nan, nan) for a miss"""
    T = np.dtype(dtype)
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3).astype(T)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3).astype(T)
    m = len(o)
    lo_t, hi_t = _bounds(m, t_min, t_max, T)
    tri = np.asarray(verts, np.float32).astype(T)[np.asarray(faces, np.int64).reshape(-1, 3)]
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    t, face = np.empty(m, T), np.empty(m, np.int32)
    uv, point = np.empty((m, 2), T), np.empty((m, 3), T)
    step = max(1, (1 << 18) // max(len(tri), 1))
    for s in range(0, m, step):
        e = slice(s, s + step)
        tt, u, v, p, _ = face_values(o[e, None, :], d[e, None, :], a, b, c, T.type(np.float32(pad)), lo_t[e, None],
                                     hi_t[e, None], T)
        k = np.argmin(tt, axis=1)                  # the first minimum: the lowest face
        r = np.arange(len(k))
        t[e], face[e], point[e] = tt[r, k], k, p[r, k]
        uv[e, 0], uv[e, 1] = u[r, k], v[r, k]
    miss = ~(t < np.inf)
    t[miss], face[miss], uv[miss], point[miss] = np.inf, -1, np.nan, np.nan
    return t, face, uv, point


def n_hitters(origins, dirs, verts, faces, pad, t_min=0.0, t_max=np.inf):
    """how many faces are hit at the winning fp32 t of each ray (0 for a miss)"""
    o, d = NC._f4(origins), NC._f4(dirs)
    lo_t, hi_t = _bounds(len(o), t_min, t_max, np.float32)
    tri = np.asarray(verts, np.float32)[np.asarray(faces, np.int64)]
    t = face_values(o[:, None, :], d[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], pad,
                    lo_t[:, None], hi_t[:, None])[0]
    best = t.min(1, keepdims=True)
    return ((t == best) & (best < np.inf)).sum(1)


def default_pad(verts):
    """ops.mesh_ray_pad: fp32(2^-12 * the largest fp32 extent)"""
    v = np.asarray(verts, np.float32)
    return np.float32(2.0 ** -12) * (v.max(0) - v.min(0)).max()


def pads(verts):
    """the `pad` arguments every mesh is cast with: none, the default, an eighth of the extent"""
    v = np.asarray(verts, np.float32)
    ext = float((v.max(0) - v.min(0)).max())
    return [0.0, float(default_pad(v)), float(np.float32(ext / 8 if ext > 0 else 0.125))]


# ---- the walk ------------------------------------------------------------------------------------------------
def _cell(p, lo, h, g):
    """nn_cell for one fp32 coordinate: clamp(floor((p - lo) / h), 0, g - 1), every operation rounded once"""
    with np.errstate(all="ignore"):
        t = np.floor((np.float32(p) - np.float32(lo)) / np.float32(h))
    return min(int(min(max(t, np.float32(0)), np.float32(2.0 ** 30))), g - 1)


class GridIndex:
    """the triangle grid as a dict of cells: what ops.mesh_index builds, with the same cell function and the same
    rule for big faces"""

    def __init__(self, verts, faces, cell=None, pad=0.0, big_face=BIG_FACE):
        v = np.asarray(verts, np.float32)
        f = np.asarray(faces, np.int64)
        self.pad = np.float32(pad)
        lo, hi = v.min(0), v.max(0)
        ext = [max(float(b) - float(a), 0.0) for a, b in zip(lo, hi)]
        if cell is None:
            area = ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2]
            cell = math.sqrt(32.0 * area / len(f)) if area > 0 else (32.0 * max(ext) / len(f) if max(ext) > 0 else 1.0)
        self.h = np.float32(cell)
        self.lo = lo
        self.g = [int(math.floor(e / float(self.h))) + 1 for e in ext]
        self.tri = v[f]
        self.cells, self.big = {}, []
        with np.errstate(all="ignore"):
            blo, bhi = self.tri.min(1) - self.pad, self.tri.max(1) + self.pad
        for i in range(len(f)):
            c0 = [_cell(blo[i, a], lo[a], self.h, self.g[a]) for a in range(3)]
            c1 = [_cell(bhi[i, a], lo[a], self.h, self.g[a]) for a in range(3)]
            if (c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1) > big_face:
                self.big.append(i)
                continue
            for x in range(c0[0], c1[0] + 1):
                for y in range(c0[1], c1[1] + 1):
                    for z in range(c0[2], c1[2] + 1):
                        self.cells.setdefault((x, y, z), []).append(i)


def _at(o, t, d):
    with np.errstate(all="ignore"):
        return np.float32(o) + np.float32(t) * np.float32(d)


def _checked(om, dm, lom, h, gm, s, w, k):
    """a time whose major-axis cell has been CHECKED to lie strictly before (w = -1) or after (w = +1) slab k in ray
    order, or None: mr_checked of the kernel"""
    f4 = np.float32
    with np.errstate(all="ignore"):
        plane = lom + f4(k + 1 if s * w > 0 else k) * h
        tg = (plane - om) / dm
        step = (max(abs(om), abs(plane), abs(lom), h) / abs(dm) + abs(tg)) * f4(2.0 ** -21)
        for _ in range(48):
            tg = tg + (step if w > 0 else -step)
            if tg == tg and w * s * (_cell(_at(om, tg, dm), lom, h, gm) - k) > 0:
                return tg
            step = step * f4(2.0)
    return None


def walk_ref(origins, dirs, index, t_min=0.0, t_max=np.inf, stats=None):
    """(t [m] f4, face [m] i4): the slab walk of csrc/hm_mesh_ray.hip, ray by ray, over a GridIndex.  stats: a dict
    that receives "face_tests" and "early_stops"."""
    o_all, d_all = NC._f4(origins), NC._f4(dirs)
    m = len(o_all)
    lo_t, hi_t = _bounds(m, t_min, t_max, np.float32)
    tri, G, h, g, pad = index.tri, index.lo, index.h, index.g, index.pad
    t_out, face_out = np.full(m, np.inf, np.float32), np.full(m, -1, np.int32)
    n_tests = n_early = 0
    big = np.asarray(index.big, np.int64)
    for i in range(m):
        o, d, tmin, tmax = o_all[i], d_all[i], lo_t[i], hi_t[i]
        best_t, best_f = np.float32(np.inf), -1

        def test(ids):
            nonlocal best_t, best_f, n_tests
            if len(ids) == 0:
                return
            n_tests += len(ids)
            t = face_values(o[None], d[None], tri[ids, 0], tri[ids, 1], tri[ids, 2], pad, tmin, tmax)[0]
            k = int(np.argmin(t))
            if t[k] < best_t or (t[k] == best_t and t[k] < np.inf and ids[k] < best_f):
                best_t, best_f = t[k], int(ids[k])

        test(big)
        T = min(tmax, FLT_MAX)
        maj = int(np.argmax(np.abs(d)))             # the first maximum: the lowest axis among equal
        om, dm, lom, gm = o[maj], d[maj], G[maj], g[maj]
        if dm != 0 and tmin <= T:
            s = 1 if dm > 0 else -1
            k = _cell(_at(om, tmin, dm), lom, h, gm)
            k1 = _cell(_at(om, T, dm), lom, h, gm)
            t_lo = tmin
            for _ in range(gm):
                t_hi = min(T, best_t)
                if k != k1:
                    ta = _checked(om, dm, lom, h, gm, s, 1, k)
                    if ta is not None:
                        t_hi = min(t_hi, ta)
                if t_lo <= t_hi:
                    rng = []
                    for a in range(3):
                        ca = _cell(_at(o[a], t_lo, d[a]), G[a], h, g[a])
                        cb = _cell(_at(o[a], t_hi, d[a]), G[a], h, g[a])
                        rng.append((k, k) if a == maj else (min(ca, cb), max(ca, cb)))
                    ids = []
                    for x in range(rng[0][0], rng[0][1] + 1):
                        for y in range(rng[1][0], rng[1][1] + 1):
                            for z in range(rng[2][0], rng[2][1] + 1):
                                ids += index.cells.get((x, y, z), ())
                    test(np.asarray(sorted(set(ids)), np.int64))
                if k == k1:
                    break
                tb = _checked(om, dm, lom, h, gm, s, -1, k + s)
                if tb is not None and best_t <= tb:
                    n_early += 1
                    break
                t_lo = max(tmin, tb) if tb is not None else tmin
                k += s
        if best_f >= 0:
            t_out[i], face_out[i] = best_t, best_f
    if stats is not None:
        stats["face_tests"], stats["early_stops"] = n_tests, n_early
    return t_out, face_out


# ---- the cases -----------------------------------------------------------------------------------------------
# planar's rays and what each must give: (origin, direction, t, hitters, winning face); straight down onto an inner
# vertex (6 faces tie), an inner edge midpoint (2), a face interior (1), the corner vertex from z = 2, past the rim,
# and a slanted ray onto the vertex (2, 1, 0)
PLANAR_RAYS = (((2, 2, 1), (0, 0, -1), 1.0, 6, 12), ((2.5, 2, 1), (0, 0, -1), 1.0, 2, 23),
               ((2.25, 2.5, 1), (0, 0, -1), 1.0, 1, 25), ((0, 0, 2), (0, 0, -1), 2.0, 2, 0),
               ((-2, 2.5, 1), (0, 0, -1), math.inf, 0, -1), ((0.5, 0.25, 3), (0.5, 0.25, -1), 3.0, 6, None))


def _unit(rng, n):
    w = rng.standard_normal((n, 3))
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def _rays(v, f, rng):
    """344 seeded rays of every kind for the mesh (v, f): (origins, dirs, t_min, t_max) in fp32"""
    v64 = v.astype(np.float64)
    lo, hi = v64.min(0), v64.max(0)
    mid, ext = (lo + hi) / 2, max(float((hi - lo).max()), 1e-3)
    tri = v64[f]
    O, D, LO, HI = [], [], [], []

    def add(o, d, t_min=0.0, t_max=np.inf):
        o, d = np.atleast_2d(o), np.atleast_2d(d)
        O.append(o)
        D.append(np.broadcast_to(d, o.shape))
        LO.append(np.broadcast_to(np.asarray(t_min, np.float64), (len(o),)))
        HI.append(np.broadcast_to(np.asarray(t_max, np.float64), (len(o),)))

    def outside(n, far=2.0):
        return mid + far * ext * _unit(rng, n)

    def centroids(n, jitter=1e-3):
        return tri[rng.integers(0, len(f), n)].mean(1) + jitter * ext * rng.standard_normal((n, 3))

    def aim(o, target, scale=1.0, **kw):
        """fp32 rays from o through the fp32 target: the direction is target - origin, rounded once"""
        o32, t32 = NC._f4(o), NC._f4(target)
        add(o32, (t32 - o32).astype(np.float64) * scale, **kw)

    o = outside(40)
    w = centroids(40) - o
    add(o, w / np.linalg.norm(w, axis=1, keepdims=True))                           # unit, at jittered centroids
    pick = rng.integers(0, len(f), 30)
    aim(outside(30), v64[f[pick, 0]])                                              # exactly at vertices
    aim(outside(30), (v[f[pick, 0]] + v[f[pick, 1]]).astype(np.float64) / 2)       # and at edge midpoints
    for axis in range(3):
        for sign in (-1.0, 1.0):
            o = np.concatenate([centroids(3), v64[rng.integers(0, len(v), 3)]])    # through faces and through vertices
            o[:, axis] = mid[axis] - sign * 2 * ext
            add(NC._f4(o), np.eye(3)[axis] * sign)
    add(lo + rng.random((20, 3)) * (hi - lo), _unit(rng, 20))                      # origins inside the box
    add(NC._f4(tri[rng.integers(0, len(f), 10)].mean(1)), _unit(rng, 10))          # origins on the mesh: t = 0
    add(v64[rng.integers(0, len(v), 10)], _unit(rng, 10))
    aim(outside(20, far=100.0), centroids(20))                                     # 100 extents away, t about 1
    o = outside(20)
    add(o, (o - mid) / np.linalg.norm(o - mid, axis=1, keepdims=True))             # pointing away: misses
    add(outside(4), np.zeros(3))                                                   # zero directions
    for length in (1e-3, 1e3):
        o = outside(20)
        w = centroids(20) - o
        add(o, w / np.linalg.norm(w, axis=1, keepdims=True) * length)
    aim(outside(64), centroids(64, jitter=0.02), t_max=1.0)                        # segments: target minus origin
    o = outside(20)                                                                # t_min beyond the first hit
    c = centroids(20, jitter=0.0)
    dist = np.linalg.norm(c - o, axis=1)
    add(o, (c - o) / dist[:, None], t_min=dist + 0.01 * ext)
    return (NC._f4(np.concatenate(O)), NC._f4(np.concatenate(D)), np.concatenate(LO).astype(np.float32),
            np.concatenate(HI).astype(np.float32))


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(sum(map(ord, name)) + 191)
    if name.startswith("rays_"):
        m = int(name.split("_")[1])
        v, f = NC.icosphere(2)
        o = 3.0 * _unit(rng, m)
        w = (rng.random((m, 3)) * 2 - 1) * 0.9 - o                                 # through the box: most of them hit
        return _frozen(v, f, NC._f4(o), NC._f4(w / np.linalg.norm(w, axis=1, keepdims=True)),
                       np.zeros(m, np.float32), np.full(m, np.inf, np.float32))
    v, f = MC.case(name)[:2]
    o, d, t_min, t_max = _rays(v, f, rng)
    if name == "planar":
        k = len(PLANAR_RAYS)
        o = np.concatenate([NC._f4([r[0] for r in PLANAR_RAYS]), o])
        d = np.concatenate([NC._f4([r[1] for r in PLANAR_RAYS]), d])
        t_min = np.concatenate([np.zeros(k, np.float32), t_min])
        t_max = np.concatenate([np.full(k, np.inf, np.float32), t_max])
    return _frozen(v, f, o, d, t_min, t_max)


def cells(verts):
    """the `cell` arguments every mesh is indexed with: the default, one cell, 1/64 of the extent"""
    return NC.cells(verts)


@functools.lru_cache(maxsize=None)
def reference(name, which_pad):
    v, f, o, d, t_min, t_max = case(name)
    return _frozen(*ray_ref(o, d, v, f, pads(v)[which_pad], t_min, t_max))


# ---- spheres ---------------------------------------------------------------------------------------------------
def sphere_entry(o, d, radius):
    """(t, through) in fp64: the entry of the unit-direction rays (o, d) into the sphere of `radius` about the
    origin, and whether the line passes inside it"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    b = (o * d).sum(-1)
    disc = b * b - ((o * o).sum(-1) - radius * radius)
    return -b - np.sqrt(np.maximum(disc, 0.0)), disc > 0


def inner_radius(verts, faces):
    """the smallest distance of a face's plane from the origin, fp64: the sphere inscribed in a convex mesh"""
    tri = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return float(np.abs((n * tri[:, 0]).sum(1) / np.linalg.norm(n, axis=1)).min())
