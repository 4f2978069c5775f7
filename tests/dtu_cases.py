"""Shared inputs of the DTU-evaluation tests (numpy only) and the numpy restatements that serve as the references of
csrc/hm_nn_radius.hip and csrc/hm_dtu_filter.hip:

  downsample_ref(points, radius)       the reference's sequential loop over fp32-exact radius neighbourhoods
  flags_ref(points, mask, bb, ...)     the three filter bits in fp64
  dtu_ref(...)                         the whole pipeline, with cKDTree distances

Everything is computed once and read-only."""
import functools

import numpy as np

import nn_cases as NC


def radius2_f32(radius):
    r = np.float32(radius)
    return r * r


def neighbour_lists(points, radius):
    """for every point the ascending indices j (itself included) with the fp32 value (dx*dx + dy*dy) + dz*dz <=
    fp32(radius)^2: candidates from a cKDTree at a slightly larger radius, filtered by the fp32 expression"""
    from scipy.spatial import cKDTree
    p = NC._f4(points)
    r2 = radius2_f32(radius)
    cand = cKDTree(p.astype(np.float64)).query_ball_point(p.astype(np.float64), float(np.float32(radius)) * (1 + 1e-5))
    out = []
    for i, c in enumerate(cand):
        c = np.sort(np.asarray(c, np.int64))
        d = p[i][None, :] - p[c]
        d *= d
        v = (d[:, 0] + d[:, 1]) + d[:, 2]
        assert v.dtype == np.float32
        out.append(c[v <= r2])
    return out


def greedy_loop(nb, n):
    """mask = ones; for curr in order: if mask[curr]: mask[nb[curr]] = 0; mask[curr] = 1"""
    mask = np.ones(n, bool)
    for curr in range(n):
        if mask[curr]:
            mask[nb[curr]] = False
            mask[curr] = True
    return mask


def downsample_ref(points, radius):
    """keep [n] bool of DTU's greedy radius down-sampling in index order"""
    p = NC._f4(points)
    return greedy_loop(neighbour_lists(p, radius), len(p))


def flags_ref(points, mask, bb, res, patch, plane):
    """uint8 [n]: bit 0 inbound, bit 1 in the observation mask, bit 2 above the plane; 0 for a non-finite row"""
    p32 = NC._f4(points)
    finite = np.isfinite(p32).all(1)
    p = np.where(finite[:, None], p32, np.float32(0)).astype(np.float64)
    bb = np.asarray(bb, np.float64)
    P = np.asarray(plane, np.float64).reshape(4)
    shape = np.asarray(mask.shape)
    inbound = (p >= bb[0] - patch).all(1) & (p < bb[1] + patch * 2).all(1)
    k = np.around((p - bb[0]) / np.float64(res))
    inside = ((k >= 0) & (k < shape)).all(1)
    ki = np.where(inside[:, None], k, 0).astype(np.int64)
    in_obs = inside & (mask[ki[:, 0], ki[:, 1], ki[:, 2]] != 0)
    above = ((P[0] * p[:, 0] + P[1] * p[:, 1]) + P[2] * p[:, 2]) + P[3] > 0
    f = inbound.astype(np.uint8) | (in_obs.astype(np.uint8) << 1) | (above.astype(np.uint8) << 2)
    return np.where(finite, f, 0).astype(np.uint8)


def _mean_below(d, max_dist):
    k = d < max_dist
    return (d[k].mean() if k.any() else np.nan), int(k.sum())


def dtu_ref(verts, faces, stl, order, mask, bb, res, plane, density, patch, max_dist):
    """dict of the pipeline's results (and the two distance arrays d2s, s2d) as the reference computes them"""
    v = np.asarray(verts, np.float32)
    data = np.concatenate([v, NC.sample_ref(v, faces, density)[0]])[order]
    keep = downsample_ref(data, density)
    down = data[keep]
    fl = flags_ref(down, mask, bb, res, patch, plane)
    data_in = down[(fl & 1) != 0]
    in_obs = down[(fl & 3) == 3]
    above = (flags_ref(stl, mask, bb, res, patch, plane) & 4) != 0
    d2s = NC.one_sided_ref(in_obs, stl)
    s2d = NC.one_sided_ref(stl[above], data_in)
    acc, n_d2s = _mean_below(d2s, max_dist)
    comp, n_s2d = _mean_below(s2d, max_dist)
    return {"accuracy": acc, "completeness": comp, "overall": 0.5 * (acc + comp), "n_cloud": len(data),
            "n_down": len(down), "n_in": len(data_in), "n_in_obs": len(in_obs), "n_stl_above": int(above.sum()),
            "n_d2s": n_d2s, "n_s2d": n_s2d, "d2s": d2s, "s2d": s2d}


# ---- clouds for the thinning ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sphere(order, n=20000):
    """n seeded points of the unit sphere, "shuffled" (as drawn) or "swept" (by latitude band of 0.02, then angle)"""
    rng = np.random.default_rng(11)
    p = rng.standard_normal((n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    if order == "swept":
        band = np.floor((p[:, 2] + 1.0) / 0.02)
        p = p[np.lexsort((np.arctan2(p[:, 1], p[:, 0]), band))]
    elif order != "shuffled":
        raise KeyError(order)
    return NC._frozen(NC._f4(p))[0]


def line(n=1025, spacing=0.6):
    """points on the x axis in index order: with radius 1 each point's only neighbours are the two next to it"""
    p = np.zeros((n, 3), np.float32)
    p[:, 0] = np.arange(n, dtype=np.float32) * np.float32(spacing)
    return p


@functools.lru_cache(maxsize=None)
def reference(name, radius):
    """downsample_ref of a named cloud, computed once"""
    if name.startswith("sphere_"):
        p = sphere(name.split("_", 1)[1])
    elif name == "line":
        p = line()
    elif name == "line_reversed":
        p = line()[::-1]
    elif name == "lattice":
        p = NC.lattice()
    else:
        p = NC.cloud(name)[0]
    return NC._frozen(downsample_ref(p, radius))[0]


# ---- volumes and points for the flags ----------------------------------------------------------------------------
FLAG_CASES = {
    # shape, bb, res, patch, plane: the arithmetic at the boundaries below is exact in fp32 and fp64
    "5x7x3": ((5, 7, 3), [[-1.0, 2.0, 0.5], [1.0, 5.0, 1.5]], 0.5, 0.25, [0.5, -1.0, 2.0, 0.25]),
    "4x4x4": ((4, 4, 4), [[0.0, 0.0, 0.0], [3.0, 3.0, 3.0]], 1.0, 2.0, [0.0, 0.0, 1.0, -1.5]),
}


@functools.lru_cache(maxsize=None)
def flag_volume(name):
    shape = FLAG_CASES[name][0]
    rng = np.random.default_rng(sum(map(ord, name)))
    return NC._frozen((rng.random(shape) < 0.6).astype(np.uint8))[0]


def flag_boundary_points(name):
    """points exactly at every boundary the filters have, then one +inf, one -inf and one NaN row"""
    shape, bb, res, patch, plane = FLAG_CASES[name]
    bb = np.asarray(bb, np.float64)
    mid = (bb[0] + bb[1]) / 2
    rows = []
    for a in range(3):
        for value in (bb[0][a] - patch,                         # inclusive lower bound
                      np.nextafter(np.float32(bb[0][a] - patch), np.float32(-np.inf)),
                      bb[1][a] + 2 * patch,                     # exclusive upper bound
                      np.nextafter(np.float32(bb[1][a] + 2 * patch), np.float32(-np.inf)),
                      bb[0][a] + 0.5 * res,                     # k + 0.5, k = 0 (even): rounds to 0
                      bb[0][a] + 1.5 * res,                     # k = 1 (odd): rounds to 2
                      bb[0][a] + 2.5 * res,                     # k = 2: rounds to 2
                      bb[0][a] - 0.5 * res,                     # -0.5 rounds to -0: index 0
                      bb[0][a] - 0.75 * res,                    # index -1
                      bb[0][a] - 1.0 * res,                     # index -1 exactly
                      bb[0][a] + (shape[a] - 0.5) * res,        # shape - 0.5: to shape (odd shape - 1) or shape - 1
                      bb[0][a] + shape[a] * res,                # index == shape
                      bb[0][a] + (shape[a] - 1) * res,          # the last index
                      1e30, -1e30):                             # far beyond int32 and int64 after the division
            row = mid.copy()
            row[a] = value
            rows.append(row)
    P = np.asarray(plane, np.float64)
    a = int(np.argmax(np.abs(P[:3])))
    for eps in (0.0, 1.0, -1.0):                                # plane value exactly 0, then just either side
        row = mid.copy()
        row[a] = 0.0
        row[a] = -(P[:3] @ row + P[3]) / P[a]
        if eps:
            row[a] = np.nextafter(np.float32(row[a]), np.float32(eps * np.inf * np.sign(P[a])))
        rows.append(row)
    rows += [[np.inf, mid[1], mid[2]], [mid[0], -np.inf, mid[2]], [mid[0], mid[1], np.nan]]
    return NC._f4(np.asarray(rows, np.float64))


def flag_points(name, n):
    """n points: the boundary points first (as many as fit), then seeded points in and around the padded box"""
    shape, bb, res, patch, plane = FLAG_CASES[name]
    bb = np.asarray(bb, np.float64)
    edge = flag_boundary_points(name)[:n]
    rng = np.random.default_rng(n)
    lo, hi = bb[0] - 2 * patch - res, bb[1] + 3 * patch + res
    fill = lo + (hi - lo) * rng.random((n - len(edge), 3))
    return NC._f4(np.concatenate([edge, fill]))


# ---- the end-to-end case ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dtu_case():
    """an icosphere of radius 10 against a perturbed scan, a mask volume that misses part of the sphere, a plane that
    cuts the lower cap: every stage removes something and keeps something"""
    verts, faces = NC.icosphere()
    verts = NC._f4(verts.astype(np.float64) * 10.0)
    stl = NC.perturbed_target(verts, 20000, 0.3)
    density, patch, max_dist, res = 0.2, 2.0, 0.6, 1.0
    bb = np.array([[-11.0, -11.0, -11.0], [3.0, 11.0, 11.0]])      # x >= 7 is out of bounds, x >= 3.5 beyond the volume
    shape = (15, 23, 23)
    ax = [bb[0][a] + res * np.arange(shape[a]) for a in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    mask = ((Y < 4.0) & (X * X + Y * Y + Z * Z < 12.0 ** 2)).astype(np.uint8)   # the +y side is unobserved
    plane = np.array([0.0, 0.0, 1.0, 7.0])                        # z > -7
    n_cloud = len(verts) + len(NC.sample_ref(verts, faces, density)[0])
    order = np.random.default_rng(3).permutation(n_cloud)
    case = dict(verts=verts, faces=faces, stl=stl, density=density, patch=patch, max_dist=max_dist, res=res, bb=bb,
                mask=np.ascontiguousarray(mask), plane=plane, order=order)
    NC._frozen(verts, stl, bb, case["mask"], plane, order)
    return case


@functools.lru_cache(maxsize=None)
def dtu_case_reference():
    c = dtu_case()
    return dtu_ref(c["verts"], c["faces"], c["stl"], c["order"], c["mask"], c["bb"], c["res"], c["plane"], c["density"],
                   c["patch"], c["max_dist"])
