"""Plain numpy marching cubes driven by the generated case table (scripts/gen_mc_table.py): the reference the HIP
kernels of csrc/hm_mesh.hip are checked against, and the mesh the CPU topology tests inspect.

Same conventions and the same fp32 operations as the kernels (include/hashmod.h, mesh extraction): vertices by owning
lattice point then axis, faces by cell then table order, normals toward increasing values.  Also the mesh checks the
tests share (closed / manifold / oriented, Euler characteristic, signed volume)."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_gen():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "scripts", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _load_gen()
TABLE = gen.table_array()                            # [256, 16] int8
EDGE_CORNER = np.asarray(gen.EDGE_CORNER, np.int64)
EDGE_AXIS = np.asarray(gen.EDGE_AXIS, np.int64)


def _gradient(v, sp, i, j, k):
    """central differences over the spacing, one-sided at the border, at the points (i, j, k) - fp32 as the kernel"""
    n = v.shape
    g = np.empty((len(i), 3), np.float32)
    for a, p in enumerate((i, j, k)):
        lo = np.maximum(p - 1, 0)
        hi = np.minimum(p + 1, n[a] - 1)
        plo = [i, j, k]
        phi = [i, j, k]
        plo[a] = lo
        phi[a] = hi
        g[:, a] = (v[tuple(phi)] - v[tuple(plo)]) / ((hi - lo).astype(np.float32) * sp[a])
    return g


def marching_cubes(volume, level=0.0, spacing=(1.0, 1.0, 1.0)):
    """(verts [V,3] fp32, faces [F,3] int64, normals [V,3] fp32)"""
    v = np.asarray(volume, dtype=np.float32)
    nx, ny, nz = v.shape
    lev = np.float32(level)
    sp = np.asarray(spacing, np.float32)
    inside = v < lev
    cross = np.zeros((nx, ny, nz, 3), bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = cross.reshape(-1)
    vid = np.cumsum(flat, dtype=np.int64) - 1          # vertex id of (point, axis), valid where flat
    idx = np.nonzero(flat)[0]
    p, ax = idx // 3, idx % 3
    i, j, k = np.unravel_index(p, (nx, ny, nz))
    i1, j1, k1 = i + (ax == 0), j + (ax == 1), k + (ax == 2)
    a = v[i, j, k]
    b = v[i1, j1, k1]
    t = (lev - a) / (b - a)
    ijk = np.stack([i, j, k], 1).astype(np.float32)
    rows = np.arange(len(idx))
    ijk[rows, ax] = ijk[rows, ax] + t
    verts = ijk * sp
    g0 = _gradient(v, sp, i, j, k)
    g1 = _gradient(v, sp, i1, j1, k1)
    nn = g0 + t[:, None] * (g1 - g0)
    d = nn[:, 0] * nn[:, 0] + nn[:, 1] * nn[:, 1] + nn[:, 2] * nn[:, 2]
    s = np.sqrt(d)
    with np.errstate(invalid="ignore", divide="ignore"):
        normals = np.where(d[:, None] > 0, nn / s[:, None], np.float32(0)).astype(np.float32)
    # cells
    ins = inside.astype(np.int64)
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c in range(8):
        di, dj, dk = gen.corner_offset(c)
        case |= ins[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk] << c
    ntri = TABLE[case, 0].astype(np.int64)
    cells = np.nonzero(ntri.reshape(-1))[0]
    ci, cj, ck = np.unravel_index(cells, (nx - 1, ny - 1, nz - 1))
    cnt = ntri.reshape(-1)[cells]
    rep = np.repeat(np.arange(len(cells)), cnt)
    tri = np.arange(len(rep)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    cs = case.reshape(-1)[cells][rep]
    faces = np.empty((len(rep), 3), np.int64)
    for m in range(3):
        e = TABLE[cs, 1 + 3 * tri + m].astype(np.int64)
        c = EDGE_CORNER[e]
        q = ((ci[rep] + (c & 1)) * ny + cj[rep] + ((c >> 1) & 1)) * nz + ck[rep] + ((c >> 2) & 1)
        faces[:, m] = vid[q * 3 + EDGE_AXIS[e]]
    return verts.astype(np.float32), faces, normals


# ---- mesh checks -----------------------------------------------------------------------------------------
def edge_check(faces):
    """(every undirected edge in exactly two faces, every directed edge once with its reverse once)"""
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    nv = int(f.max()) + 1 if len(f) else 1
    key = d[:, 0] * nv + d[:, 1]
    rkey = d[:, 1] * nv + d[:, 0]
    uk, ucnt = np.unique(key, return_counts=True)
    directed_once = bool(np.all(ucnt == 1))
    und = np.minimum(key, rkey)
    _, und_cnt = np.unique(und, return_counts=True)
    two_faces = bool(np.all(und_cnt == 2))
    reverse_once = directed_once and bool(np.all(np.isin(rkey, uk)))
    return two_faces, reverse_once


def euler(verts, faces):
    f = np.asarray(faces, np.int64)
    d = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    n_edges = len(np.unique(d[:, 0] * (len(verts) + 1) + d[:, 1]))
    return len(np.unique(f)) - n_edges + len(f)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def read_ply(path):
    """(vertices [V,3] f4, normals [V,3] f4 or None, faces [F,3] i4) of a binary little-endian PLY as TriMesh.export
    writes it (float vertex properties, one list uchar int face property)"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = nf = 0
    props = []
    for line in head:
        w = line.split()
        if w[:2] == ["element", "vertex"]:
            nv = int(w[2])
        elif w[:2] == ["element", "face"]:
            nf = int(w[2])
        elif w[:2] == ["property", "float"]:
            props.append(w[2])
    vert = np.frombuffer(data, np.dtype([(p, "<f4") for p in props]), nv, end)
    face = np.frombuffer(data, np.dtype([("count", "u1"), ("index", "<i4", (3,))]), nf, end + vert.nbytes)
    assert np.all(face["count"] == 3)
    verts = np.stack([vert[p] for p in ("x", "y", "z")], 1)
    normals = np.stack([vert[p] for p in ("nx", "ny", "nz")], 1) if "nx" in props else None
    return verts, normals, face["index"].copy()
