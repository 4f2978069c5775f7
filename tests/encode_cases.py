"""Case table and reference helpers of the grid-encoder tests (test_encode_cases_cpu.py / test_encode_cases_gpu.py).

No GPU code here: level tables, point sets, seeded inputs, the C oracle's results (cached, read-only) and the float64
torch restatements whose autograd supplies the first / second order references.

Exact inputs.  The `lattice` points are x = m / 16 with integer m, so x * res is exact in fp32 for every res used here
and every trilinear weight is a multiple of 2^-12.  With integer table entries (forward) or integer d_feat (scatter)
every term is then a multiple of 2^-12, and as long as the sum of the terms' magnitudes stays below 2^12 in every cell
(2^24 in reference mode, where the weights are 0 / 1) every partial sum in ANY order is exactly representable in fp32:
a kernel can be compared with the oracle by array_equal, in trilinear mode and through atomics too.  The bound is
checked with the oracle for every case and mode (test_encode_cases_cpu.py), not assumed."""
import functools
import math

import numpy as np
import torch

import params as P
from oracle import c_oracle as O

MODES = {"reference": 0, "trilinear": 1}
N_BIG = 131072 + 37          # a big-launch kernel is the subject
N_BELOW = 131071             # its just-below neighbour (the tile kernel on the same table)
N_SMALL = 3001
BIG_TABLE_BYTES = 8 << 20    # tables above it take the sweep / z-ordered kernels (n >= 131072)
SMALL_TABLE_ROWS = 4096      # tables up to it (and up to SMALL_TABLE_LDS bytes) take the LDS-privatised scatter
SMALL_TABLE_LDS = 48 * 1024


class Grid:
    """level table from explicit res / rows lists: the attributes oracle.c_oracle.encode_fwd / encode_bwd_table and
    _trilinear_torch read (c_oracle.Grid only builds level_table() grids with L >= 2)"""

    def __init__(self, res, rows, F):
        assert len(res) == len(rows) >= 1
        self.L, self.F = len(res), int(F)
        self.res = np.asarray(res, np.int32)
        self.rows = np.asarray(rows, np.uint32)
        self.row_off = np.concatenate([[0], np.cumsum(self.rows.astype(np.uint64))]).astype(np.uint64)
        self.total_rows = int(self.row_off[-1])
        self.E = 3 + 2 * self.L + self.L * self.F

    @property
    def table_bytes(self):
        return self.total_rows * self.F * 4


def _lt(L, T, b, d):
    return P.level_table(L, T, b, d)


# name: (res, rows, F, what the case is for)
CASES = {
    "Z1": ([160], [2 ** 21], 2, "z-order, sweep, z-order bwd; L = 1"),
    "Z3": ([16, 90, 301], [4096, 729000, 2 ** 19], 2, "odd L; dense non-pow2 level at res 90"),
    "Z15": (*_lt(15, 17, 16, 2048), 2, "odd L; res up to 2048 (outside the 2^11 window)"),
    "Z17": (*_lt(17, 17, 8, 512), 2, "LF = 34: second pack chunk with cw = 2"),
    "Z32": (*_lt(32, 16, 4, 512), 2, "HM_MAX_LEVELS; LDS and row-store limits"),
    "S_F1": ([3, 16], [27, 4069], 1, "hashed non-pow2 rows; small-table scatter"),
    "S_F3": ([1, 2, 5, 7], [1, 8, 125, 343], 3, "res = 1, rows = 1; small-table scatter"),
    "S_F3_edge": ([64], [4096], 3, "total_rows*F*4 == 48 KiB exactly (LDS path)"),
    "S_F4_over": ([64], [4096], 4, "same rows, 64 KiB: falls to the atomic kernel"),
    "G_F4": (*_lt(5, 12, 4, 64), 4, "generic forward, atomic scatter"),
    "G_F8": ([4, 9, 33], [64, 729, 4096], 8, "F maximum (acc[8])"),
    "T_F2": ([4, 9, 33], [64, 729, 4096], 2, "tile kernel on a hand-made table, for the stride tests"),
    "DX_F2": ([8, 20, 48], [512, 1024, 1024], 2, "3 hashed levels, F = 2: input-gradient kernels against torch"),
}
Z_CASES = ("Z1", "Z3", "Z15", "Z17", "Z32")
SMALL_SCATTER = ("S_F1", "S_F3", "S_F3_edge")              # encode_bwd_table_small_kernel once n*L*C >= 4096
ATOMIC_SCATTER = ("S_F4_over", "G_F4", "G_F8")             # encode_bwd_table_kernel at every n
FN_CASES = SMALL_SCATTER + ATOMIC_SCATTER                  # F != 2
DX_CASES = ("G_F4", "S_F3", "G_F8", "T_F2", "DX_F2")


@functools.lru_cache(maxsize=None)
def grid(name):
    res, rows, F, _ = CASES[name]
    return Grid(res, rows, F)


def fn_sizes(name):
    """point counts of the F != 2 cases: 1 and 7 stay below the small-table kernel's n * L * C >= 4096 in both modes,
    the last one is above it in both (a one-level table needs n >= 4096 in reference mode, where C = 1)"""
    return (1, 7, N_SMALL) + ((4099,) if grid(name).L == 1 else ())


def small_scatter_taken(name, n, mode):
    """the host rule of hm_encode_bwd_table for encode_bwd_table_small_kernel"""
    g = grid(name)
    return (g.total_rows <= SMALL_TABLE_ROWS and g.table_bytes <= SMALL_TABLE_LDS
            and n * g.L * (1 if mode == "reference" else 8) >= 4096)


def default_n(name):
    return N_BIG if name in Z_CASES else N_SMALL


def _seed(name, *extra):
    s = sum((i + 1) * ord(ch) for i, ch in enumerate(name))
    for e in extra:
        s = s * 31 + int(e)
    return s % (2 ** 31 - 1)


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- point sets ------------------------------------------------------------------------------------------------
LATTICE_NODES = np.asarray([(0, 0, 0), (1, 1, 1), (-1, -1, -1), (1, -1, 0), (-1, 0, 1)], np.float32)


@functools.lru_cache(maxsize=None)
def points(name, kind, n):
    """[n,3] fp32, read-only.  'real': uniform in [-1.3, 1.3]^3 with the fixed rows the encoder tests add (duplicated
    points, (+-1, -+1, +-1)) and params.adversarial_points(res) at the end; 'lattice': x = m / 16, integer m uniform in
    [-21, 21], a few nodes common to every res in front."""
    g = grid(name)
    rs = np.random.RandomState(_seed(name, n, kind == "real"))
    if kind == "real":
        x = rs.uniform(-1.3, 1.3, (n, 3)).astype(np.float32)
        if n >= 5000:
            x[3000:5000] = x[:2000]
        if n >= 9:
            x[7] = (1.0, -1.0, 1.0)
            x[8] = (-1.0, 1.0, -1.0)
        adv = P.adversarial_points([int(r) for r in g.res])
        k = min(len(adv), n // 2)
        if k:
            x[n - k:] = adv[:k]
    elif kind == "lattice":
        x = (rs.randint(-21, 22, (n, 3)) / 16.0).astype(np.float32)
        if n >= 16:
            x[:len(LATTICE_NODES)] = LATTICE_NODES
    else:
        raise KeyError(kind)
    return _frozen(x)


# ---- tables, Fourier matrix, upstream gradients ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(name, exact):
    g = grid(name)
    rs = np.random.RandomState(_seed(name, 101, exact))
    if exact:
        t = rs.randint(-8, 9, (g.total_rows, g.F)).astype(np.float32)
    else:
        t = rs.uniform(-0.5, 0.5, (g.total_rows, g.F)).astype(np.float32)
    return _frozen(t)


@functools.lru_cache(maxsize=None)
def fourier_B(L, seed=3):
    return _frozen(P.make_fourier_B(seed, L, P.fourier_sigma(16, 512)))


@functools.lru_cache(maxsize=8)
def d_feat(name, kind, n, mode):
    """[n, L*F] fp32, read-only.  lattice: integers, {-1, 0, 1} in trilinear mode and [-8, 8] in reference mode;
    real: standard normal"""
    g = grid(name)
    rs = np.random.RandomState(_seed(name, 202, n, MODES[mode], kind == "real"))
    if kind == "lattice":
        lo, hi = (-1, 2) if mode == "trilinear" else (-8, 9)
        d = rs.randint(lo, hi, (n, g.L * g.F)).astype(np.float32)
    else:
        d = rs.standard_normal((n, g.L * g.F)).astype(np.float32)
    return _frozen(d)


def as_d_out(g, d):
    """the [n, E] upstream gradient the oracle's scatter takes: d in the hash columns, zero elsewhere"""
    d_out = np.zeros((d.shape[0], g.E), np.float32)
    d_out[:, 3 + 2 * g.L:] = d
    return d_out


# ---- the oracle's results (computed once, shared, read-only) ---------------------------------------------------
@functools.lru_cache(maxsize=6)
def oracle_fwd(name, kind, n, mode):
    """[n, E] rows of the C oracle: lattice points go with the integer table, real points with the uniform one"""
    g = grid(name)
    return _frozen(O.encode_fwd(g, points(name, kind, n), table(name, kind == "lattice"), fourier_B(g.L), MODES[mode]))


def scatter(name, x, d, mode):
    g = grid(name)
    return O.encode_bwd_table(g, x, as_d_out(g, d), MODES[mode])


@functools.lru_cache(maxsize=8)
def oracle_scatter(name, kind, n, mode):
    return _frozen(scatter(name, points(name, kind, n), d_feat(name, kind, n, mode), mode))


def exact_bound(mode):
    """what the scatter of |d_feat| must stay below in every cell for order-independent fp32 sums (module docstring)"""
    return float(2 ** 12 if mode == "trilinear" else 2 ** 24)


# ---- float64 torch restatements --------------------------------------------------------------------------------
def _trilinear_torch(x, table, desc):
    """differentiable torch restatement of the trilinear encoder (fp64): floor voxel, 8 hashed corners, product
    weights - the opt-in mode has no counterpart in the reference, so autograd on this expression is the checker"""
    feats = []
    xd = x.double()
    for l in range(desc.L):
        r, rows, off = int(desc.res[l]), int(desc.rows[l]), int(desc.row_off[l])
        xs = (x.detach() * float(r)).double()              # value: the kernel forms x * res in fp32
        xs = xs + (xd * float(r) - (xd * float(r)).detach())   # gradient: of the exact product
        fl = torch.floor(xs.detach())
        t = xs - fl
        acc = 0.0
        for c in range(8):
            w, h = 1.0, None
            for d, prime in enumerate((1, 3, 2654435761)):
                bit = (c >> d) & 1
                w = w * (t[:, d] if bit else 1.0 - t[:, d])
                u = ((fl[:, d].long() + bit) & 0xFFFFFFFF) * prime & 0xFFFFFFFF
                h = u if h is None else h ^ u
            acc = acc + w[:, None] * table[off + (h % rows)].double()
        feats.append(acc)
    return torch.cat(feats, 1)


def fourier_row_torch(x, B):
    """[x | sin(2 pi x B) | cos(2 pi x B)] in float64 (frequency_enc.py:63-67): autograd on it is the reference of
    hm_fourier_bwd_input (first order) and hm_fourier_bwd_input_bwd (second order)"""
    xd = x.double()
    a = (2.0 * math.pi) * (xd @ B.double())
    return torch.cat([xd, torch.sin(a), torch.cos(a)], 1)
