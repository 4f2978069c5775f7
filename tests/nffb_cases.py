"""Case table, point sets and float64 reference of the fused filter-bank embedder tests (test_nffb_cases_cpu.py /
test_nffb_cases_gpu.py; the kernels are csrc/hm_nffb.hip).

No GPU code here: seeded parameters (params.make_nffb_params), the points, the numpy restatement `ref_fwd` of
FourierFilterBanks.forward and the error budget measured on that restatement alone.

The reference.  xn = x / bound and u = (x + bound) / (2 bound) are single correctly rounded fp32 operations, as the
kernel and torch perform them.  The grid row is the C oracle's (oracle/hm_oracle.c), fp32 by definition.  Everything
behind it - the row cut into L chunks of 4, the positional encoding [c, c, sin(c 2^m), cos(c 2^m)], the SIREN trunk
with w0 = L^2 - L, StyleAttention (linear_transform, then the per-row normalisation with biased variance and
eps = 1e-5), the shared out_layer and the mean over L - runs in the requested dtype.

The bound.  Two quantities are measured per case on the reference alone (test_nffb_cases_cpu.py re-derives them):
  A  max |ref_fwd(float32) - ref_fwd(float64)|: what fp32 arithmetic costs whoever performs it;
  B  the response of ref_fwd(float64) to a +-2 ulp perturbation (random signs) of every entry of the oracle's grid
     row: the device sincosf and the host libm may differ by that much, and the positional encoding multiplies the
     difference by up to 2^(L-1).
A kernel's feature columns must lie within MARGIN * (A + B) of ref_fwd(float64); MARGIN = 3 stands for the kernels'
k-ordered fma chains summing in another order than numpy's blocked product, the device sinf of the trunk and the
two kernels rounding differently.  Nothing here is derived from what a kernel returns."""
import collections
import functools

import numpy as np

import params as P
from oracle import c_oracle as O

MODES = {"reference": 0, "trilinear": 1}
STYLES = {False: "FFB", True: "StyleModNFFB"}
# name: (log2_T, base resolution).  T14: level 0 dense with 16^3 = 2^12 rows, level 1 upward hashed into 2^14 rows.
# T12: level 0 dense with 12^3 = 1728 rows (no power of two), level 1 upward hashed into 2^12 rows.  Levels 0 .. L-5
# reach the output, so at L = 6 both consumed levels of T12 are the dense non-power-of-two one and a hashed one.
GRIDS = {"T14": (14, 16), "T12": (12, 12)}
DESIRED = 512
SEED = 11
TABLE_SCALE = 0.3

Case = collections.namedtuple("Case", "L style mode bound grid")

ALL = tuple(Case(L, style, mode, bound, grid) for L in (6, 8) for style in (False, True) for mode in MODES
            for bound in (1.0, 1.5) for grid in GRIDS)
# one plain and one style case per L for the tests that are about batch sizes, not about the configuration
SIZE_CASES = (Case(6, False, "reference", 1.5, "T12"), Case(6, True, "trilinear", 1.0, "T14"),
              Case(8, False, "trilinear", 1.5, "T14"), Case(8, True, "reference", 1.0, "T12"))
STRIDE_CASES = (Case(8, True, "reference", 1.5, "T14"), Case(6, False, "trilinear", 1.0, "T12"))   # MFMA grid-stride

# ---- batch sizes -----------------------------------------------------------------------------------------------
SMALL_MAX = 8192                       # kSmallCount of hm_nffb.hip: up to it the lanes-per-point (VALU) kernel
N_VALU = 3001
N_MFMA = SMALL_MAX + 16 * 3 + 5        # three full 16-point waves and a 5-point tail behind the hand-over
HANDOVER_SIZES = (1, 7, 8, 9, 8191, 8192, 8193, 8192 + 15, 8192 + 16, 8192 + 63, 8192 + 65)
N_POINTS = max(HANDOVER_SIZES)         # one point set (and one reference) per case serves all of the above
N_STRIDE = 2048 * 64 + 16 + 5          # the MFMA launch has at most 2048 workgroups of 64 points
N_STRIDE_TAIL = 16 + 5
N_PERM = 9000

# ---- error budget (module docstring), keyed by (L, style); measured at SEED over ALL ------------------------------
MARGIN = 3.0
RECORD_SLACK = 1.5       # a recorded constant lies in [1, RECORD_SLACK] x the largest fresh measurement of its cases
ERR_A = {(6, False): 7.40e-7, (6, True): 7.45e-7, (8, False): 1.60e-6, (8, True): 1.48e-6}
ERR_B = {(6, False): 1.12e-6, (6, True): 1.59e-6, (8, False): 3.38e-6, (8, True): 5.13e-6}
PERTURB_ULPS = 2


def case_id(c):
    return f"L{c.L}-{STYLES[c.style]}-{c.mode}-b{c.bound}-{c.grid}"


def width(c):
    return 3 + 8 + 8 * c.L


def bound_of(c):
    """absolute bound of a kernel's feature columns against ref_fwd(float64)"""
    k = (c.L, c.style)
    return MARGIN * (ERR_A[k] + ERR_B[k])


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def grid(c):
    log2_T, base = GRIDS[c.grid]
    return O.Grid(c.L, log2_T, base, DESIRED)


@functools.lru_cache(maxsize=None)
def params(c):
    """make_nffb_params of the case (read-only arrays), keyed as the state_dict of Custom_Embedding_Network.embedder_obj"""
    log2_T, base = GRIDS[c.grid]
    p = P.make_nffb_params(SEED, c.L, c.style, TABLE_SCALE, log2_T=log2_T, base=base, desired=DESIRED)
    return {k: _frozen(v) for k, v in p.items()}


def consumed_levels(c):
    """levels whose features reach the output: chunks 0 .. L-3 of the row [sin(L) | cos(L) | L x 2 features]"""
    return range(c.L - 4)


def rerandomised_dead_levels(c, seed=23):
    """params(c) with the table rows of levels L-4 and above drawn again"""
    rs = np.random.RandomState(seed)
    p = dict(params(c))
    for l in range(c.L - 4, c.L):
        k = f"grid_enc.levels.{l}.embedding.weight"
        p[k] = rs.uniform(-TABLE_SCALE, TABLE_SCALE, p[k].shape).astype(np.float32)
    return p


def adversarial_tail(c):
    """params.adversarial_points(res) as they are (+-1, |x| up to 3, +-0), preceded by the same points mapped by
    x = (2 a - 1) bound, which puts u = (x + bound) / (2 bound) on or next to the voxel faces a = k / res of every
    level (those that stay within |x| <= 3)"""
    b = np.float32(c.bound)
    adv = P.adversarial_points([int(r) for r in grid(c).res])
    mapped = ((np.float32(2) * adv - np.float32(1)) * b).astype(np.float32)
    return np.concatenate([mapped[np.abs(mapped).max(1) <= 3.0], adv], 0)


def n_adversarial(c, n=N_POINTS):
    return min(len(adversarial_tail(c)), n // 2)


@functools.lru_cache(maxsize=None)
def points(c, n=N_POINTS):
    """[n,3] fp32, read-only: uniform in [-1.3, 1.3]^3 * bound with adversarial_tail(c) at the end.  Same points for
    every style and frac_mode."""
    rs = np.random.RandomState(1000 * c.L + 10 * int(round(c.bound * 10)) + GRIDS[c.grid][0] + n)
    x = (rs.uniform(-1.3, 1.3, (n, 3)).astype(np.float32) * np.float32(c.bound)).astype(np.float32)
    tail = adversarial_tail(c)
    k = n_adversarial(c, n)
    if k:
        x[n - k:] = tail[len(tail) - k:]
    return _frozen(x)


def inputs_fp32(c, x):
    """(xn, u) as the kernel forms them: one correctly rounded fp32 operation each"""
    x = np.ascontiguousarray(x, np.float32)
    b = np.float32(c.bound)
    return (x / b).astype(np.float32), ((x + b) / (np.float32(2) * b)).astype(np.float32)


def table_of(p, L):
    return np.concatenate([p[f"grid_enc.levels.{l}.embedding.weight"] for l in range(L)], 0)


def grid_row(c, u, p=None, g=None):
    """[N, 4L] fp32: the C oracle's embedding row of u without its 3 pass-through columns"""
    p = params(c) if p is None else p
    g = grid(c) if g is None else g
    return O.encode_fwd(g, u, table_of(p, c.L), p["grid_enc.freq_encoding.B"], MODES[c.mode])[:, 3:]


def grid_row_two_pi(c, u, two_pi, p=None, g=None):
    """the row with its Fourier arguments formed from s = fl32(two_pi * u), two_pi a float64, instead of the kernel's
    s = fl32(fl32(2 pi) * u) (mutations only).  two_pi = numpy.pi is the mutation of the issue ('two_pi taken as
    float64 pi': the factor 2 lost); two_pi = 2 * numpy.pi changes the argument by at most one fp32 step, which the
    budget B allows by construction - no bound of this kind can tell it from the kernel's form."""
    p = params(c) if p is None else p
    row = grid_row(c, u, p, g).copy()
    B = p["grid_enc.freq_encoding.B"].astype(np.float64)
    s = (two_pi * u.astype(np.float64)).astype(np.float32).astype(np.float64)
    a = (s[:, 0:1] * B[0:1]).astype(np.float32).astype(np.float64)     # the oracle's k-ordered chain, each step rounded
    a = (a + s[:, 1:2] * B[1:2]).astype(np.float32).astype(np.float64)  # to fp32; with the kernel's two_pi the result
    a = (a + s[:, 2:3] * B[2:3]).astype(np.float32)                     # is within one fp32 step of the oracle's row
    row[:, :c.L], row[:, c.L:2 * c.L] = np.sin(a), np.cos(a)            # (numpy's fp32 sin / cos, not libm's)
    return row


def perturbed(row, ulps=PERTURB_ULPS, seed=7):
    """every entry moved by `ulps` fp32 steps, up or down at random"""
    up = np.random.RandomState(seed).randint(0, 2, row.shape).astype(bool)
    to = np.where(up, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    out = row.astype(np.float32)
    for _ in range(ulps):
        out = np.nextafter(out, to)
    return out


MUTATIONS = ("sincos_swap", "chunk_off_by_one", "unbiased_variance", "no_mean_over_L", "no_trunk_add", "two_pi_f64")


def forward(c, p, xn, u, row, dtype, mutation=None):
    """[N, 3 + 8 + 8L] in `dtype` from the fp32 inputs xn, u and the fp32 grid row (module docstring)"""
    dt = np.dtype(dtype).type
    L, W = c.L, 8 + 8 * c.L
    n = xn.shape[0]

    def lin(v, name):
        return v @ p[name + ".weight"].astype(dt).T + p[name + ".bias"].astype(dt)

    chunks = row.astype(dt).reshape(n, L, 4)
    w0 = dt(L * L - L)
    h = xn.astype(dt)
    feats = np.zeros((n, W), dt)
    for layer in range(L - 1):
        h = np.sin(w0 * lin(h, f"ff_lin{layer}"))
        if layer == 0:
            continue
        ch = chunks[:, layer if mutation == "chunk_off_by_one" else layer - 1]
        parts = [ch, ch]
        for m in range(L):
            arg = ch * dt(2 ** m)
            sc = [np.sin(arg), np.cos(arg)]
            parts += sc[::-1] if (mutation == "sincos_swap" and m == 1) else sc
        e = np.concatenate(parts, 1)
        assert e.shape == (n, W) and e.dtype == dt
        if c.style:
            y = lin(e, "StyleAttentionBlock.linear_transform")
            mean = y.mean(1, keepdims=True)
            d = y - mean
            var = (d * d).sum(1, keepdims=True) / dt(W - 1 if mutation == "unbiased_variance" else W)
            e = d / np.sqrt(var + dt(1e-5))
        if mutation != "no_trunk_add":
            e = e + h
        feats = feats + lin(e, "out_layer")
    if mutation != "no_mean_over_L":
        feats = feats / dt(L)
    out = np.concatenate([u.astype(dt), feats], 1)
    assert out.dtype == dt
    return out


def ref_fwd(c, x, dtype=np.float64, p=None, mutation=None, g=None):
    """the embedding rows of the points x [N,3] (not cached; `p` replaces the case's parameters, `g` its level table)"""
    assert mutation is None or mutation in MUTATIONS
    p = params(c) if p is None else p
    xn, u = inputs_fp32(c, x)
    row = grid_row_two_pi(c, u, np.pi, p, g) if mutation == "two_pi_f64" else grid_row(c, u, p, g)
    return forward(c, p, xn, u, row, dtype, mutation)


@functools.lru_cache(maxsize=None)
def reference(c, n=N_POINTS):
    """ref_fwd(float64) on points(c, n): computed once, shared, read-only"""
    return _frozen(ref_fwd(c, points(c, n)))


@functools.lru_cache(maxsize=None)
def measure(c):
    """(A, B, output scale) of the case on points(c): see the module docstring"""
    x = points(c)
    xn, u = inputs_fp32(c, x)
    row = grid_row(c, u)
    r64 = reference(c)
    a = np.abs(forward(c, params(c), xn, u, row, np.float32).astype(np.float64) - r64)[:, 3:].max()
    b = np.abs(forward(c, params(c), xn, u, perturbed(row), np.float64) - r64)[:, 3:].max()
    return float(a), float(b), float(np.abs(r64[:, 3:]).max())
