"""Case tables, inputs and float64 references of the autograd nodes of hashmodnffbanks_idr_amd/mlp_grad.py (_SdfMlp,
_SdfMlpRows, _ReluMlp) under frozen-parameter masks, shared by tests/test_mlp_grad_cases_cpu.py (the references and the
conditioning of every case, on the CPU) and tests/test_mlp_grad_masks_gpu.py (the nodes against them).  Import-only: no
test lives here.

The nodes run no arithmetic of their own: they hand saved activations and cotangents to kernels that have bit-level tests.
What can go wrong is the orchestration - which layers' weight gradients are one stacked product over 2N rows, which GEMM
epilogue writes into which half of a stack buffer, which copy is skipped, what two nodes hand each other - and every such
decision hangs on which inputs require a gradient.  So the cases are (network, batch, mask, loss), the reference knows
nothing of mlp_grad.py (plain torch layers and autograd, written for any dtype), and because a gradient with respect to a
subset of the leaves is the subset of all gradients there is ONE reference per (network, rows, loss) whatever the mask.

Tolerance: elem_cases.limit / elem_cases.compare unchanged - |got - ref64| <= min(4 e32 + 2^-22 scale, 2e-5 scale) per
tensor, e32 = max |torch's fp32 evaluation of the same expression - ref64|, scale = max |ref64|.

predicted_products() states, from the layer shapes, the mask, the rows and the merge flag alone, the weight-gradient
products one backward pass hands to gemm_group_tn / gemm_group_tn_add; the GPU test compares it with what it records,
which is how it shows that a mask reached the arm it was written for.
"""
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from elem_cases import CAP, F32, F64, _gen, errors, f32, limit

BETA_SP, THR_SP, BETA_RHO = 100.0, 20.0, 0.1        # the model's values

# ---- networks --------------------------------------------------------------------------------------------------------
Net = namedtuple("Net", "name E dims skip")         # dims: (out, in) per layer; skip: the layer that reads cat[h, e], or -1
NETS = {n.name: n for n in (
    Net("skip2", 27, ((64, 27), (37, 64), (64, 64), (64, 64), (9, 64)), 2),     # odd width 37, concatenated v-bar
    Net("depth0", 27, ((9, 27),), -1),                                          # L = 1: no stack, no u, rank-1 g_e
    Net("depth1", 11, ((33, 11), (5, 33)), -1),                                 # L = 2: l = 0 is first and L - 2
    Net("skip_last", 19, ((48, 19), (29, 48), (3, 48)), 2),                     # the skip is the last layer
    Net("skip1", 19, ((13, 19), (40, 32), (1, 40)), 1),                         # layer 0 feeds the concat; 1 output
)}
BATCHES = (1, 7, 33, 64, 130)       # odd and below a GEMM tile | K = 2N = 128: the grouped kernel | K = 260: the plain GEMM
LOSSES = ("out", "ge", "both", "sum")

# ---- masks -----------------------------------------------------------------------------------------------------------
Mask = namedtuple("Mask", "e w b")                  # which inputs require a gradient: bool, tuple per layer, tuple per layer


def _mask_table(L, skip):
    every, none = (True,) * L, (False,) * L
    only = lambda live: tuple(l in live for l in range(L))          # noqa: E731
    table = [
        ("all", Mask(True, every, every)),
        ("w_none", Mask(True, none, every)),
        ("w_even_frozen", Mask(True, only(set(range(1, L, 2))), every)),        # skip2: {0, 2, 4} frozen
        ("w_odd_frozen", Mask(True, only(set(range(0, L, 2))), every)),         # skip2: {1, 3} frozen
        ("w_skip_frozen", Mask(True, only(set(range(L)) - {skip}), every) if skip >= 0 else None),
        ("w_last_frozen", Mask(True, only(set(range(L - 1))), every)),
        ("w_last_only", Mask(True, only({L - 1}), every)),
        ("b_none", Mask(True, every, none)),
        ("b_ends_frozen", Mask(True, every, only(set(range(1, L - 1))))),
        ("e_off", Mask(False, every, every)),
        ("e_only", Mask(True, none, none)),
    ]
    return table


def masks(net):
    """{name: Mask} of the masks that exist for the network (one that coincides with an earlier one is left out)"""
    out = {}
    for name, m in _mask_table(len(net.dims), net.skip):
        if m is not None and m not in out.values():
            out[name] = m
    return out


LOSS_SWEEP_MASKS = ("all", "w_none", "e_off", "e_only")


def single_pairs(net):
    """the (mask name, loss) pairs of the single-node test: skip2 takes the full cross; the other networks run every
    mask under the loss with both cotangents and every loss under the masks whose arms depend on the cotangents (all on,
    no weight gradient, no input gradient, nothing but the input gradient)"""
    ms = masks(net)
    if net.name == "skip2":
        return [(m, lo) for m in ms for lo in LOSSES]
    return [(m, "both") for m in ms] + [(m, lo) for m in LOSS_SWEEP_MASKS if m in ms for lo in LOSSES if lo != "both"]


# ---- the two-node arrangement ----------------------------------------------------------------------------------------
PAIR_NET = "skip2"
PAIR_ROWS = (            # (n_eik, n_ray, row0, n): the batch has n_eik + n_ray rows, the row node covers [row0, row0 + n)
    (8, 24, 8, 24),      # the case of tests/test_wgrad_once_gpu.py
    (5, 9, 5, 9),        # odd row0, odd n, odd widths: operand pointers that are only 4-byte aligned; K = 28
    (3, 13, 1, 7),
    (0, 16, 0, 16),      # the row node covers the whole batch
    (12, 20, 31, 1),     # n = 1 on the last row
    (16, 48, 16, 48),    # K = 128, row0 % 4 == 0: the kernel takes the addends
    (16, 48, 18, 46),    # K = 128, row0 % 4 != 0: the addend is added to a copy beforehand
)
MISALIGNED_ROWS = ((5, 9, 5, 9), (3, 13, 1, 7))
PAIR_LOSS = "both"


def pair_masks(net):
    """{name: (owner's Mask, row node's Mask)}"""
    L = len(net.dims)
    every, none = (True,) * L, (False,) * L
    but = lambda l: tuple(k != l for k in range(L))                 # noqa: E731
    return {
        "all": (Mask(True, every, every), Mask(True, every, every)),
        "w2_frozen": (Mask(True, but(2), every), Mask(True, but(2), every)),
        "w1_frozen_on_rows": (Mask(True, every, every), Mask(True, but(1), every)),     # the owner adds the sums up
        "b_none": (Mask(True, every, none), Mask(True, every, none)),
    }


# ---- predicted weight-gradient products ------------------------------------------------------------------------------
def _owner_products(dims, need_w, N, merged):
    """the batch node, downwards: hidden layers as ONE stacked product [u; z-bar]^T [v-bar; a] over 2N rows (with the row
    node's cotangents as addends where it left them), the last layer as z-bar^T a over N rows"""
    L = len(dims)
    out = []
    for l in range(L - 1, -1, -1):
        if need_w[l]:
            o, i = dims[l]
            out.append((2 * N, o, i, l in merged, l in merged) if l < L - 1 else (N, o, i, False, False))
    return out


def _row_products(dims, need_w, n, merge):
    """the row node has no stack: u^T v-bar per hidden layer upwards, then z-bar^T a per layer downwards, all over its n
    rows; merged, its hidden layers contribute nothing"""
    L = len(dims)
    hidden = [] if merge else [l for l in range(L - 1) if need_w[l]]
    down = [l for l in range(L - 1, -1, -1) if need_w[l] and (l == L - 1 or not merge)]
    return [(n, dims[l][0], dims[l][1], False, False) for l in hidden + down]


def predicted_products(dims, mask, N, rows=None, merge=False, row_mask=None):
    """[(K, M, N, has_a_addend, has_b_addend)] in the order one backward pass hands the products to gemm_group_tn /
    gemm_group_tn_add: the row node's (its backward runs first), then the batch node's.  rows = (row0, n) adds the row
    node; its hidden layers merge into the batch node's products only when both nodes want the same gradients."""
    if rows is None:
        return _owner_products(dims, mask.w, N, ())
    row_mask = mask if row_mask is None else row_mask
    merge = bool(merge) and (mask.w, mask.b) == (row_mask.w, row_mask.b)
    merged = [l for l in range(len(dims) - 1) if row_mask.w[l]] if merge else []
    return _row_products(dims, row_mask.w, rows[1], merge) + _owner_products(dims, mask.w, N, merged)


# ---- the SDF reference -----------------------------------------------------------------------------------------------
def sdf_trunk(e, Ws, bs, skip, beta_sp, thr_sp):
    """the last layer's output: plain layers, cat[h, e] / sqrt 2 at the skip, softplus between layers"""
    h, L = e, len(Ws)
    for l in range(L):
        if l == skip:
            h = torch.cat([h, e], 1) / math.sqrt(2.0)
        h = h @ Ws[l].t() + bs[l]
        if l < L - 1:
            h = F.softplus(h, beta=beta_sp, threshold=thr_sp)
    return h


def clamp_rho(s, beta_rho):
    beta = f32(beta_rho)
    return (1.0 / beta) * (0.5 + 0.5 * torch.sign(s) * torch.expm1(-s.abs() / beta))


def sdf_forward(e, Ws, bs, skip, beta_sp, thr_sp, beta_rho, rho=None):
    """(out [N, out_last] with the soft-clamped SDF in column 0, the SDF [N]): sdf = tanh(s / (2 + rho(s))) of column 0 of
    the trunk with rho held constant (rho: its values, else computed from s without gradient)"""
    h = sdf_trunk(e, Ws, bs, skip, beta_sp, thr_sp)
    s = h[:, 0]
    if rho is None:
        with torch.no_grad():
            rho = clamp_rho(s, beta_rho)
    sdf = torch.tanh(s / (2.0 + rho))
    return torch.cat([sdf.unsqueeze(1), h[:, 1:]], 1), sdf


def sdf_mlp_ref(e, Ws, bs, skip, beta_sp, thr_sp, beta_rho):
    """(out, g_e = d sum(sdf) / d e), differentiable once more; e must require a gradient"""
    out, sdf = sdf_forward(e, Ws, bs, skip, beta_sp, thr_sp, beta_rho)
    (g_e,) = torch.autograd.grad(sdf.sum(), e, create_graph=True)
    return out, g_e


def relu_mlp_ref(x, Ws, bs):
    h, L = x, len(Ws)
    for l in range(L):
        h = h @ Ws[l].t() + bs[l]
        if l < L - 1:
            h = torch.relu(h)
    return h


def loss_of(kind, out, g_e, R, Rg):
    """the cotangent patterns: d_ge arrives as zeros | d_out arrives as zeros | both | both as stride-0 expansions"""
    if kind == "out":
        return (out * R).sum()
    if kind == "ge":
        return (g_e * Rg).sum() + ((g_e.norm(dim=1) - 1) ** 2).mean()
    if kind == "both":
        return loss_of("out", out, g_e, R, Rg) + loss_of("ge", out, g_e, R, Rg)
    assert kind == "sum", kind
    return out.sum() + g_e.sum()


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _draw(shape, scale, *key):
    return scale * torch.randn(shape, generator=_gen(*key), dtype=F32)


def _params(dims, *key):
    Ws = [_draw((o, i), 1.0 / math.sqrt(i), *key, 10 + l) for l, (o, i) in enumerate(dims)]
    bs = [_draw((o,), 0.1, *key, 40 + l) for l, (o, _) in enumerate(dims)]
    return Ws, bs


SEEDS = 16


def _sdf_draw(name, N, seed):
    net = NETS[name]
    key = (1, list(NETS).index(name), N, seed)
    Ws, bs = _params(net.dims, *key)
    return dict(e=_draw((N, net.E), 0.25, *key, 1), Ws=Ws, bs=bs, R=_draw((N, net.dims[-1][0]), 1.0, *key, 2),
                Rg=_draw((N, net.E), 1.0, *key, 3))


def orders(name, N):
    """the other (row order, embedding column order) pairs torch's fp32 evaluation is repeated in: both reversed, and
    three seeded shuffles"""
    E = NETS[name].E
    out = [(torch.arange(N - 1, -1, -1), torch.arange(E - 1, -1, -1))]
    return out + [(torch.randperm(N, generator=_gen(4, N, k)), torch.randperm(E, generator=_gen(5, E, k))) for k in range(3)]


def representative(r64, r32, others):
    """does a case measure the kernel?  From the reference alone (as elem_cases.rownorm_inputs draws its rows):
      - torch's fp32 evaluation stays within a quarter of the cap for every tensor, and no tensor is all zero;
      - the SAME fp32 evaluation in other summation orders (`others`: rows and embedding columns reordered) passes the
        limit the first sets.  The limit is 4 e32 + 2^-22 scale with e32 ONE sample of fp32 rounding; where a tensor is a
        cancelling sum over the rows (depth0, loss ge, N = 130: db0 has one non-zero element, the sum of 130 terms of
        both signs, 1 / 21 of the sum of their magnitudes, each proportional to an SDF value of about 0.1 that carries
        the rounding of its 27-term dot product) that sample ranges from 1.9e-8 to 1.1e-7 with the summation order and
        the machine's vector width, so a lucky one sets a limit that torch itself misses in another order - such a
        draw measures luck, and is drawn again."""
    for k in r64:
        e32, scale = errors(r64[k], r32[k])
        if not (scale > 0.0 and e32 <= 0.25 * CAP * scale):
            return False
        lim = limit(e32, scale)
        if any(float((o[k].to(F64) - r64[k]).abs().max()) > lim for o in others):
            return False
    return True


@functools.lru_cache(maxsize=None)
def sdf_seed(name, N):
    """the first seed whose draw is representative() under every loss"""
    for seed in range(SEEDS):
        inp = _sdf_draw(name, N, seed)
        if all(representative(_sdf_single(name, inp, lo, F64), _sdf_single(name, inp, lo, F32),
                              [_sdf_single(name, inp, lo, F32, order) for order in orders(name, N)]) for lo in LOSSES):
            return seed
    raise AssertionError(f"no representative draw for {name}, N = {N}")


@functools.lru_cache(maxsize=None)
def sdf_inputs(name, N):
    """fp32 CPU tensors: e ~ 0.25 randn, W ~ randn / sqrt(in), b ~ 0.1 randn, R, Rg ~ randn"""
    return _sdf_draw(name, N, sdf_seed(name, N))


@functools.lru_cache(maxsize=None)
def pair_inputs(rows):
    net = NETS[PAIR_NET]
    n_eik, n_ray, row0, n = rows
    N = n_eik + n_ray
    key = (2, PAIR_ROWS.index(rows), 0)
    Ws, bs = _params(net.dims, *key)
    out_w = net.dims[-1][0]
    return dict(e=_draw((N, net.E), 0.25, *key, 1), Ws=Ws, bs=bs, R=_draw((N, out_w), 1.0, *key, 2),
                Rg=_draw((N, net.E), 1.0, *key, 3), R2=_draw((n, out_w), 1.0, *key, 4), Rg2=_draw((n, net.E), 1.0, *key, 5))


def _leaf(t, dt):
    return t.to(dt, copy=True).requires_grad_(True)     # (a copy: the inputs are shared and stay without gradient)


def _leaves(inp, dt, first="e"):
    return _leaf(inp[first], dt), [_leaf(w, dt) for w in inp["Ws"]], [_leaf(b, dt) for b in inp["bs"]]


def _named(L, outs, grads, names):
    res = {k: v.detach() for k, v in outs.items()}
    res.update({k: g.detach() for k, g in zip(names, grads[:len(names)])})
    res.update({f"dW{l}": g.detach() for l, g in enumerate(grads[len(names):len(names) + L])})
    res.update({f"db{l}": g.detach() for l, g in enumerate(grads[len(names) + L:])})
    return res


def _sdf_single(name, inp, loss, dt, order=None):
    """order = (row order, embedding column order) or None: evaluate the same expression with the rows and the
    embedding's columns (with them the matching columns of W_0 and of the skip layer's W) in that order - other
    summation orders of the sums over the rows and of the first dot products; the results are put back"""
    net = NETS[name]
    e, Ws, bs = _leaves(inp, dt)
    R, Rg = inp["R"].to(dt), inp["Rg"].to(dt)
    if order is not None:
        rows, cols = order
        e, R, Rg = e.detach()[rows][:, cols].requires_grad_(True), R[rows], Rg[rows][:, cols]
        wcols = {0: cols}
        if net.skip > 0:
            dh = net.dims[net.skip][1] - net.E
            wcols[net.skip] = torch.cat([torch.arange(dh), dh + cols])
        Ws = [w.detach()[:, wcols[l]].requires_grad_(True) if l in wcols else w for l, w in enumerate(Ws)]
    out, g_e = sdf_mlp_ref(e, Ws, bs, net.skip, BETA_SP, THR_SP, BETA_RHO)
    lo = loss_of(loss, out, g_e, R, Rg)
    grads = torch.autograd.grad(lo, [e, *Ws, *bs], allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, [e, *Ws, *bs])]
    res = _named(len(Ws), dict(out=out, g_e=g_e), grads, ["d_e"])
    if order is not None:
        rback, cback = torch.argsort(rows), torch.argsort(cols)
        res["out"] = res["out"][rback]
        res.update({k: res[k][rback][:, cback] for k in ("g_e", "d_e")})
        res.update({f"dW{l}": res[f"dW{l}"][:, torch.argsort(wc)] for l, wc in wcols.items()})
    return res


@functools.lru_cache(maxsize=None)
def sdf_single_ref(name, N, loss):
    """(float64 reference, torch's fp32 evaluation): dicts out, g_e, d_e, dW{l}, db{l}; shared and left unchanged"""
    inp = sdf_inputs(name, N)
    return _sdf_single(name, inp, loss, F64), _sdf_single(name, inp, loss, F32)


def row_detached(masks):
    """the layers whose weight the row node sees detached (frozen on the row node only)"""
    return tuple(l for l, (w, w2) in enumerate(zip(masks[0].w, masks[1].w)) if w and not w2)


def _sdf_pair(rows, detached, dt):
    """two calls of sdf_mlp_ref on shared parameters; the second on e2 = e.detach()[sl] + (out[sl, :1] - out[sl, :1].detach()),
    the construction of tests/test_wgrad_once_gpu.py (the same numbers, a gradient path into the first call's output).
    detached: layers whose weight the second call sees detached - that is another function of the leaves, not a subset
    of the same gradients, so it has a reference of its own"""
    net, inp = NETS[PAIR_NET], pair_inputs(rows)
    _, _, row0, n = rows
    sl = slice(row0, row0 + n)
    e, Ws, bs = _leaves(inp, dt)
    out, g_e = sdf_mlp_ref(e, Ws, bs, net.skip, BETA_SP, THR_SP, BETA_RHO)
    e2 = e.detach()[sl] + (out[sl, :1] - out[sl, :1].detach())
    Ws2 = [w.detach() if l in detached else w for l, w in enumerate(Ws)]
    out2, g2 = sdf_mlp_ref(e2, Ws2, bs, net.skip, BETA_SP, THR_SP, BETA_RHO)
    lo = loss_of(PAIR_LOSS, out, g_e, inp["R"].to(dt), inp["Rg"].to(dt)) + \
        loss_of(PAIR_LOSS, out2, g2, inp["R2"].to(dt), inp["Rg2"].to(dt))
    grads = torch.autograd.grad(lo, [e, e2, *Ws, *bs])
    return _named(len(Ws), dict(out=out, g_e=g_e, out2=out2, g2=g2), grads, ["d_e", "d_e2"])


@functools.lru_cache(maxsize=None)
def sdf_pair_ref(rows, detached=()):
    return _sdf_pair(rows, detached, F64), _sdf_pair(rows, detached, F32)


# ---- relu_mlp --------------------------------------------------------------------------------------------------------
RELU_DIMS = ((7, 3), (5, 33, 1), (281, 129, 64, 33, 100, 3))
RELU_N = (1, 77, 130)
PLANT_ZERO, PLANT_DEAD = 3, 7       # units of the first hidden layer: pre-activation exactly 0 | bias -10


def relu_masks(L):
    """{name: (x, per-layer W, per-layer b)}"""
    every, none = (True,) * L, (False,) * L
    out = {"all": Mask(True, every, every), "w_alternating": Mask(True, tuple(l % 2 == 1 for l in range(L)), every),
           "b_none": Mask(True, every, none), "x_off": Mask(False, every, every), "x_only": Mask(True, none, none)}
    return out


def relu_variants(dims):
    return (False, True) if len(dims) > 2 else (False,)


@functools.lru_cache(maxsize=None)
def relu_inputs(dims, n, planted):
    """x ~ randn, W ~ randn / sqrt(in), b ~ 0.1 randn, R ~ randn.  planted: unit PLANT_ZERO of the first hidden layer has
    a zero weight row and zero bias (pre-activation exactly 0, where relu' = 0 as torch has it), unit PLANT_DEAD has
    bias -10 (dead on every row)"""
    key = (3, RELU_DIMS.index(dims), n, 0)
    layer = list(zip(dims[1:], dims[:-1]))
    Ws, bs = _params(layer, *key)
    if planted:
        Ws[0][PLANT_ZERO] = 0.0
        bs[0][PLANT_ZERO] = 0.0
        bs[0][PLANT_DEAD] = -10.0
    return dict(x=_draw((n, dims[0]), 1.0, *key, 1), Ws=Ws, bs=bs, R=_draw((n, dims[-1]), 1.0, *key, 2))


def _relu(dims, n, planted, dt):
    inp = relu_inputs(dims, n, planted)
    x, Ws, bs = _leaves(inp, dt, "x")
    y = relu_mlp_ref(x, Ws, bs)
    grads = torch.autograd.grad((y * inp["R"].to(dt)).sum(), [x, *Ws, *bs])
    return _named(len(Ws), dict(y=y), grads, ["d_x"])


@functools.lru_cache(maxsize=None)
def relu_ref(dims, n, planted):
    return _relu(dims, n, planted, F64), _relu(dims, n, planted, F32)
