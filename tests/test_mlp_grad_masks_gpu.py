"""The autograd nodes of mlp_grad.py (_SdfMlp, _SdfMlpRows, _ReluMlp) under frozen-parameter masks, against the float64
references of tests/mlp_grad_cases.py (checked on the CPU by tests/test_mlp_grad_cases_cpu.py), in the default (atomic)
mode and under ops.deterministic().  Every comparison prints its error, e32, scale and limit (elem_cases.compare).

Arm of _sdf_mlp_backward -> case:
  stacked product [u; z-bar]^T [v-bar; a]     every hidden layer whose weight wants a gradient on the batch node
  loose / want_out3, unstacked skip concat    a frozen hidden weight on the batch node (w_none, w_even / w_odd / w_skip
                                              _frozen, w_last_only); every hidden layer of the row node
  dst of the adjoint epilogue, need_w[nxt]    w_odd_frozen / w_even_frozen: a stacked layer after an unstacked one and back
  copy into stack[l][:N] skipped or not       the same masks (layer 0, and a stacked layer after an unstacked one)
  last layer's c^T v-bar without need_w       w_last_frozen, w_none, e_only;  need_e false: e_off
  zero / expanded cotangents                  losses out, ge, sum
  L = 1, L = 2, skip at L - 1, at 1           depth0, depth1, skip_last, skip1
  wgrad_acc handed over / added up            pair masks all, w2_frozen, b_none / w1_frozen_on_rows
  row_cot addends taken by the kernel or not  rows (16, 48, 16, 48) / (16, 48, 18, 46) and every K = 2N that is not 128
  saved rows at 4-byte aligned addresses      rows (5, 9, 5, 9), (3, 13, 1, 7)
The weight-gradient products each backward pass hands to gemm_group_tn / gemm_group_tn_add are recorded and compared
with mlp_grad_cases.predicted_products: that is what shows a mask reached its arm.

The d_ge is None arm of _sdf_mlp_backward is not reached: autograd materialises both cotangents of a node.
The largest err / limit per group and mode is printed by the last test; the figures observed are kept in
tests/golden/mlp_grad_masks_observed.json (a record no test reads)."""
import json

import pytest
import torch

import elem_cases as E
import mlp_grad_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("atomic", "deterministic")
_WORST = {}


def _mods():
    from hashmodnffbanks_idr_amd import mlp_grad, ops
    return mlp_grad, ops


def _check(group, what, got, refs, live):
    """every tensor of `got` against the float64 reference; a frozen tensor has no gradient"""
    r64, r32 = refs
    assert set(got) == set(r64), (what, sorted(got), sorted(r64))
    for k in sorted(r64):
        if not live.get(k, True):
            assert got[k] is None, f"{what}: {k} is frozen and has a gradient"
            continue
        assert got[k] is not None, f"{what}: {k} has no gradient"
        e32, scale = E.errors(r64[k], r32[k])
        lim = E.limit(e32, scale)
        err = float((got[k].detach().to("cpu", torch.float64) - r64[k]).abs().max())
        _WORST[group] = max(_WORST.get(group, 0.0), err / lim if lim > 0.0 else float(err > 0.0))
        E.compare(f"{what} {k}", got[k], r64[k], r32[k])


def _live(mask, names=("d_e",)):
    live = {names[0]: mask.e}
    for l, (w, b) in enumerate(zip(mask.w, mask.b)):
        live[f"dW{l}"], live[f"db{l}"] = w, b
    return live


class _Recorder:
    """records (K, M, N, has_a_addend, has_b_addend) and the operands' addresses of every product handed to
    mlp_grad.gemm_group_tn / gemm_group_tn_add, then runs it"""

    def __init__(self, mlp_grad):
        self.m, self.products, self.ptrs = mlp_grad, [], []

    def __enter__(self):
        self.orig = (self.m.gemm_group_tn, self.m.gemm_group_tn_add)

        def plain(problems):
            for a, b, c in problems:
                self.products.append((a.shape[0], a.shape[1], b.shape[1], False, False))
                self.ptrs += [a.data_ptr(), b.data_ptr()]
            return self.orig[0](problems)

        def add(problems):
            for a, b, c, aa, ba in problems:
                self.products.append((a.shape[0], a.shape[1], b.shape[1], aa is not None, ba is not None))
                self.ptrs += [a.data_ptr(), b.data_ptr()]
            return self.orig[1](problems)
        self.m.gemm_group_tn, self.m.gemm_group_tn_add = plain, add
        return self

    def __exit__(self, *exc):
        self.m.gemm_group_tn, self.m.gemm_group_tn_add = self.orig


def _mode(ops, mode):
    return ops.deterministic(mode == "deterministic")


def _params(inp, mask):
    Ws = [w.to(DEV).requires_grad_(mask.w[l]) for l, w in enumerate(inp["Ws"])]
    bs = [b.to(DEV).requires_grad_(mask.b[l]) for l, b in enumerate(inp["bs"])]
    return Ws, bs


def _same_bits(what, a, b):
    assert set(a) == set(b)
    for k, v in a.items():
        assert (v is None) == (b[k] is None) and (v is None or torch.equal(v, b[k])), f"{what}: {k} differs between two runs"


# ---- sdf_mlp, one node ---------------------------------------------------------------------------------------------------
def _run_single(net, N, mask, loss, mode):
    mlp_grad, ops = _mods()
    inp = C.sdf_inputs(net.name, N)
    e = inp["e"].to(DEV).requires_grad_(mask.e)
    Ws, bs = _params(inp, mask)
    with _Recorder(mlp_grad) as rec, _mode(ops, mode):
        out, g_e = mlp_grad.sdf_mlp(e, Ws, bs, net.skip, C.BETA_SP, C.THR_SP, C.BETA_RHO)
        C.loss_of(loss, out, g_e, inp["R"].to(DEV), inp["Rg"].to(DEV)).backward()
        torch.cuda.synchronize()
    res = {"out": out.detach(), "g_e": g_e.detach(), "d_e": e.grad}
    res.update({f"dW{l}": w.grad for l, w in enumerate(Ws)})
    res.update({f"db{l}": b.grad for l, b in enumerate(bs)})
    return res, rec


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", C.BATCHES)
@pytest.mark.parametrize("name", list(C.NETS))
def test_sdf_mlp_under_masks(name, N, mode):
    net = C.NETS[name]
    ms = C.masks(net)
    for mname, loss in C.single_pairs(net):
        mask = ms[mname]
        what = f"{name} N={N} {mname} {loss} {mode}"
        res, rec = _run_single(net, N, mask, loss, mode)
        assert rec.products == C.predicted_products(net.dims, mask, N), (what, rec.products)
        _check(f"single node, {mode}", what, res, C.sdf_single_ref(name, N, loss), _live(mask))
        if mode == "deterministic":
            _same_bits(what, res, _run_single(net, N, mask, loss, mode)[0])


# ---- sdf_mlp + sdf_mlp_rows ------------------------------------------------------------------------------------------
def _run_pair(rows, merge, masks, mode):
    mlp_grad, ops = _mods()
    net = C.NETS[C.PAIR_NET]
    mask, row_mask = masks
    n_eik, n_ray, row0, n = rows
    sl = slice(row0, row0 + n)
    inp = C.pair_inputs(rows)
    e = inp["e"].to(DEV).requires_grad_(mask.e)
    Ws, bs = _params(inp, mask)
    with _Recorder(mlp_grad) as rec, _mode(ops, mode):
        cache = {}
        out, g_e = mlp_grad.sdf_mlp(e, Ws, bs, net.skip, C.BETA_SP, C.THR_SP, C.BETA_RHO, cache_out=cache)
        # the row node's input: the same numbers, a gradient path of its own and one into the batch node's output, so
        # that the row node's backward runs first
        e2 = e.detach()[sl] + (out[sl, :1] - out[sl, :1].detach())
        e2.retain_grad()
        Ws2 = [w if row_mask.w[l] else w.detach() for l, w in enumerate(Ws)]
        bs2 = [b if row_mask.b[l] else b.detach() for l, b in enumerate(bs)]
        out2, g2 = mlp_grad.sdf_mlp_rows(e2, cache, row0, n, Ws2, bs2, merge_wgrad=merge)
        saved = [t[sl].data_ptr() for k in ("a_list", "z_list", "v_list") for t in cache[k]]
        lo = C.loss_of(C.PAIR_LOSS, out, g_e, inp["R"].to(DEV), inp["Rg"].to(DEV)) + \
            C.loss_of(C.PAIR_LOSS, out2, g2, inp["R2"].to(DEV), inp["Rg2"].to(DEV))
        lo.backward()
        torch.cuda.synchronize()
    res = {"out": out.detach(), "g_e": g_e.detach(), "out2": out2.detach(), "g2": g2.detach(), "d_e": e.grad,
           "d_e2": e2.grad}
    res.update({f"dW{l}": w.grad for l, w in enumerate(Ws)})
    res.update({f"db{l}": b.grad for l, b in enumerate(bs)})
    return res, rec, saved


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mname", list(C.pair_masks(C.NETS[C.PAIR_NET])))
@pytest.mark.parametrize("merge", (True, False), ids=("merged", "unmerged"))
@pytest.mark.parametrize("rows", C.PAIR_ROWS, ids=str)
def test_sdf_mlp_rows_under_masks(rows, merge, mname, mode):
    net = C.NETS[C.PAIR_NET]
    masks = C.pair_masks(net)[mname]
    n_eik, n_ray, row0, n = rows
    N, sl = n_eik + n_ray, slice(row0, row0 + n)
    what = f"rows {rows} {'merged' if merge else 'unmerged'} {mname} {mode}"
    res, rec, saved = _run_pair(rows, merge, masks, mode)
    want = C.predicted_products(net.dims, masks[0], N, rows=(row0, n), merge=merge, row_mask=masks[1])
    assert rec.products == want, (what, rec.products)
    assert torch.equal(res["out2"], res["out"][sl]) and torch.equal(res["g2"], res["g_e"][sl]), what
    live = _live(masks[0])
    live["d_e2"] = True
    _check(f"two nodes {'merged' if merge else 'unmerged'}, {mode}", what, res,
           C.sdf_pair_ref(rows, C.row_detached(masks)), live)
    if rows in C.MISALIGNED_ROWS:
        # the row node's saved rows, and (unmerged, where its hidden layers form products of their own) the operands
        # of its products, start off a 16-byte boundary - else the case does not test what it is for
        assert any(p % 16 for p in saved), what
        assert merge or any(p % 16 for p in rec.ptrs), what
    if mode == "deterministic":
        _same_bits(what, res, _run_pair(rows, merge, masks, mode)[0])


# ---- relu_mlp --------------------------------------------------------------------------------------------------------
def _run_relu(dims, n, planted, mask, mode):
    mlp_grad, ops = _mods()
    inp = C.relu_inputs(dims, n, planted)
    x = inp["x"].to(DEV).requires_grad_(mask.e)
    Ws, bs = _params(inp, mask)
    with _Recorder(mlp_grad) as rec, _mode(ops, mode):
        y = mlp_grad.relu_mlp(x, Ws, bs)
        (y * inp["R"].to(DEV)).sum().backward()
        torch.cuda.synchronize()
    res = {"y": y.detach(), "d_x": x.grad}
    res.update({f"dW{l}": w.grad for l, w in enumerate(Ws)})
    res.update({f"db{l}": b.grad for l, b in enumerate(bs)})
    return res, rec


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", C.RELU_N)
@pytest.mark.parametrize("dims", C.RELU_DIMS, ids=str)
def test_relu_mlp_under_masks(dims, n, mode):
    L = len(dims) - 1
    for planted in C.relu_variants(dims):
        for mname, mask in C.relu_masks(L).items():
            what = f"relu {dims} n={n} {mname} planted={planted} {mode}"
            res, rec = _run_relu(dims, n, planted, mask, mode)
            want = [(n, dims[l + 1], dims[l], False, False) for l in range(L - 1, -1, -1) if mask.w[l]]
            assert rec.products == want, (what, rec.products)
            _check(f"relu, {mode}", what, res, C.relu_ref(dims, n, planted), _live(mask, ("d_x",)))
            if planted:     # relu'(0) = 0 and a dead unit: exactly no gradient, as the reference has it
                for unit in (C.PLANT_ZERO, C.PLANT_DEAD):
                    if mask.w[0]:
                        assert int(torch.count_nonzero(res["dW0"][unit])) == 0, (what, unit)
                    if mask.b[0]:
                        assert float(res["db0"][unit]) == 0.0, (what, unit)
            if mode == "deterministic":
                _same_bits(what, res, _run_relu(dims, n, planted, mask, mode)[0])


def test_zz_observed_figures():
    """the largest err / limit per group and mode of the tests above that ran in this session"""
    print("mlp_grad_masks_observed " + json.dumps({k: float(f"{v:.3g}") for k, v in sorted(_WORST.items())}))
    assert all(v <= 1.0 for v in _WORST.values())
