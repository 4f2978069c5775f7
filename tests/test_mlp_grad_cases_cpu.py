"""tests/mlp_grad_cases.py on the CPU: the references against float64 gradcheck of the forward expression under them (so a
reference cannot share a mistake with mlp_grad.py), the two-node restatement against one network over cat[e, e2], the
conditioning of every case tests/test_mlp_grad_masks_gpu.py runs (torch's fp32 evaluation stays within a quarter of the
2e-5 cap, so the cap never decides a limit), the properties the cases rely on (both sides of the softplus threshold, the
planted ReLU units) and the product-list predictor on the arrangements tests/test_wgrad_once_gpu.py documents."""
import pytest
import torch

import elem_cases as E
import mlp_grad_cases as C

F32, F64 = torch.float32, torch.float64


def _conditioned(what, refs):
    r64, r32 = refs
    assert set(r64) == set(r32)
    for k in r64:
        e32, scale = E.errors(r64[k], r32[k])
        print(f"    {what} {k}: fp32 torch error / scale {e32 / max(scale, 1e-300):.3e}")
        assert bool(torch.isfinite(r64[k]).all()) and scale > 0.0, (what, k)
        assert e32 <= 0.25 * E.CAP * scale, (what, k, e32, scale)


# ---- the references --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["depth1", "skip1"])
def test_sdf_reference_against_gradcheck(name):
    """gradcheck / gradgradcheck of the forward expression (rho held at its values, as the clamp holds it), and g_e of
    sdf_mlp_ref is that expression's gradient"""
    net = C.NETS[name]
    inp = C.sdf_inputs(name, 3)
    e, Ws, bs = C._leaves(inp, F64)
    L = len(Ws)
    out_ref, g_ref = C.sdf_mlp_ref(e, Ws, bs, net.skip, C.BETA_SP, C.THR_SP, C.BETA_RHO)
    with torch.no_grad():
        rho = C.clamp_rho(C.sdf_trunk(e, Ws, bs, net.skip, C.BETA_SP, C.THR_SP)[:, 0], C.BETA_RHO)
    assert float(rho.abs().min()) > 0.0             # (held constant below: a numerical derivative would see it move)

    def fwd(e_, *p):
        return C.sdf_forward(e_, p[:L], p[L:], net.skip, C.BETA_SP, C.THR_SP, C.BETA_RHO, rho=rho)[0]
    out_fixed = fwd(e, *Ws, *bs)
    assert float((out_fixed - out_ref).detach().abs().max()) <= 1e-12
    (g_fixed,) = torch.autograd.grad(out_fixed[:, 0].sum(), e)
    assert float((g_fixed - g_ref).detach().abs().max()) <= 1e-12 * float(g_ref.detach().abs().max())
    assert torch.autograd.gradcheck(fwd, (e, *Ws, *bs), eps=1e-6, atol=1e-7, rtol=1e-5)
    assert torch.autograd.gradgradcheck(fwd, (e, *Ws, *bs), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_relu_reference_against_gradcheck():
    inp = C.relu_inputs((5, 33, 1), 1, False)
    x = C._draw((3, 5), 1.0, 99).to(F64).requires_grad_(True)
    _, Ws, bs = C._leaves(inp, F64, "x")
    L = len(Ws)
    assert torch.autograd.gradcheck(lambda x_, *p: C.relu_mlp_ref(x_, p[:L], p[L:]), (x, *Ws, *bs), eps=1e-6, atol=1e-7)
    y = C.relu_mlp_ref(x, Ws, bs)
    h = torch.relu(x @ Ws[0].t() + bs[0])
    assert torch.equal(y, h @ Ws[1].t() + bs[1])


@pytest.mark.parametrize("rows", C.PAIR_ROWS, ids=str)
def test_two_node_restatement_is_one_network_over_both_inputs(rows):
    """float64: the outputs and gradients of the two calls equal ONE evaluation of cat[e, e2] under the same loss, with
    the gradient that reaches e2 handed on to column 0 of the first rows' output by hand"""
    net, inp = C.NETS[C.PAIR_NET], C.pair_inputs(rows)
    _, _, row0, n = rows
    N = inp["e"].shape[0]
    sl = slice(row0, row0 + n)
    ref = C.sdf_pair_ref(rows)[0]
    e, Ws, bs = C._leaves(inp, F64)
    e2 = e.detach()[sl].clone().requires_grad_(True)
    out_all, g_all = C.sdf_mlp_ref(torch.cat([e, e2], 0), Ws, bs, net.skip, C.BETA_SP, C.THR_SP, C.BETA_RHO)
    lo = C.loss_of(C.PAIR_LOSS, out_all[:N], g_all[:N], inp["R"].to(F64), inp["Rg"].to(F64)) + \
        C.loss_of(C.PAIR_LOSS, out_all[N:], g_all[N:], inp["R2"].to(F64), inp["Rg2"].to(F64))
    grads = list(torch.autograd.grad(lo, [e, e2, *Ws, *bs]))
    # e2 = const + out[sl, :1] - const: its cotangent, summed over the columns, arrives at out[sl, 0]
    out_first = C.sdf_forward(e, Ws, bs, net.skip, C.BETA_SP, C.THR_SP, C.BETA_RHO)[0]
    extra = torch.autograd.grad((out_first[sl, 0] * grads[1].sum(1)).sum(), [e, *Ws, *bs])
    grads = [grads[0] + extra[0], grads[1]] + [g + x for g, x in zip(grads[2:], extra[1:])]
    got = C._named(len(Ws), dict(out=out_all[:N], g_e=g_all[:N], out2=out_all[N:], g2=g_all[N:]), grads, ["d_e", "d_e2"])
    assert set(got) == set(ref)
    for k in ref:
        scale = float(ref[k].abs().max())
        assert float((got[k] - ref[k]).abs().max()) <= 1e-12 * scale, (rows, k)
    for a, b in (("out2", "out"), ("g2", "g_e")):     # the same numbers: e2 equals e[sl] in value
        assert float((ref[a] - ref[b][sl]).abs().max()) <= 1e-12 * float(ref[b].abs().max())


# ---- conditioning ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.NETS))
def test_single_node_cases_are_conditioned(name):
    """... and torch's fp32 evaluation in other summation orders passes the limit the first evaluation sets
    (mlp_grad_cases.representative: else the draw measures the luck of one fp32 sample, not the kernel)"""
    for N in C.BATCHES:
        inp = C.sdf_inputs(name, N)
        print(f"    {name} N={N}: seed {C.sdf_seed(name, N)}")
        for loss in C.LOSSES:
            r64, r32 = C.sdf_single_ref(name, N, loss)
            _conditioned(f"{name} N={N} {loss}", (r64, r32))
            for order in C.orders(name, N):
                other = C._sdf_single(name, inp, loss, F32, order)
                for k in r64:
                    assert float((other[k].to(F64) - r64[k]).abs().max()) <= E.limit(*E.errors(r64[k], r32[k])), (name, N, loss, k)


@pytest.mark.parametrize("rows", C.PAIR_ROWS, ids=str)
def test_two_node_cases_are_conditioned(rows):
    for detached in sorted({C.row_detached(m) for m in C.pair_masks(C.NETS[C.PAIR_NET]).values()}):
        _conditioned(f"pair {rows} detached on the row node {detached}", C.sdf_pair_ref(rows, detached))


@pytest.mark.parametrize("dims", C.RELU_DIMS, ids=str)
def test_relu_cases_are_conditioned(dims):
    """... and no hidden pre-activation other than the planted one sits where its sign could differ between two
    evaluations (a flipped unit moves a gradient by a finite amount)"""
    for n in C.RELU_N:
        for planted in C.relu_variants(dims):
            _conditioned(f"relu {dims} n={n} planted={planted}", C.relu_ref(dims, n, planted))
            inp = C.relu_inputs(dims, n, planted)
            h = inp["x"].to(F64)
            for l in range(len(dims) - 2):
                z = h @ inp["Ws"][l].to(F64).t() + inp["bs"][l].to(F64)
                if planted and l == 0:
                    z = z.clone()
                    z[:, C.PLANT_ZERO] = 1.0
                # an fp32 sum of K terms is off by about sqrt(K) roundings of the sum of their magnitudes
                mag = h.abs() @ inp["Ws"][l].to(F64).abs().t() + inp["bs"][l].to(F64).abs()
                assert bool((z.abs() > h.shape[1] ** 0.5 * 2.0 ** -24 * mag).all()), (dims, n, l)
                h = torch.relu(z)


# ---- properties the cases rely on ------------------------------------------------------------------------------------
def test_case_tables():
    inp = C.sdf_inputs("skip2", 7)
    C.sdf_single_ref("skip2", 7, "both")
    assert not any(t.requires_grad for t in [inp["e"], *inp["Ws"], *inp["bs"]])     # the shared inputs stay plain
    ms = C.masks(C.NETS["skip2"])
    assert len(ms) == 11 and [k for k, m in ms.items() if not m.e] == ["e_off"]
    assert ms["w_even_frozen"].w == (False, True, False, True, False)
    assert ms["w_odd_frozen"].w == (True, False, True, False, True)
    assert ms["w_skip_frozen"].w == (True, True, False, True, True)
    assert ms["w_last_only"].w == (False, False, False, False, True)
    assert ms["b_ends_frozen"].b == (False, True, True, True, False)
    assert ms["e_only"] == C.Mask(True, (False,) * 5, (False,) * 5)
    for net in C.NETS.values():
        assert len(set(C.masks(net).values())) == len(C.masks(net))
        assert {m for m, _ in C.single_pairs(net)} == set(C.masks(net))
        assert {lo for _, lo in C.single_pairs(net)} == set(C.LOSSES)
        for l, (o, i) in enumerate(net.dims):      # the layer widths chain, with the skip's concatenation
            prev = net.E if l == 0 else net.dims[l - 1][0] + (net.E if l == net.skip else 0)
            assert i == prev, (net.name, l)
    assert len(C.single_pairs(C.NETS["skip2"])) == 44
    draw = C._sdf_draw("skip1", 7, 0)      # a reordered evaluation is the same expression: equal in float64
    plain = C._sdf_single("skip1", draw, "both", F64)
    for order in C.orders("skip1", 7):
        other = C._sdf_single("skip1", draw, "both", F64, order)
        assert all(float((other[k] - plain[k]).abs().max()) <= 1e-12 * float(plain[k].abs().max()) for k in plain)
    for n_eik, n_ray, row0, n in C.PAIR_ROWS:
        assert 0 <= row0 and row0 + n <= n_eik + n_ray and n >= 1
    for rows in C.MISALIGNED_ROWS:        # rows of odd widths that start off a 16-byte boundary
        assert rows in C.PAIR_ROWS and (rows[2] * 27) % 4 != 0 and (rows[2] * 37) % 4 != 0


def test_skip2_straddles_the_softplus_threshold():
    net, inp = C.NETS["skip2"], C.sdf_inputs("skip2", 33)
    e = inp["e"]
    h = e
    for l in range(len(net.dims) - 1):
        if l == net.skip:
            h = torch.cat([h, e], 1) / 2.0 ** 0.5
        z = h @ inp["Ws"][l].t() + inp["bs"][l]
        assert bool((C.BETA_SP * z > C.THR_SP).any()) and bool((C.BETA_SP * z < C.THR_SP).any()), l
        h = torch.nn.functional.softplus(z, beta=C.BETA_SP, threshold=C.THR_SP)


@pytest.mark.parametrize("dims", [d for d in C.RELU_DIMS if len(d) > 2], ids=str)
def test_planted_relu_units(dims):
    for n in C.RELU_N:
        inp = C.relu_inputs(dims, n, True)
        z = inp["x"] @ inp["Ws"][0].t() + inp["bs"][0]
        assert z.dtype == F32 and bool((z[:, C.PLANT_ZERO] == 0).all()) and bool((z[:, C.PLANT_DEAD] < 0).all())
        r64, r32 = C.relu_ref(dims, n, True)
        for r in (r64, r32):
            for unit in (C.PLANT_ZERO, C.PLANT_DEAD):
                assert int(torch.count_nonzero(r["dW0"][unit])) == 0 and float(r["db0"][unit]) == 0.0
        assert int(torch.count_nonzero(r64["dW0"])) > 0


# ---- the predictor ---------------------------------------------------------------------------------------------------
def test_predicted_products_of_the_documented_arrangements():
    net = C.NETS["skip2"]
    dims, L = net.dims, len(net.dims)
    pm = C.pair_masks(net)
    every = pm["all"][0]
    hidden = [(128, o, i, True, True) for o, i in reversed(dims[:-1])]
    # all on at (16, 48, 16): none from the row node's hidden layers, its last layer, the owner's last layer, four
    # owner products with K = 128 and addends
    assert C.predicted_products(dims, every, 64, rows=(16, 48), merge=True) == [(48, 9, 64, False, False),
                                                                               (64, 9, 64, False, False)] + hidden
    # unmerged: the row node's u^T v-bar upwards and z-bar^T a downwards over its 48 rows, the owner's without addends
    loose = [(48, o, i, False, False) for o, i in dims]
    assert C.predicted_products(dims, every, 64, rows=(16, 48), merge=False) == \
        loose[:-1] + loose[::-1] + [(64, 9, 64, False, False)] + [(k, m, n, False, False) for k, m, n, _, _ in hidden]
    # frozen layer 2 on both nodes: no product for it, the other hidden layers still merge
    got = C.predicted_products(dims, *pm["w2_frozen"][:1], 64, rows=(16, 48), merge=True, row_mask=pm["w2_frozen"][1])
    assert got == [(48, 9, 64, False, False), (64, 9, 64, False, False), hidden[0], hidden[2], hidden[3]]
    assert sum(1 for p in got if p[0] == 128) == 3
    # layer 1 frozen on the row node only: nothing merges, the row node forms no product for layer 1
    got = C.predicted_products(dims, *pm["w1_frozen_on_rows"][:1], 64, rows=(16, 48), merge=True,
                               row_mask=pm["w1_frozen_on_rows"][1])
    assert not any(p[3] or p[4] for p in got) and sum(1 for p in got if p[0] == 48) == 2 * 3 + 1
    assert C.row_detached(pm["w1_frozen_on_rows"]) == (1,) and C.row_detached(pm["w2_frozen"]) == ()
    assert (48, 37, 64, False, False) not in got and (128, 37, 64, False, False) in got
    # one node: stacked hidden layers over 2N rows, the last layer over N; a frozen layer has none
    assert C.predicted_products(dims, every, 7) == [(7, 9, 64, False, False)] + [(14, o, i, False, False)
                                                                                for o, i in reversed(dims[:-1])]
    assert C.predicted_products(dims, C.masks(net)["w_none"], 7) == []
    assert C.predicted_products(dims, C.masks(net)["w_last_only"], 7) == [(7, 9, 64, False, False)]
    assert C.predicted_products(C.NETS["depth0"].dims, every._replace(w=(True,), b=(True,)), 33) == [(33, 9, 27, False, False)]
    assert L == 5
