"""Hyper-parameter schedules in the graph-captured training step: lr / betas (ClipAdam, hm_adam_step_dev) and the loss
weights / alpha (hm_idr_loss_dev) are read by the replayed kernels when they run, and what a replay cannot follow
raises before any replay.  Under ops.deterministic() a captured run and an eager run of the same schedule agree bit for
bit."""
import os
import socket
import tempfile

import numpy as np
import pytest
import torch

import bench
from helpers import idr_conf

pytestmark = pytest.mark.gpu


def _setup(seed=3):
    from hashmodnffbanks_idr_amd.model.implicit_differentiable_renderer import IDRNetwork
    from hashmodnffbanks_idr_amd.model.loss import IDRLoss
    torch.manual_seed(seed)
    model = IDRNetwork(idr_conf("C1")).cuda()
    with torch.no_grad():  # let the hash features matter
        model.implicit_network.lin0.weight_v[:, 3:].normal_(0, 0.02)
        model.implicit_network.embed_model.embedder_obj.table.uniform_(-0.05, 0.05)
    model.train()
    inp, gt = bench.synthetic_batch(21, 512, "cuda")
    rs = np.random.RandomState(4)
    inp["object_mask"] = torch.from_numpy(rs.uniform(0, 1, (1, 512)) < 0.8).cuda()
    gt["rgb"] = torch.from_numpy(rs.uniform(-1, 1, (1, 512, 3)).astype(np.float32)).cuda()
    return model, IDRLoss(eikonal_weight=0.1, mask_weight=100.0, alpha=50.0), inp, gt


def _params(model):
    torch.cuda.synchronize()
    return {n: p.detach().clone() for n, p in model.named_parameters()}


def _assert_frozen(model, snap):
    for n, p in _params(model).items():
        assert torch.equal(p, snap[n]), f"{n} moved"


def _stepper(model, loss_fn, opt, **kw):
    from hashmodnffbanks_idr_amd.training.graph_step import GraphedTrainStep
    return GraphedTrainStep(model, loss_fn, opt, warmup=2, **kw)


def test_lr_zero_freezes_the_parameters_of_replayed_steps():
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    model, loss_fn, inp, gt = _setup()
    opt = ClipAdam(model.parameters(), lr=1e-4)
    stepper = _stepper(model, loss_fn, opt)
    torch.manual_seed(9)
    for _ in range(4):
        stepper.step(inp, gt)
    assert stepper.g_fb is not None, "graph capture fell back to eager"
    opt.param_groups[0]["lr"] = 0.0
    snap = _params(model)
    for _ in range(3):
        stepper.step(inp, gt)
    _assert_frozen(model, snap)
    opt.param_groups[0]["lr"] = 1e-4
    stepper.step(inp, gt)
    after = _params(model)
    assert any(not torch.equal(after[n], snap[n]) for n in snap), "restoring lr did not move the parameters"


def _scheduled_run(use_graph, schedule, steps=10):
    """(per-step loss terms, final parameters) of a deterministic run; schedule(opt, loss_fn) -> callback(i) run after
    step i (0-based), or None"""
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    model, loss_fn, inp, gt = _setup()
    opt = ClipAdam(model.parameters(), lr=1e-4, max_norm=1.0)
    after_step = schedule(opt, loss_fn) if schedule else None
    stepper = _stepper(model, loss_fn, opt, use_graph=use_graph, deterministic=True)
    torch.manual_seed(9)
    trace = []
    for i in range(steps):
        _, lo = stepper.step(inp, gt)
        trace.append({k: v.clone() for k, v in lo.items()})
        if after_step:
            after_step(i)
    assert stepper.g_fb is not None or not use_graph, "graph capture fell back to eager"
    return trace, _params(model)


def _assert_same_runs(a, b):
    (ta, pa), (tb, pb) = a, b
    for i, (x, y) in enumerate(zip(ta, tb)):
        for k in x:
            assert torch.equal(x[k], y[k]), f"step {i}: {k} {x[k].item()} != {y[k].item()}"
    for n in pa:
        assert torch.equal(pa[n], pb[n]), f"parameter {n}: max |d| = {(pa[n] - pb[n]).abs().max().item():.3e}"


def _reference_schedule(opt, loss_fn):
    """the reference runner's: MultiStepLR stepped every step, alpha doubled at its milestones
    (training/idr_train.py:131,175-179,227-228,330)"""
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[4, 7], gamma=0.5)

    def after_step(i):
        sched.step()
        if i + 1 in (5, 8):
            loss_fn.alpha *= 2
    return after_step


def test_constant_schedule_captured_equals_eager_bitwise():
    _assert_same_runs(_scheduled_run(True, None), _scheduled_run(False, None))


def test_reference_schedule_captured_equals_eager_bitwise():
    _assert_same_runs(_scheduled_run(True, _reference_schedule), _scheduled_run(False, _reference_schedule))


def test_one_cycle_lr_with_momentum_captured_equals_eager_bitwise():
    def one_cycle(opt, loss_fn):
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, total_steps=12, cycle_momentum=True)
        betas = []

        def after_step(i):
            betas.append(opt.param_groups[0]["betas"][0])
            sched.step()
            if i == 9:
                assert len(set(betas)) > 3, betas     # beta1 really moved
        return after_step
    _assert_same_runs(_scheduled_run(True, one_cycle), _scheduled_run(False, one_cycle))


def test_loss_values_changed_after_capture_are_followed():
    from hashmodnffbanks_idr_amd.model.loss import idr_loss_terms_torch
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    model, loss_fn, inp, gt = _setup()
    stepper = _stepper(model, loss_fn, ClipAdam(model.parameters(), lr=1e-4))
    torch.manual_seed(9)
    for _ in range(3):
        stepper.step(inp, gt)
    assert stepper.g_fb is not None
    loss_fn.alpha, loss_fn.mask_weight, loss_fn.eikonal_weight = 80.0, 30.0, 0.7
    out, lo = stepper.step(inp, gt)
    ref = idr_loss_terms_torch(out, gt["rgb"], 0.7, 30.0, 80.0)
    for k in ("loss", "eikonal_loss", "mask_loss"):
        np.testing.assert_allclose(lo[k].item(), ref[k].item(), rtol=3e-6, atol=1e-7, err_msg=k)


def _captured(opt_factory, steps=3):
    model, loss_fn, inp, gt = _setup()
    opt = opt_factory(model)
    stepper = _stepper(model, loss_fn, opt)
    torch.manual_seed(9)
    for _ in range(steps):
        stepper.step(inp, gt)
    assert stepper.g_fb is not None
    return model, loss_fn, opt, stepper, inp, gt


def test_float_lr_of_capturable_torch_adam_changed_after_capture_raises():
    model, _, opt, stepper, inp, gt = _captured(lambda m: torch.optim.Adam(m.parameters(), lr=1e-4, capturable=True))
    opt.param_groups[0]["lr"] = 5e-5
    snap = _params(model)
    with pytest.raises(RuntimeError, match="lr=torch.tensor"):
        stepper.step(inp, gt)
    _assert_frozen(model, snap)


def test_tensor_lr_of_capturable_torch_adam_follows_multistep_lr():
    model, _, opt, stepper, inp, gt = _captured(
        lambda m: torch.optim.Adam(m.parameters(), lr=torch.tensor(1e-4, device="cuda"), capturable=True))
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.0)
    sched.step()                                  # lr tensor filled with 0 in place
    assert opt.param_groups[0]["lr"].item() == 0.0
    snap = _params(model)
    for _ in range(2):
        stepper.step(inp, gt)
    _assert_frozen(model, snap)


def test_max_norm_turned_on_after_a_capture_without_clipping_raises():
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    model, _, opt, stepper, inp, gt = _captured(lambda m: ClipAdam(m.parameters(), lr=1e-4, max_norm=0.0))
    opt.max_norm = 1.0
    snap = _params(model)
    with pytest.raises(RuntimeError, match="max_norm"):
        stepper.step(inp, gt)
    _assert_frozen(model, snap)
    opt.max_norm = 0.0
    stepper.step(inp, gt)          # back to what was captured: replays again


def test_max_norm_turned_off_after_capture_is_followed():
    """captured with clipping, max_norm 0 afterwards: the device value gives clip coefficient 1 (no clipping)"""
    runs = []
    for use_graph in (True, False):
        def off_after_4(opt, loss_fn):
            def after_step(i):
                if i == 3:
                    opt.max_norm = 0.0
            return after_step
        runs.append(_scheduled_run(use_graph, off_after_4, steps=6))
    _assert_same_runs(*runs)


def test_clip_adam_load_state_dict_after_capture_raises():
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    _, _, opt, _, _, _ = _captured(lambda m: ClipAdam(m.parameters(), lr=1e-4))
    sd = opt.state_dict()
    with pytest.raises(RuntimeError, match="load_state_dict"):
        opt.load_state_dict(sd)


@pytest.mark.parametrize("what", ["lr", "beta", "alpha"])
def test_invalid_values_raise_value_error_before_anything_runs(what):
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    model, loss_fn, opt, stepper, inp, gt = _captured(lambda m: ClipAdam(m.parameters(), lr=1e-4))
    if what == "lr":
        opt.param_groups[0]["lr"] = -1e-4
    elif what == "beta":
        opt.param_groups[0]["betas"] = (1.0, 0.999)
    else:
        loss_fn.alpha = 0.0
    snap = _params(model)
    with pytest.raises(ValueError):
        stepper.step(inp, gt)
    _assert_frozen(model, snap)


# ---- the entry points ---------------------------------------------------------------------------------------------
HYPERS = [(1e-3, 0.9, 0.999, 1e-8, 1.0), (0.0, 0.9, 0.999, 1e-8, 1.0), (2e-4, 0.5, 0.9, 1e-6, 0.0),
          (5e-3, 0.0, 0.0, 0.0, 0.05), (3e-4, 0.95, 0.99, 1e-8, 1e9)]


def _adam_run(sizes, hp, dev_hyper, clip, seed):
    import ctypes as C
    from hashmodnffbanks_idr_amd import _lib
    g = torch.Generator().manual_seed(seed)
    ts = [[torch.randn(n, generator=g).cuda() * s for s in (1.0, 0.3, 0.1)] + [torch.rand(n, generator=g).cuda() * 0.01]
          for n in sizes]
    steps = torch.tensor([3 + i for i in range(len(sizes))], dtype=torch.int64, device="cuda")
    table = (_lib.AdamTensor * len(sizes))()
    for i, (p, gr, m, v) in enumerate(ts):
        table[i] = _lib.AdamTensor(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), steps.data_ptr() + 8 * i,
                                   p.numel())
    L = _lib.lib()
    scratch = torch.zeros(_lib.check(L.hm_adam_scratch_floats(C.cast(table, C.c_void_p), len(sizes))), device="cuda")
    hyper = torch.tensor(hp, dtype=torch.float32, device="cuda")
    for _ in range(2):
        if dev_hyper:
            _lib.check(L.hm_adam_step_dev(C.cast(table, C.c_void_p), len(sizes), _lib.dptr(hyper), int(clip),
                                          _lib.dptr(scratch), _lib.stream_ptr(hyper)))
        else:
            _lib.check(L.hm_adam_step(C.cast(table, C.c_void_p), len(sizes), *hp, _lib.dptr(scratch),
                                      _lib.stream_ptr(hyper)))
    torch.cuda.synchronize()
    return [t for row in ts for t in row] + [steps]


@pytest.mark.parametrize("sizes", [[1], [3, 8192, 5], [8195, 1027, 16, 7], [70001] + [13] * 70])
@pytest.mark.parametrize("hp", HYPERS)
def test_adam_step_dev_equals_adam_step(sizes, hp):
    ref = _adam_run(sizes, hp, False, False, seed=len(sizes))
    for clip in ({hp[4] > 0, True} if hp[4] <= 0 else {True}):     # clipping on with a device max_norm of 0: coef 1
        got = _adam_run(sizes, hp, True, clip, seed=len(sizes))
        for i, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), (i, clip)


@pytest.mark.parametrize("n,m", [(2048, 3072), (777, 0), (1, 1), (301, 455)])
@pytest.mark.parametrize("w", [(0.1, 100.0, 50.0), (0.7, 30.0, 200.0), (0.0, 0.0, 1e-3)])
def test_idr_loss_dev_equals_idr_loss(n, m, w):
    from hashmodnffbanks_idr_amd.model import loss as L
    g = torch.Generator().manual_seed(n + m)
    leaves = (torch.rand(n, 3, generator=g), torch.randn(n, 1, generator=g) * 0.05, torch.randn(m, 3, generator=g))
    gt = torch.rand(1, n, 3, generator=g).cuda()
    hit, inside = (torch.rand(n, generator=g) > 0.4).cuda(), (torch.rand(n, generator=g) > 0.3).cuda()
    res = []
    for hyper in (None, torch.tensor(w, dtype=torch.float32, device="cuda")):
        rgb, sdf, grad = (t.cuda().requires_grad_(True) for t in leaves)
        out = {"rgb_values": rgb, "sdf_output": sdf, "grad_theta": grad, "network_object_mask": hit,
               "object_mask": inside}
        lo = L.idr_loss_terms(out, gt, *w) if hyper is None else L.idr_loss_terms(out, gt, hyper=hyper)
        (lo["loss"] * 1.7).backward()
        res.append([lo[k].detach() for k in ("loss", "rgb_loss", "eikonal_loss", "mask_loss")]
                   + [t.grad if t.grad is not None else torch.zeros(0) for t in (rgb, sdf, grad)])
    for i, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), i


# ---- data parallel ------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HM_DIST_BACKEND="gloo")
    from hashmodnffbanks_idr_amd import parallel
    from hashmodnffbanks_idr_amd.model.implicit_differentiable_renderer import IDRNetwork
    from hashmodnffbanks_idr_amd.model.loss import IDRLoss
    from hashmodnffbanks_idr_amd.training.graph_step import GraphedTrainStep
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    parallel.init_distributed()
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    model = IDRNetwork(idr_conf("C1")).cuda()
    with torch.no_grad():
        model.implicit_network.lin0.weight_v[:, 3:].normal_(0, 0.02)
        model.implicit_network.embed_model.embedder_obj.table.uniform_(-0.05, 0.05)
    model.train()
    inp, gt = bench.synthetic_batch(1234 + rank, 512, "cuda")
    rs = np.random.RandomState(40 + rank)
    inp["object_mask"] = torch.from_numpy(rs.uniform(0, 1, (1, 512)) < 0.8).cuda()
    gt["rgb"] = torch.from_numpy(rs.uniform(-1, 1, (1, 512, 3)).astype(np.float32)).cuda()
    opt = ClipAdam(model.parameters(), lr=1e-4, max_norm=1.0)
    reducer = parallel.StaticGradExchange(model.parameters(),
                                          tables=[model.implicit_network.embed_model.embedder_obj,
                                                  model.rendering_network.embed_model.embedder_obj])
    stepper = GraphedTrainStep(model, IDRLoss(eikonal_weight=0.1, mask_weight=100.0, alpha=50.0), opt, reducer,
                               warmup=2, deterministic=True)
    torch.manual_seed(100 + rank)
    for _ in range(4):
        stepper.step(inp, gt)
    torch.cuda.synchronize()
    moving = {n: p.detach().cpu() for n, p in model.named_parameters()}
    opt.param_groups[0]["lr"] = 0.0
    for _ in range(3):
        stepper.step(inp, gt)
    reducer.check()
    torch.cuda.synchronize()
    rec = {"graph": stepper.g_fb is not None, "at_step4": moving,
           "params": {n: p.detach().cpu() for n, p in model.named_parameters()}}
    torch.save(rec, os.path.join(out_dir, f"rank{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_gloo_ranks_freeze_together_when_lr_drops_to_zero():
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_dp_worker, args=(2, _free_port(), d), nprocs=2, join=True)
        r = [torch.load(os.path.join(d, f"rank{k}.pt"), weights_only=False) for k in range(2)]
    assert r[0]["graph"] and r[1]["graph"]
    for n, p in r[0]["params"].items():
        assert torch.equal(p, r[0]["at_step4"][n]), f"rank 0: {n} moved with lr 0"
        assert torch.equal(p, r[1]["params"][n]), f"replicas differ in {n}"
