"""Deterministic mode (ops.deterministic, GraphedTrainStep(deterministic=...)): the library's reductions without fp32
atomics give the same bits on every run - operator by operator, under concurrent load on another stream, and for whole
captured / eager training steps from fresh builds of the same seeded model."""
import os
import socket
import tempfile

import numpy as np
import pytest
import torch

import bench
from helpers import idr_conf

pytestmark = pytest.mark.gpu

REPEATS = 20


def _ops():
    from hashmodnffbanks_idr_amd import ops
    return ops


def _repeat_under_load(fn):
    """fn() REPEATS times, each while a large GEMM runs on a second stream (perturbs workgroup arrival order)"""
    side = torch.cuda.Stream()
    big = torch.randn(4096, 4096, device="cuda")
    outs = []
    for _ in range(REPEATS):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            big @ big
        outs.append(fn().clone())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return outs


def _assert_all_equal(outs):
    for i, o in enumerate(outs[1:], 1):
        assert torch.equal(o, outs[0]), f"repeat {i} differs from the first"


GEMM_CASES = [   # (M, N, K, trans_a, trans_b, accumulate): split-K shapes, both transposes, K tails
    (72, 72, 8192, True, False, False),
    (3, 512, 6144, False, False, False),
    (3, 512, 6144, True, True, True),
    (257, 445, 6000, True, False, True),
    (64, 96, 6000, False, True, False),
    (512, 67, 4096, True, False, False),
]


@pytest.mark.parametrize("M,N,K,ta,tb,acc", GEMM_CASES)
def test_gemm_deterministic_repeats_and_matches_float64(M, N, K, ta, tb, acc):
    ops = _ops()
    g = torch.Generator().manual_seed(M * 7 + N + K)
    a = torch.randn(*((K, M) if ta else (M, K)), generator=g).cuda()
    b = torch.randn(*((N, K) if tb else (K, N)), generator=g).cuda()
    c0 = torch.randn(M, N, generator=g).cuda()
    bias = None if acc else torch.randn(N, generator=g).cuda()

    def run():
        c = c0.clone()
        ops.gemm(a, b, bias, ta, tb, out=c, accumulate=acc)
        return c
    with ops.deterministic():
        outs = _repeat_under_load(run)
    _assert_all_equal(outs)
    A = (a.T if ta else a).double().cpu()
    B = (b.T if tb else b).double().cpu()
    ref = A @ B + (c0.double().cpu() if acc else 0) + (bias.double().cpu() if bias is not None else 0)
    err = (outs[0].double().cpu() - ref).abs().max().item()
    assert err <= 1e-5 * np.sqrt(K) * ref.abs().max().item() + 1e-5, err


def test_gemm_group_tn_deterministic_mixed_shapes():
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    shapes = [(512, 445, 4096), (257, 512, 4096), (4, 512, 2048), (64, 67, 6144), (33, 20, 1000)]   # last: K tail
    probs = []
    for M, N, K in shapes:
        probs.append((torch.randn(K, M, generator=g).cuda(), torch.randn(K, N, generator=g).cuda(),
                      torch.randn(M, N, generator=g).cuda()))

    def run():
        cs = [c.clone() for _, _, c in probs]
        ops.gemm_group_tn([(a, b, c) for (a, b, _), c in zip(probs, cs)])
        return torch.cat([c.flatten() for c in cs])
    with ops.deterministic():
        outs = _repeat_under_load(run)
    _assert_all_equal(outs)
    o = 0
    for (a, b, c), (M, N, K) in zip(probs, shapes):
        ref = a.double().cpu().T @ b.double().cpu() + c.double().cpu()
        got = outs[0][o:o + M * N].reshape(M, N).double().cpu()
        o += M * N
        assert (got - ref).abs().max().item() <= 1e-5 * np.sqrt(K) * ref.abs().max().item() + 1e-5, (M, N, K)


def test_gemm_group_tn_deterministic_terms_into_one_output():
    """two problems of one call adding into the same C (the two terms of one weight gradient) are summed in item order"""
    ops = _ops()
    g = torch.Generator().manual_seed(12)
    a1, b1 = torch.randn(4096, 445, generator=g).cuda(), torch.randn(4096, 512, generator=g).cuda()
    a2, b2 = torch.randn(2048, 445, generator=g).cuda(), torch.randn(2048, 512, generator=g).cuda()
    c0 = torch.randn(445, 512, generator=g).cuda()

    def run():
        c = c0.clone()
        ops.gemm_group_tn([(a1, b1, c), (a2, b2, c)])
        return c
    with ops.deterministic():
        outs = _repeat_under_load(run)
        seq = c0.clone()
        ops.gemm_group_tn([(a1, b1, seq)])
        ops.gemm_group_tn([(a2, b2, seq)])
    _assert_all_equal(outs)
    assert torch.equal(outs[0], seq)
    ref = a1.double().cpu().T @ b1.double().cpu() + a2.double().cpu().T @ b2.double().cpu() + c0.double().cpu()
    assert (outs[0].double().cpu() - ref).abs().max().item() <= 1e-5 * np.sqrt(6144) * ref.abs().max().item() + 1e-5


@pytest.mark.parametrize("kind", ["colsum", "colsum_into", "colsum_into_multi"])
def test_colsums_deterministic_repeat_and_match_float64(kind):
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(M, N, generator=g).cuda() for M, N in ((100000, 257), (2048, 512), (33, 445), (0, 4))]
    base = [torch.randn(x.shape[1], generator=g).cuda() for x in xs]

    def run():
        if kind == "colsum":
            return torch.cat([ops.colsum(x) for x in xs])
        outs = [o.clone() for o in base]
        if kind == "colsum_into":
            for x, o in zip(xs, outs):
                ops.colsum_into(x, o)
        else:
            ops.colsum_into_multi(list(zip(xs, outs)))
        return torch.cat(outs)
    with ops.deterministic():
        outs = _repeat_under_load(run)
    _assert_all_equal(outs)
    ref = torch.cat([x.double().cpu().sum(0) + (0 if kind == "colsum" else o.double().cpu()) for x, o in zip(xs, base)])
    assert (outs[0].double().cpu() - ref).abs().max().item() <= 1e-3


def test_deterministic_tracked_scatter_matches_sorted_dense_and_tracked_rows():
    from hashmodnffbanks_idr_amd import ops, parallel
    from hashmodnffbanks_idr_amd.model.embeddings.hashGridEmbedding import MultiResHashGridMLP
    import params as P
    L, T, b, d = P.CONFIGS["C1"]
    emb = MultiResHashGridMLP(True, 3, L, 2, T, b, d).cuda()
    x = torch.from_numpy(P.make_points(8, 20000, -1.0, 1.0)).cuda()
    d_feat = torch.randn(x.shape[0], L * 2, generator=torch.Generator().manual_seed(3)).cuda()
    dense_ref = ops.encode_bwd_table(emb.desc, x, d_feat, 0, deterministic=True)

    def tracked(det):
        ex = parallel.TouchedRowExchange(emb)
        ex.attach()
        with ops.deterministic(det):
            ex.add(x, d_feat)
        torch.cuda.synchronize()
        n = int(ex.count.item())
        return ex.dense.clone(), n, set(ex.rows[:min(n, ex.cap)].cpu().tolist()), ex.bits.clone()
    runs = [tracked(True) for _ in range(3)]
    atomic = tracked(False)
    emb.grad_collector = None
    for dense, n, rows, bits in runs:
        assert torch.equal(dense, dense_ref)
        assert n == atomic[1] and rows == atomic[2] and len(rows) == n
        assert torch.equal(bits, atomic[3])


# ---- whole steps -------------------------------------------------------------------------------------------------
def _c1_model():
    from hashmodnffbanks_idr_amd.model.implicit_differentiable_renderer import IDRNetwork
    torch.manual_seed(3)
    model = IDRNetwork(idr_conf("C1")).cuda()
    with torch.no_grad():  # let the hash features matter
        model.implicit_network.lin0.weight_v[:, 3:].normal_(0, 0.02)
        model.implicit_network.embed_model.embedder_obj.table.uniform_(-0.05, 0.05)
    model.train()
    inp, gt = bench.synthetic_batch(21, 512, "cuda")
    rs = np.random.RandomState(4)
    inp["object_mask"] = torch.from_numpy(rs.uniform(0, 1, (1, 512)) < 0.8).cuda()
    gt["rgb"] = torch.from_numpy(rs.uniform(-1, 1, (1, 512, 3)).astype(np.float32)).cuda()
    return model, inp, gt


def _c2_model():
    model = bench._build("C2", "cuda", 1e-4)
    inp, gt = bench.synthetic_batch(1234, bench.RAYS_PER_GPU, "cuda")
    gt["rgb"] = torch.from_numpy(np.random.RandomState(7).uniform(-1, 1, (1, bench.RAYS_PER_GPU, 3))
                                 .astype(np.float32)).cuda()
    return model, inp, gt


def _c5_model(golden):
    from helpers import make_idr_nffb
    g = golden("idr_step_C5")
    model = make_idr_nffb(str(g["embed_type"]), int(g["seed"]))
    model.train()
    inp = {k: torch.from_numpy(g[k]).cuda() for k in ("intrinsics", "uv", "pose", "object_mask")}
    return model, inp, {"rgb": torch.from_numpy(g["rgb_gt"]).cuda()}


def _run_steps(make, steps, deterministic=True, use_graph=True):
    """a fresh build of the seeded model, `steps` steps; (per-step outputs + loss terms, final parameters)"""
    from hashmodnffbanks_idr_amd.model.loss import IDRLoss
    from hashmodnffbanks_idr_amd.training.graph_step import GraphedTrainStep
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    model, inp, gt = make()
    opt = ClipAdam(model.parameters(), lr=1e-4, max_norm=1.0)
    stepper = GraphedTrainStep(model, IDRLoss(eikonal_weight=0.1, mask_weight=100.0, alpha=50.0), opt, warmup=2,
                               use_graph=use_graph, deterministic=deterministic)
    torch.manual_seed(9)
    trace = []
    for _ in range(steps):
        out, lo = stepper.step(inp, gt)
        trace.append({**{k: v.clone() for k, v in out.items() if torch.is_tensor(v)},
                      **{"loss." + k: v.clone() for k, v in lo.items()}})
    assert stepper.g_fb is not None or not use_graph, "graph capture fell back to eager"
    torch.cuda.synchronize()
    params = {n: p.detach().clone() for n, p in model.named_parameters()}
    return stepper, trace, params


def _assert_runs_equal(r1, r2):
    (_, t1, p1), (_, t2, p2) = r1, r2
    assert "network_object_mask" in t1[0] and "points" in t1[0]     # the tracer's mask, and cam + dists * dir
    for i, (a, b) in enumerate(zip(t1, t2)):
        for k in a:
            assert torch.equal(a[k], b[k]), f"step {i}: {k} differs between the two runs"
    for n in p1:
        assert torch.equal(p1[n], p2[n]), f"parameter {n} differs between the two runs"


@pytest.mark.parametrize("cfg,steps", [("C1", 30), ("C2", 30)])
def test_captured_steps_are_bitwise_reproducible(cfg, steps):
    make = _c1_model if cfg == "C1" else _c2_model
    r1 = _run_steps(make, steps)
    r2 = _run_steps(make, steps)
    assert r1[0].deterministic
    _assert_runs_equal(r1, r2)


def test_captured_filter_bank_steps_are_bitwise_reproducible(golden):
    make = lambda: _c5_model(golden)  # noqa: E731
    _assert_runs_equal(_run_steps(make, 20), _run_steps(make, 20))


def test_torch_deterministic_flag_turns_the_mode_on():
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        r1 = _run_steps(_c1_model, 10, deterministic=None)
        r2 = _run_steps(_c1_model, 10, deterministic=None)
    finally:
        torch.use_deterministic_algorithms(prev)
    assert r1[0].deterministic and r2[0].deterministic
    _assert_runs_equal(r1, r2)


def test_eager_train_step_under_the_context_is_reproducible():
    from hashmodnffbanks_idr_amd import ops, parallel
    from hashmodnffbanks_idr_amd.model.loss import IDRLoss
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    runs = []
    for _ in range(2):
        model, inp, gt = _c1_model()
        opt = ClipAdam(model.parameters(), lr=1e-4, max_norm=1.0)
        loss_fn = IDRLoss(eikonal_weight=0.1, mask_weight=100.0, alpha=50.0)
        torch.manual_seed(9)
        losses = []
        with ops.deterministic():
            for _ in range(3):
                _, lo = parallel.train_step(model, loss_fn, opt, inp, gt)
                losses.append({k: v.detach().clone() for k, v in lo.items()})
        runs.append((losses, {n: p.detach().clone() for n, p in model.named_parameters()}))
    (l1, p1), (l2, p2) = runs
    for a, b in zip(l1, l2):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    for n in p1:
        assert torch.equal(p1[n], p2[n]), n


def test_deterministic_step_agrees_with_the_default_step():
    """one step each: within the bounds test_graph_step_gpu.py uses between eager and graphed steps"""
    _, ta, pa = _run_steps(_c1_model, 1, deterministic=True, use_graph=False)
    _, tb, pb = _run_steps(_c1_model, 1, deterministic=False, use_graph=False)
    a, b = ta[0]["loss.loss"].item(), tb[0]["loss.loss"].item()
    assert abs(a - b) <= 2e-3 * abs(b) + 1e-6
    for n in pa:
        assert (pa[n] - pb[n]).abs().max().item() <= 5e-4, n


def test_deterministic_graph_contains_no_memset_or_memcpy_nodes(tmp_path):
    import re
    os.environ["HM_GRAPH_DUMP"] = str(tmp_path)
    try:
        stepper, trace, _ = _run_steps(_c1_model, 4)
    finally:
        os.environ.pop("HM_GRAPH_DUMP", None)
    dot = open(tmp_path / "g_fb.dot").read()
    kinds = re.findall(r'label="\{\s*\n?(\w+)\n', dot)
    assert kinds.count("KERNEL") > 100
    assert kinds.count("MEMSET") == 0 and kinds.count("MEMCPY") == 0, kinds
    assert "gemm_part_reduce_kernel" in dot and "colsum_part_reduce_kernel" in dot   # the deterministic kernels ran
    assert "segment_scatter_kernel" in dot
    assert np.isfinite(trace[-1]["loss.loss"].item())


# ---- data parallel -----------------------------------------------------------------------------------------------
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
    for _ in range(5):
        stepper.step(inp, gt)
    reducer.check()
    torch.cuda.synchronize()
    rec = {"graph": stepper.g_fb is not None, "params": {n: p.detach().cpu() for n, p in model.named_parameters()}}
    torch.save(rec, os.path.join(out_dir, f"rank{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_gloo_ranks_deterministic_jobs_give_the_same_parameters():
    import torch.multiprocessing as mp
    jobs = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as d:
            mp.spawn(_dp_worker, args=(2, _free_port(), d), nprocs=2, join=True)
            jobs.append(torch.load(os.path.join(d, "rank0.pt"), weights_only=False))
    assert jobs[0]["graph"] and jobs[1]["graph"]
    for n, p in jobs[0]["params"].items():
        assert torch.equal(p, jobs[1]["params"][n]), n
