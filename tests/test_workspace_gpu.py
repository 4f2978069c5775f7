"""Library scratch memory under graph replay (_lib.Workspace): a buffer a captured graph was recorded on stays allocated
when a later, larger call outgrows it, so the replay writes where it always wrote."""
import numpy as np
import pytest
import torch

import params as P
from helpers import make_implicit

pytestmark = pytest.mark.gpu


def _ptrs(buffers):
    return [t.data_ptr() for t in buffers]


def test_sort_pairs_replays_after_its_workspace_has_grown(monkeypatch):
    from hashmodnffbanks_idr_amd import _lib, ops
    monkeypatch.setattr(ops, "_SORT_WS", _lib.Workspace("sort_pairs"))    # whatever earlier tests sorted, start empty
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(5)
    keys = (torch.randint(0, 1 << 12, (4096,), generator=g) % 1000).to(torch.int32).cuda()      # many equal keys
    big = torch.randint(0, 1 << 20, (1 << 18,), generator=g).to(torch.int32).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.sort_pairs(keys, 12)                                           # warm-up sizes the workspace
    torch.cuda.current_stream().wait_stream(side)
    (captured_on,) = ops._SORT_WS.buffers(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        sk, perm = ops.sort_pairs(keys, 12)
    assert _ptrs(ops._SORT_WS.buffers(dev)) == [captured_on.data_ptr()]    # the capture did not grow it

    bk, bp = ops.sort_pairs(big, 20)                                       # eager and larger: grows
    live, *held = ops._SORT_WS.buffers(dev)
    assert live.numel() > captured_on.numel() and live.data_ptr() != captured_on.data_ptr()
    assert captured_on.data_ptr() in _ptrs(held)                           # still allocated for the graph
    rk, rp = torch.sort(big, stable=True)
    assert torch.equal(bk, rk) and torch.equal(bp, rp)

    sk.zero_()
    perm.zero_()
    graph.replay()
    torch.cuda.synchronize()
    rk, rp = torch.sort(keys, stable=True)
    assert torch.equal(sk, rk) and torch.equal(perm, rp)


def test_ray_tracer_keeps_its_workspace_across_a_larger_evaluation():
    """one RayTracing module serves 512 training rays, then a 4096-ray evaluation, then the 512 rays again: the buffer of
    the first call is held, and the third call gives the first call's points, mask and distances bit for bit"""
    from hashmodnffbanks_idr_amd.model.ray_tracing import RayTracing
    net = make_implicit("tiny", (64,) * 8, 16, 3, 0.1, 0.05, bias=0.6)
    net.eval()
    net.sdf_tile_points = 16    # one SDF tile body for every point, as where test_raytrace_gpu.py asserts equal bits
    dev =torch.device("cuda", torch.cuda.current_device())
    rt = RayTracing(1.0, 5.0e-5, 0.5, 3, 10, 100, 8).cuda()
    rt.steps_override = torch.from_numpy(np.random.RandomState(2).uniform(0, 1, 100).astype(np.float32))

    def trace(n_rays, seed, training):
        cam, dirs = P.make_rays(seed, n_rays)
        om = torch.from_numpy(np.random.RandomState(seed).uniform(0, 1, n_rays) < 0.7).cuda()
        rt.train(training)
        with torch.no_grad():
            return rt(sdf=net.sdf, cam_loc=torch.from_numpy(cam).cuda(), object_mask=om,
                      ray_directions=torch.from_numpy(dirs).cuda())

    p1, m1, d1 = trace(512, 0, True)
    (first,) = rt._ws.buffers(dev)                          # (the device tracer ran: the generic one has no workspace)
    assert 0 < int(m1.sum()) < 512                          # some rays hit the surface, some take the mask-loss search
    trace(4096, 1, False)
    live, *held = rt._ws.buffers(dev)
    assert live.numel() > first.numel() and _ptrs(held) == [first.data_ptr()]
    p3, m3, d3 = trace(512, 0, True)
    assert _ptrs(rt._ws.buffers(dev)) == [live.data_ptr(), first.data_ptr()]
    assert torch.equal(m3, m1) and torch.equal(d3, d1) and torch.equal(p3, p1)
