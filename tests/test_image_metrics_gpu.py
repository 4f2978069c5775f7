"""The device image metrics (csrc/hm_image.hip, ops.image_psnr / image_ssim, evaluation.images) against the float64
reference of tests/image_cases.py.

Bounds.  SSIM, 1e-10 on |map - ref| and on the mean: an fp64 weighted sum of win^2 <= 961 terms with weights summing to
1 carries an absolute error of at most about win^2 2^-53 L^2; the variance terms are divided by at least C2 = 9e-4 L^2,
which puts each factor's relative error under about 1.5e-11 at win = 11.  PSNR, 1e-12 relative on the mse: an fp64 sum
of at most a few ten thousand squares of exactly formed differences, n 2^-53 << 1e-12."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import image_cases as IC
from hashmodnffbanks_idr_amd import _lib, ops
from hashmodnffbanks_idr_amd.evaluation import render_view, view_metrics
from hashmodnffbanks_idr_amd.utils import general as utils

pytestmark = pytest.mark.gpu

TILE = ops.SSIM_TILE
SSIM_BOUND = 1e-10
MSE_BOUND = 1e-12


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # a copy: the shared inputs are read-only


# ---- SSIM ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IC.ssim_cases(TILE)))
def test_ssim_against_the_direct_reference(name):
    x, y, (want, want_map), win, L = IC.ssim_case(name, TILE)
    dx, dy = _dev(x), _dev(y)
    got, got_map = ops.image_ssim(dx, dy, data_range=L, win=win, return_map=True)
    assert got.dtype == got_map.dtype == torch.float64 and got.shape == (x.shape[0],)
    assert tuple(got_map.shape) == want_map.shape
    e_map = np.abs(got_map.cpu().numpy() - want_map).max()
    e_mean = np.abs(got.cpu().numpy() - want).max()
    print(f"ssim {name} {x.shape} win {win} L {L}: map {e_map:.3e} mean {e_mean:.3e}")
    assert e_map <= SSIM_BOUND and e_mean <= SSIM_BOUND
    alone = ops.image_ssim(dx, dy, data_range=L, win=win)              # without the map: the same bits
    assert torch.equal(alone, got)
    if x.shape[0] == 1:                                                # [H, W, C] is B = 1
        assert torch.equal(ops.image_ssim(dx[0], dy[0], data_range=L, win=win), got)


@pytest.mark.parametrize("name", ["one_position", "edge_17x17", "two_tiles_each_way", "win3", "win31"])
def test_ssim_exactness_and_repeatability(name):
    x, y, _, win, L = IC.ssim_case(name, TILE)
    dx, dy = _dev(x), _dev(y)
    one, one_map = ops.image_ssim(dx, dx.clone(), data_range=L, win=win, return_map=True)
    assert bool((one == 1.0).all()) and bool((one_map == 1.0).all())
    a, a_map = ops.image_ssim(dx, dy, data_range=L, win=win, return_map=True)
    b, b_map = ops.image_ssim(dx, dy, data_range=L, win=win, return_map=True)
    assert torch.equal(a, b) and torch.equal(a_map, b_map) and not bool((a == 1.0).any())


def test_ssim_parameters_reach_the_kernel():
    x, y = IC.make_pair("params", 2, 20, 23, 3, 1.0, "noise")
    dx, dy = _dev(x), _dev(y)
    for sigma, win in ((0.8, 5), (3.0, 11)):
        want, want_map = IC.ssim_ref(x, y, 1.0, win, sigma)
        got, got_map = ops.image_ssim(dx, dy, win=win, sigma=sigma, return_map=True)
        assert np.abs(got_map.cpu().numpy() - want_map).max() <= SSIM_BOUND
        assert np.abs(got.cpu().numpy() - want).max() <= SSIM_BOUND
    base = ops.image_ssim(dx, dy)
    assert not torch.equal(ops.image_ssim(dx, dy, k1=0.05), base) and not torch.equal(ops.image_ssim(dx, dy, k2=0.1), base)
    # scaling the data and the range together (by a power of two: exact in fp32) changes nothing but C1's and C2's rounding
    assert (ops.image_ssim(dx * 256, dy * 256, data_range=256.0) - base).abs().max().item() <= SSIM_BOUND


# ---- PSNR ------------------------------------------------------------------------------------------------------
def _check_psnr(got, x, y, mask, L, what):
    want, mse, n = IC.psnr_ref(x, y, mask, L)
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape
    for b in range(len(want)):
        if n[b] == 0:
            assert np.isnan(got[b]), what
        elif mse[b] == 0:
            assert np.isposinf(got[b]), what
        else:
            got_mse = L * L * 10.0 ** (-got[b] / 10.0)
            rel = abs(got_mse / mse[b] - 1.0)
            print(f"psnr {what} [{b}]: {got[b]:.6f} dB, mse rel {rel:.3e}")
            assert rel <= MSE_BOUND, what


@pytest.mark.parametrize("name", sorted(IC.psnr_cases(ops.SQERR_PIXELS)))
def test_psnr_against_the_reference(name):
    B, H, W, Cn, L = IC.psnr_cases(ops.SQERR_PIXELS)[name]
    x, y = IC.make_pair("psnr_" + name, B, H, W, Cn, L, "noise")
    dx, dy = _dev(x), _dev(y)
    _check_psnr(ops.image_psnr(dx, dy, data_range=L), x, y, None, L, name)
    mask = IC.psnr_masks(name, B, H, W)
    as_bool = ops.image_psnr(dx, dy, mask=_dev(mask), data_range=L)
    _check_psnr(as_bool, x, y, mask, L, name + " bool mask")
    as_u8 = ops.image_psnr(dx, dy, mask=_dev(mask.astype(np.uint8) * 255), data_range=L)
    assert torch.equal(as_u8.nan_to_num(nan=-1.0), as_bool.nan_to_num(nan=-1.0))
    if B >= 2:
        assert math.isnan(as_bool[0].item()) and torch.equal(as_bool[1], ops.image_psnr(dx, dy, data_range=L)[1])
    if B == 1:
        assert torch.equal(ops.image_psnr(dx[0], dy[0], mask=_dev(mask[0]), data_range=L), as_bool)
    # exactness and repeatability
    assert bool(torch.isposinf(ops.image_psnr(dx, dx.clone(), data_range=L)).all())
    assert bool(torch.isnan(ops.image_psnr(dx, dy, mask=torch.zeros(B, H, W, dtype=torch.bool, device="cuda"))).all())
    again = ops.image_psnr(dx, dy, mask=_dev(mask), data_range=L)
    assert torch.equal(again.nan_to_num(nan=-1.0), as_bool.nan_to_num(nan=-1.0))


# ---- memory discipline -----------------------------------------------------------------------------------------
def _window(a, pad):
    """a copy of `a` placed `pad` elements inside a NaN-filled buffer: (view, buffer)"""
    buf = torch.full((a.size + 2 * pad,), float("nan"), device="cuda")
    view = buf[pad:pad + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    return view, buf


@pytest.mark.parametrize("name", ["edge_15x17", "two_tiles_each_way", "win31"])
def test_nothing_outside_the_images_is_read(name):
    x, y, _, win, L = IC.ssim_case(name, TILE)
    (vx, _), (vy, _) = _window(x, 1000), _window(y, 1000)
    assert vx.is_contiguous() and vy.is_contiguous()
    clean, clean_map = ops.image_ssim(_dev(x), _dev(y), data_range=L, win=win, return_map=True)
    got, got_map = ops.image_ssim(vx, vy, data_range=L, win=win, return_map=True)
    assert torch.equal(got, clean) and torch.equal(got_map, clean_map)
    B, H, W, _ = x.shape
    mask = IC.psnr_masks(name, B, H, W)
    want = ops.image_psnr(_dev(x), _dev(y), mask=_dev(mask), data_range=L)
    hole = ~torch.from_numpy(mask).cuda()
    vx[hole] = float("nan")                                            # pixels outside the mask are not read either
    vy[hole] = float("nan")
    got = ops.image_psnr(vx, vy, mask=_dev(mask), data_range=L)
    assert torch.equal(got.nan_to_num(nan=-1.0), want.nan_to_num(nan=-1.0))
    has_hole = hole.flatten(1).any(1)                                  # without the mask those NaNs are read, and show
    assert bool(has_hole.any()) and bool(torch.isnan(ops.image_psnr(vx, vy, data_range=L))[has_hole].all())


@pytest.mark.parametrize("name", ["edge_17x15", "two_tiles_each_way", "win31_c1"])
def test_writes_stay_inside_their_buffers(name):
    x, y, (want, want_map), win, L = IC.ssim_case(name, TILE)
    B, H, W, Cn = x.shape
    lib = _lib.lib()
    sentinel = -7.25e30
    dx, dy = _dev(x), _dev(y)
    weights = torch.from_numpy(ops.ssim_window(win, 1.5)).cuda()
    n_map = want_map.size
    ws_bytes = lib.hm_image_ssim_workspace_bytes(B, H, W, win)
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    map_buf = torch.full((n_map + 64,), sentinel, dtype=torch.float64, device="cuda")
    out_buf = torch.full((B + 64,), sentinel, dtype=torch.float64, device="cuda")
    ws_buf = torch.full((ws_bytes // 8 + 64,), sentinel, dtype=torch.float64, device="cuda")
    smap, out, ws = map_buf[32:32 + n_map], out_buf[32:32 + B], ws_buf[32:32 + ws_bytes // 8]
    _lib.check(lib.hm_image_ssim(_lib.dptr(dx), _lib.dptr(dy), B, H, W, Cn, win, _lib.dptr(weights), (IC.K1 * L) ** 2,
                                 (IC.K2 * L) ** 2, _lib.dptr(smap), _lib.dptr(ws), _lib.dptr(out), _lib.stream_ptr(dx)))
    torch.cuda.synchronize()
    assert np.abs(smap.cpu().numpy().reshape(want_map.shape) - want_map).max() <= SSIM_BOUND
    assert np.abs(out.cpu().numpy() - want).max() <= SSIM_BOUND
    for buf, n in ((map_buf, n_map), (out_buf, B), (ws_buf, ws_bytes // 8)):
        assert bool((buf[:32] == sentinel).all()) and bool((buf[32 + n:] == sentinel).all())
        assert not bool((buf[32:32 + n] == sentinel).any())
    # the squared-error sums: out [B, 2] and its partials
    ws_bytes = lib.hm_image_sqerr_workspace_bytes(B, H, W)
    out_buf = torch.full((2 * B + 64,), sentinel, dtype=torch.float64, device="cuda")
    ws_buf = torch.full((ws_bytes // 8 + 64,), sentinel, dtype=torch.float64, device="cuda")
    out, ws = out_buf[32:32 + 2 * B], ws_buf[32:32 + ws_bytes // 8]
    mask = IC.psnr_masks(name, B, H, W)
    _lib.check(lib.hm_image_sqerr(_lib.dptr(dx), _lib.dptr(dy), _lib.dptr(_dev(mask)), B, H, W, Cn, _lib.dptr(ws),
                                  _lib.dptr(out), _lib.stream_ptr(dx)))
    torch.cuda.synchronize()
    _, mse, n = IC.psnr_ref(x, y, mask, L)
    got = out.cpu().numpy().reshape(B, 2)
    assert np.array_equal(got[:, 1], n)
    live = n > 0
    assert np.all(np.abs(got[live, 0] / (n[live] * Cn) / mse[live] - 1.0) <= MSE_BOUND) and np.all(got[~live, 0] == 0)
    for buf, n_el in ((out_buf, 2 * B), (ws_buf, ws_bytes // 8)):
        assert bool((buf[:32] == sentinel).all()) and bool((buf[32 + n_el:] == sentinel).all())
        assert not bool((buf[32:32 + n_el] == sentinel).any())


# ---- evaluation.images -------------------------------------------------------------------------------------------
def test_view_metrics_is_the_reference_convention():
    H, W = 21, 30
    rng = np.random.default_rng(5)
    gt = rng.uniform(-1, 1, (H * W, 3)).astype(np.float32)
    pred = (gt + 0.2 * rng.standard_normal((H * W, 3))).astype(np.float32)          # leaves [-1, 1] in places
    assert (np.abs(pred) > 1).any()
    mask = np.zeros((H, W), bool)
    mask[3:17, 5:26] = rng.random((14, 21)) < 0.9
    psnr, ssim = view_metrics(_dev(pred), _dev(gt), _dev(mask.reshape(-1)), (H, W))
    assert psnr.dtype == ssim.dtype == torch.float64 and psnr.shape == ssim.shape == ()
    p = np.clip((pred.reshape(H, W, 3) + np.float32(1)) / np.float32(2), 0, 1)     # fp32, as on the device
    g = (gt.reshape(H, W, 3) + np.float32(1)) / np.float32(2)
    m3 = mask[..., None]
    want_psnr, mse, _ = IC.psnr_ref((p * m3)[None], (g * m3)[None], mask[None], 1.0)
    got_mse = 10.0 ** (-psnr.item() / 10.0)
    assert abs(got_mse / mse[0] - 1.0) <= MSE_BOUND and abs(psnr.item() - want_psnr[0]) < 1e-9
    want_ssim, _ = IC.ssim_ref(np.where(m3, p, np.float32(1))[None], np.where(m3, g, np.float32(1))[None], 1.0, 11)
    assert abs(ssim.item() - want_ssim[0]) <= SSIM_BOUND
    # [1, H*W, 3] inputs, and an empty mask: nan and the SSIM of two white images
    psnr, ssim = view_metrics(_dev(pred)[None], _dev(gt)[None], _dev(np.zeros(H * W, bool)), (H, W))
    assert math.isnan(psnr.item()) and ssim.item() == 1.0


def _aimed_view(H, W, stride):
    """a H x W view through the first camera of tests/golden/dummy_scan0: its intrinsics and its centre, turned to look
    at the origin, the pixels `stride` apart around the principal point - so that the middle of the view meets the
    surface whatever part of the 1200 x 1600 frame the scan's own pose looks at"""
    from hashmodnffbanks_idr_amd.utils import rend_util
    cams = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dummy_scan0", "cameras.npz"))
    P = (cams["world_mat_0"].astype(np.float32) @ cams["scale_mat_0"].astype(np.float32))[:3, :4]
    intrinsics, pose = rend_util.load_K_Rt_from_P(None, P)
    centre = pose[:3, 3].astype(np.float64)
    z = -centre / np.linalg.norm(centre)
    xa = np.cross([0.0, 0.0, 1.0], z)
    xa /= np.linalg.norm(xa)
    pose = pose.copy()
    pose[:3, :3] = np.stack([xa, np.cross(z, xa), z], 1).astype(np.float32)
    rows, cols = np.mgrid[0:H, 0:W].astype(np.float32)
    uv = np.stack([intrinsics[0, 2] + (cols - (W - 1) / 2) * stride, intrinsics[1, 2] + (rows - (H - 1) / 2) * stride], -1)
    return {"uv": torch.from_numpy(uv.reshape(1, H * W, 2).astype(np.float32)).cuda(),
            "intrinsics": torch.from_numpy(intrinsics.astype(np.float32))[None].cuda(),
            "pose": torch.from_numpy(pose.astype(np.float32))[None].cuda(),
            "object_mask": torch.ones(1, H * W, dtype=torch.bool, device="cuda")}


def test_render_view_on_a_real_model(golden):
    """render_view against the loop written by hand, bit for bit.  Both run under ops.deterministic(): the normals of
    the rendering pass go through split-K GEMMs whose default kernels add with fp32 atomics, so that without the mode
    two runs of the very same loop differ in the last bits (DESIGN.md "Deterministic mode")."""
    from helpers import make_idr
    g = golden("idr_step_C2")
    model = make_idr("C2", int(g["seed"]), float(g["bias"]) if "bias" in g.files else 0.6).train()
    H, W = 20, 24
    inp = _aimed_view(H, W, stride=60.0)
    with ops.deterministic():
        rgb, hit = render_view(model, inp, H * W, chunk=128)
    assert model.training and rgb.shape == (1, H * W, 3) and hit.shape == (1, H * W) and hit.dtype == torch.bool
    assert not rgb.requires_grad
    n_hit = int(hit.sum())
    print(f"render_view: {n_hit} of {H * W} rays meet the surface")
    assert n_hit > 0                                    # a view of background only shows nothing
    assert bool((rgb[~hit] == 1.0).all()) and not bool((rgb[hit] == 1.0).all())
    model.eval()
    with ops.deterministic(), torch.no_grad():
        res = []
        for part in utils.split_input(inp, H * W, n_pixels=128):
            out = model(part)
            res.append({"rgb_values": out["rgb_values"].detach(),
                        "network_object_mask": out["network_object_mask"].detach()})
        want = utils.merge_output(res, H * W, 1)
    assert len(res) == 4 and res[-1]["rgb_values"].shape[0] == 96
    assert torch.equal(hit, want["network_object_mask"].reshape(1, H * W))
    diff = (rgb - want["rgb_values"].reshape(1, H * W, 3)).abs()
    print(f"render_view vs the loop: {int((diff != 0).sum())} values differ, largest {diff.max().item():.3e}")
    assert torch.equal(rgb, want["rgb_values"].reshape(1, H * W, 3))
    # and the scores of that view against itself shifted: finite numbers from the device
    psnr, ssim = view_metrics(rgb[0], rgb[0].roll(1, 0), hit[0], (H, W))
    assert math.isfinite(psnr.item()) and 0.0 < ssim.item() < 1.0
