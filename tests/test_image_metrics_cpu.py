"""The image-metric tests' reference has the properties the GPU tests rely on, the new entry points check their
arguments before they touch the device, the library exports what _lib.py declares, and the view-rendering plumbing of
evaluation.images works on a stub model (runs anywhere)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import image_cases as IC
from hashmodnffbanks_idr_amd import _lib, ops
from hashmodnffbanks_idr_amd.evaluation import images as EI
from hashmodnffbanks_idr_amd.evaluation import evaluate_views, render_view, view_metrics  # noqa: F401


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(12, 27, 3), (33, 18, 3), (40, 40, 3)])
def test_direct_reference_is_the_scipy_formulation(shape):
    """uniform noise: its variances are of the order of L^2/12, so the differences Exx - mx^2 lose no digits and the two
    fp64 formulations agree to a few hundred ulp; on near-constant images (the "blur" content) the same differences
    cancel about (L^2/4)/C2 = 280 times more, which belongs to the GPU tests' bound, not to this one"""
    H, W, Cn = shape
    x, y = IC.make_pair(f"cross_{H}x{W}", 2, H, W, Cn, 255.0, "noise")
    _, direct = IC.ssim_ref(x, y, 255.0, 11)
    sep = IC.ssim_scipy(x, y, 255.0, 11)
    assert direct.shape == sep.shape == (2, H - 10, W - 10, Cn)
    worst = np.abs(direct - sep).max()
    print(shape, "direct vs scipy", worst)
    assert worst <= 1e-13


def test_reference_corner_cases():
    x, y = IC.make_pair("corner", 3, 13, 14, 3, 1.0, "noise")
    mean, smap = IC.ssim_ref(x, x, 1.0, 11)
    assert np.all(smap == 1.0) and np.all(mean == 1.0)
    mean, smap = IC.ssim_ref(x, y, 1.0, 11)
    assert np.all(np.abs(smap) < 1.0) and mean.shape == (3,) and len(set(mean.tolist())) == 3
    assert abs(IC.window(11).sum() - 1.0) < 1e-15 and np.array_equal(IC.window(7), IC.window(7).T)
    assert np.allclose(np.outer(ops.ssim_window(11, 1.5), ops.ssim_window(11, 1.5)), IC.window(11), rtol=0, atol=1e-17)
    psnr, mse, n = IC.psnr_ref(x, x)
    assert np.all(np.isposinf(psnr)) and np.all(mse == 0) and np.all(n == 13 * 14)
    mask = IC.psnr_masks("corner", 3, 13, 14)
    psnr, mse, n = IC.psnr_ref(x, y, mask)
    assert np.isnan(psnr[0]) and n[0] == 0 and n[1] == 13 * 14 and 0 < n[2] < 13 * 14 and np.all(np.isfinite(psnr[1:]))
    # the reference's calculate_psnr on the masked images: mean over all H*W*C, times H*W / mask.sum()
    a, b = x[2].astype(np.float64) * mask[2][..., None], y[2].astype(np.float64) * mask[2][..., None]
    theirs = np.mean((a - b) ** 2) * (13 * 14) / mask[2].sum()
    assert abs(theirs / mse[2] - 1) < 1e-14 and abs(psnr[2] - 20 * math.log10(1.0 / math.sqrt(theirs))) < 1e-12
    psnr255, _, _ = IC.psnr_ref(x * 255, y * 255, mask, 255.0)
    assert np.allclose(psnr255[1:], psnr[1:], rtol=0, atol=1e-4)


def test_case_tables_cover_the_edges():
    th, tw = ops.SSIM_TILE
    cases = IC.ssim_cases(ops.SSIM_TILE)
    outs = {(H - win + 1, W - win + 1) for _, H, W, _, win, _, _ in cases.values()}
    assert {(1, 1), (1, 2)} <= outs
    assert {(th + a, tw + b) for a in (-1, 0, 1) for b in (-1, 0, 1)} <= outs
    assert any(oh > 2 * th and ow > 2 * tw for oh, ow in outs)
    assert {c[3] for c in cases.values()} == {1, 3, 4} and {c[0] for c in cases.values()} == {1, 3}
    assert {c[4] for c in cases.values()} == {3, 7, 11, 31} and {c[5] for c in cases.values()} == {1.0, 255.0}
    assert {c[6] for c in cases.values()} == set(IC.CONTENTS)
    assert all(max(c[1], c[2]) <= 100 for c in cases.values())
    x, y, (mean, smap), win, L = IC.ssim_case("two_tiles_each_way", ops.SSIM_TILE)
    assert not np.array_equal(x[0], x[1]) and len(set(mean.tolist())) == 3
    # inside the dark part x = 0 and y = L/255 are constant: s = C1 / ((L/255)^2 + C1), both variances vanish
    assert abs(smap[0, 0, 0, 0] - 1e-4 / (255.0 ** -2 + 1e-4)) < 1e-6 and smap[:, -1, -1].max() > smap[0, 0, 0, 0]
    shares = IC.psnr_cases(ops.SQERR_PIXELS)
    assert shares["one_share"][1] * shares["one_share"][2] == ops.SQERR_PIXELS
    assert ops.SQERR_PIXELS < shares["just_over_one_share"][1] * shares["just_over_one_share"][2] < 2 * ops.SQERR_PIXELS


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_image_symbols():
    L = _lib.lib()
    want = {
        "hm_image_sqerr_workspace_bytes": (C.c_int64, 3),
        "hm_image_sqerr": (C.c_int, 10),
        "hm_image_ssim_workspace_bytes": (C.c_int64, 4),
        "hm_image_ssim": (C.c_int, 14),
    }
    for name, (res, n_args) in want.items():
        assert name in _lib.SIGNATURES
        fn = getattr(L, name)
        assert fn.restype is res and len(fn.argtypes) == n_args == len(_lib.SIGNATURES[name][1])
    with open(_lib.LIB_PATH.replace("libhashmod.so", "../include/hashmod.h")) as fh:
        header = fh.read()
    for name in want:
        assert f"HM_API int{'64_t' if want[name][0] is C.c_int64 else ''} {name}(" in header


def test_workspace_sizes_follow_the_exported_tiles():
    L = _lib.lib()
    th, tw = ops.SSIM_TILE
    for win in (3, 11, 31):
        assert L.hm_image_ssim_workspace_bytes(1, win, win, win) == 8
        assert L.hm_image_ssim_workspace_bytes(3, th + win - 1, tw + win - 1, win) == 3 * 8
        assert L.hm_image_ssim_workspace_bytes(1, th + win, tw + win - 1, win) == 2 * 8
        assert L.hm_image_ssim_workspace_bytes(1, th + win - 1, tw + win, win) == 2 * 8
        assert L.hm_image_ssim_workspace_bytes(2, 2 * th + win, 2 * tw + win, win) == 2 * 9 * 8
    assert L.hm_image_ssim_workspace_bytes(1, 1200, 1600, 11) == 8 * 75 * 100
    n = ops.SQERR_PIXELS
    assert L.hm_image_sqerr_workspace_bytes(1, 1, 1) == 16 and L.hm_image_sqerr_workspace_bytes(1, 1, n) == 16
    assert L.hm_image_sqerr_workspace_bytes(3, 1, n + 1) == 3 * 32 and L.hm_image_sqerr_workspace_bytes(1, 4, n) == 64
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1 << 31, 4, 4), (1, 1 << 31, 4), (-1, 4, 4)):
        assert L.hm_image_sqerr_workspace_bytes(*bad) == -1 and b"[1, 2^31)" in L.hm_last_error()
        assert L.hm_image_ssim_workspace_bytes(*bad, 3) == -1
    assert L.hm_image_ssim_workspace_bytes(1, 10, 12, 11) == -1 and b"smaller than the window" in L.hm_last_error()
    assert L.hm_image_ssim_workspace_bytes(1, 12, 12, 10) == -1 and b"odd" in L.hm_last_error()
    assert L.hm_image_sqerr_workspace_bytes((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1) == -1   # B*H*W >= 2^62


def test_abi_rejects_bad_arguments_before_any_launch():
    """every call below must return -1 on the host: the pointers are host memory and are never dereferenced"""
    L = _lib.lib()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    null = C.c_void_p(0)

    def ssim(x=p, y=p, B=1, H=12, W=12, Cn=3, win=11, w=p, c1=1e-4, c2=9e-4, smap=null, ws=p, out=p):
        rc = L.hm_image_ssim(x, y, B, H, W, Cn, win, w, c1, c2, smap, ws, out, None)
        return rc, (L.hm_last_error() or b"").decode()

    def sqerr(x=p, y=p, mask=null, B=1, H=4, W=4, Cn=3, ws=p, out=p):
        rc = L.hm_image_sqerr(x, y, mask, B, H, W, Cn, ws, out, None)
        return rc, (L.hm_last_error() or b"").decode()

    for kw in (dict(x=null), dict(y=null), dict(w=null), dict(ws=null), dict(out=null)):
        rc, msg = ssim(**kw)
        assert rc == -1 and "hm_image_ssim: NULL pointer" in msg, (kw, rc, msg)
    for kw in (dict(x=null), dict(y=null), dict(ws=null), dict(out=null)):
        rc, msg = sqerr(**kw)
        assert rc == -1 and "hm_image_sqerr: NULL pointer" in msg, (kw, rc, msg)
    for win in (10, 12, 2, 1, 0, -3, 33, 35):
        rc, msg = ssim(win=win, H=64, W=64)
        assert rc == -1 and "win must be odd and in [3, 31]" in msg, (win, rc, msg)
    for kw in (dict(H=10), dict(W=10), dict(H=30, W=40, win=31)):
        rc, msg = ssim(**kw)
        assert rc == -1 and "smaller than the window" in msg, (kw, rc, msg)
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(B=-1), dict(W=1 << 31)):
        for call in (ssim, sqerr):
            rc, msg = call(**kw)
            assert rc == -1 and "must be in [1, 2^31)" in msg, (kw, rc, msg)
    for Cn in (0, 5, -1):
        for call in (ssim, sqerr):
            rc, msg = call(Cn=Cn)
            assert rc == -1 and "C must be in [1, 4]" in msg, (Cn, rc, msg)
    for kw in (dict(c2=0.0), dict(c2=-1e-4), dict(c1=0.0), dict(c2=float("nan")), dict(c1=float("inf"))):
        rc, msg = ssim(**kw)
        assert rc == -1 and "finite and positive" in msg, (kw, rc, msg)
    big = (1 << 31) - 1
    rc, msg = sqerr(B=big, H=big, W=big)
    assert rc == -1 and "below 2^62" in msg
    with pytest.raises(ValueError, match="NULL pointer"):
        _lib.check(sqerr(x=null)[0])


# ---------------------------------------------------------------------------------------------------------------------
# host checks of the ops
# ---------------------------------------------------------------------------------------------------------------------
def test_ops_check_their_arguments_before_the_device():
    x = torch.zeros(2, 12, 13, 3)
    bad_images = (x.double(), x.half(), torch.zeros(12, 13), torch.zeros(1, 2, 12, 13, 3), x[:, :, ::2], x[..., :2],
                  x.permute(0, 2, 1, 3), torch.zeros(2, 12, 13, 5), torch.zeros(2, 12, 13, 0), torch.zeros(0, 12, 13, 3),
                  x.numpy(), None)
    for bad in bad_images:
        like = bad if isinstance(bad, torch.Tensor) else x
        for a, b in ((bad, like), (like, bad)):
            with pytest.raises(ValueError, match="image_psnr"):
                ops.image_psnr(a, b)
            with pytest.raises(ValueError, match="image_ssim"):
                ops.image_ssim(a, b)
    for call in (ops.image_psnr, ops.image_ssim):
        with pytest.raises(ValueError, match="differ in shape"):
            call(x, torch.zeros(2, 12, 12, 3))
        with pytest.raises(ValueError, match="differ in shape"):
            call(x, x[0])
        with pytest.raises(ValueError, match="devices"):
            call(x, x.to("meta"))
        for L in (0, -1.0, float("nan"), float("inf"), "1", None, True):
            with pytest.raises(ValueError, match="data_range"):
                call(x, x, data_range=L)
    for win in (10, 1, 33, 11.0, "11", None, -3):
        with pytest.raises(ValueError, match="win"):
            ops.image_ssim(x, x, win=win)
    with pytest.raises(ValueError, match="smaller than"):
        ops.image_ssim(x, x, win=13)                    # H = 12
    with pytest.raises(ValueError, match="smaller than"):
        ops.image_ssim(torch.zeros(1, 40, 12, 1), torch.zeros(1, 40, 12, 1), win=13)
    for sigma in (0, -1.5, float("nan"), "s"):
        with pytest.raises(ValueError, match="sigma"):
            ops.image_ssim(x, x, sigma=sigma)
    for k in (0, -0.01, float("inf")):
        with pytest.raises(ValueError, match="k1"):
            ops.image_ssim(x, x, k1=k)
        with pytest.raises(ValueError, match="k2"):
            ops.image_ssim(x, x, k2=k)
    with pytest.raises(ValueError, match="positive and finite"):
        ops.image_ssim(x, x, data_range=1e-200)         # (k1 L)^2 underflows to 0
    ok = torch.ones(2, 12, 13, dtype=torch.bool)
    for mask in (ok.float(), ok.to(torch.int32), ok[:1], torch.ones(2, 12, 13, 3, dtype=torch.bool), ok[0],
                 torch.ones(2, 13, 12, dtype=torch.bool).transpose(1, 2), torch.ones(2, 12, 26, dtype=torch.bool)[..., ::2],
                 ok.to("meta"), ok.numpy()):
        with pytest.raises(ValueError, match="mask"):
            ops.image_psnr(x, x, mask=mask)
    # arguments that are right get as far as the device: no CPU fall-back
    for call in (lambda: ops.image_psnr(x, x, mask=ok), lambda: ops.image_psnr(x[0], x[0], mask=ok[0].to(torch.uint8)),
                 lambda: ops.image_ssim(x, x), lambda: ops.image_ssim(x[0], x[0], win=3, return_map=True)):
        with pytest.raises(_lib.HashmodError, match="no CPU fallback") as e:
            call()
        assert not isinstance(e.value, ValueError)


# ---------------------------------------------------------------------------------------------------------------------
# evaluation.images on a stub model
# ---------------------------------------------------------------------------------------------------------------------
class _Stub(torch.nn.Module):
    """rgb and mask are pure functions of uv, through a parameter and with a graph attached, as the real model's"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([[0.013, -0.007, 0.002], [0.004, 0.011, -0.009]]))
        self.calls = []

    def forward(self, inp):
        uv = inp["uv"]
        self.calls.append((self.training, torch.is_grad_enabled(), uv.shape[1], inp["object_mask"].shape[1]))
        with torch.enable_grad():                       # what get_rbg_value does for the normals
            rgb = torch.sin(uv.reshape(-1, 2) @ self.w)
        hit = (uv.reshape(-1, 2).sum(1) % 3) != 0
        return {"rgb_values": rgb, "network_object_mask": hit, "grad_theta": None}


def _view(H, W, batch=1):
    rows, cols = np.mgrid[0:H, 0:W]
    uv = torch.from_numpy(np.stack([cols, rows], -1).reshape(1, -1, 2).astype(np.float32)).repeat(batch, 1, 1)
    return {"uv": uv, "object_mask": torch.ones(batch, H * W, dtype=torch.bool), "pose": torch.eye(4)[None],
            "intrinsics": torch.eye(4)[None]}


@pytest.mark.parametrize("training", [True, False])
def test_render_view_is_the_chunked_loop(training):
    H, W = 20, 24
    model = _Stub().train(training)
    inp = _view(H, W, batch=2)
    inp["uv"][1] += 100.0
    rgb, hit = render_view(model, inp, H * W, chunk=128)
    assert model.training is training
    assert [c[2] for c in model.calls] == [128, 128, 128, 96] and all(c[3] == c[2] for c in model.calls)   # ragged end
    assert all(c[0] is False and c[1] is False for c in model.calls)                  # eval mode, no_grad
    assert rgb.shape == (2, H * W, 3) and hit.shape == (2, H * W) and hit.dtype == torch.bool
    assert not rgb.requires_grad and rgb.grad_fn is None
    model.calls.clear()
    with torch.no_grad():
        whole = model.eval()(inp)
    assert torch.equal(rgb, whole["rgb_values"].reshape(2, H * W, 3))
    assert torch.equal(hit, whole["network_object_mask"].reshape(2, H * W))
    assert not torch.equal(rgb[0], rgb[1]) and 0 < hit.sum() < hit.numel()
    one, _ = render_view(model, inp, H * W, chunk=H * W + 5)
    assert torch.equal(one, rgb)
    for bad in (dict(total_pixels=H * W - 1), dict(chunk=0), dict(chunk=2.5)):
        with pytest.raises(ValueError, match="render_view"):
            render_view(model, inp, **{"total_pixels": H * W, "chunk": 128, **bad})


def test_render_view_restores_the_mode_after_an_error():
    class Broken(torch.nn.Module):
        def forward(self, inp):
            raise RuntimeError("boom")
    model = Broken().train()
    with pytest.raises(RuntimeError, match="boom"):
        render_view(model, _view(4, 4), 16)
    assert model.training is True


class _Views:
    """three 6 x 8 views in SceneDataset's interface"""
    img_res = [6, 8]
    total_pixels = 48
    sampling_idx = None

    def __len__(self):
        return 3

    def __getitem__(self, i):
        v = _view(6, 8)
        sample = {"uv": v["uv"][0] + 10.0 * i, "object_mask": v["object_mask"][0], "pose": torch.eye(4),
                  "intrinsics": torch.eye(4)}
        return i, sample, {"rgb": torch.full((48, 3), 0.1 * i)}

    def collate_fn(self, batch):
        from hashmodnffbanks_idr_amd.datasets.scene_dataset import SceneDataset
        return SceneDataset.collate_fn(self, batch)


def test_evaluate_views_writes_the_csvs(tmp_path, monkeypatch):
    seen = []

    def fake_metrics(rgb_pred, rgb_gt, object_mask, img_res):      # view_metrics needs the device: test_image_metrics_gpu
        seen.append((tuple(rgb_pred.shape), tuple(rgb_gt.shape), tuple(object_mask.shape), list(img_res)))
        d = (rgb_pred.double() - rgb_gt.double()).pow(2).mean()
        return 10.0 + d, 1.0 / (1.0 + d)

    monkeypatch.setattr(EI, "view_metrics", fake_metrics)
    model = _Stub().train()
    out = tmp_path / "metrics"
    r = evaluate_views(model, _Views(), chunk=20, out_dir=str(out))
    assert model.training and seen == [((48, 3), (48, 3), (48,), [6, 8])] * 3
    assert r.indices == [0, 1, 2] and len(r.psnrs) == len(r.ssims) == 3 and len(set(r.psnrs)) == 3
    assert all(isinstance(v, float) for v in r.psnrs + r.ssims)
    assert r.psnr_mean == sum(r.psnrs) / 3 and r.ssim_mean == sum(r.ssims) / 3
    for name, values, mean in (("psnrs.csv", r.psnrs, r.psnr_mean), ("ssims.csv", r.ssims, r.ssim_mean)):
        lines = (out / name).read_text().splitlines()
        assert lines[0] == ",0" and len(lines) == 1 + 3 + 1
        rows = [ln.split(",") for ln in lines[1:]]
        assert [int(a) for a, _ in rows] == [0, 1, 2, 3]
        assert [float(b) for _, b in rows] == values + [mean]                    # repr round-trips
    sub = evaluate_views(model, _Views(), indices=[2, 0], chunk=48)
    assert sub.indices == [2, 0] and sub.psnrs == [r.psnrs[2], r.psnrs[0]] and not (tmp_path / "psnrs.csv").exists()
    with pytest.raises(ValueError, match="no view"):
        evaluate_views(model, _Views(), indices=[])
    sampled = _Views()
    sampled.sampling_idx = torch.arange(4)
    with pytest.raises(ValueError, match="change_sampling_idx"):
        evaluate_views(model, sampled)
