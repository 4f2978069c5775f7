"""Time of scoring one rendered view on the GPU (ops.image_psnr, ops.image_ssim: csrc/hm_image.hip) and on the host as
before (download, scipy's gaussian_filter for the five moments in float64, numpy), and of rendering one such view
(evaluation.images.render_view).

    python scripts/image_metrics_time.py [--height 1200] [--width 1600] [--reps 3] [--chunk 10000] [--no-render]
                                         [--out FILE]

No data files.  The pair is seeded: a smooth random image in [0, 1] and the same plus noise of 0.05, fp32
[1, H, W, 3] on the device; the mask is a centred ellipse.  After a warm-up, --reps times alternately, as wall clock
from a synchronised device to the two scalars in host memory:
  (a) device: image_psnr(x, y, mask) and image_ssim(x, y), one .tolist()
  (b) host: download of both images and the mask, the masked mse in float64, gaussian_filter(sigma 1.5, truncate 3.5,
      mode reflect) of x, y, x^2, y^2, x y in float64, the border of 5 pixels cropped, the SSIM formula and its mean
The scores must agree to 1e-9, else the script fails.  Then one render_view of H x W pixels in chunks of --chunk through
an IDRNetwork of config C2 at its geometric initialisation (seed 0), the camera on the z axis at distance 2.5 looking
at the origin with the unit sphere filling the view's height: a warm-up call on the first chunks, then one timed call.
No GPU: exits with an error instead of printing a number.  Prints a line per measurement, then one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def make_pair(H, W):
    import torch
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(0)
    coarse = torch.rand((1, 3, H // 16 + 2, W // 16 + 2), generator=gen)
    x = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    y = (x + 0.05 * torch.randn(x.shape, generator=gen)).clamp(0.0, 1.0)
    rows = (torch.arange(H)[:, None] - (H - 1) / 2) / (0.4 * H)
    cols = (torch.arange(W)[None, :] - (W - 1) / 2) / (0.4 * W)
    mask = (rows * rows + cols * cols < 1.0)[None]
    return x.contiguous().cuda(), y.contiguous().cuda(), mask.contiguous().cuda()


def device_scores(x, y, mask):
    import torch
    from hashmodnffbanks_idr_amd import ops
    psnr, ssim = torch.cat([ops.image_psnr(x, y, mask=mask), ops.image_ssim(x, y)]).tolist()
    return {"psnr": psnr, "ssim": ssim}


def host_scores(x, y, mask):
    import numpy as np
    from scipy.ndimage import gaussian_filter
    a, b, m = x.cpu().numpy()[0].astype(np.float64), y.cpu().numpy()[0].astype(np.float64), mask.cpu().numpy()[0]
    mse = ((a - b) ** 2)[m].sum() / (m.sum() * a.shape[-1])
    psnr = 10.0 * np.log10(1.0 / mse)

    def moment(img):
        return gaussian_filter(img, sigma=(1.5, 1.5, 0), truncate=3.5, mode="reflect")[5:-5, 5:-5]

    mx, my = moment(a), moment(b)
    sx2, sy2, sxy = moment(a * a) - mx * mx, moment(b * b) - my * my, moment(a * b) - mx * my
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    s = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sx2 + sy2 + c2))
    return {"psnr": float(psnr), "ssim": float(s.mean())}


def render_input(H, W, device):
    """uv, pose, intrinsics of an H x W view from (0, 0, -2.5) towards the origin; focal length such that the unit
    sphere's silhouette spans the view's height"""
    import numpy as np
    import torch
    f = 0.5 * H * np.sqrt(2.5 ** 2 - 1.0)
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = f
    K[0, 2], K[1, 2] = 0.5 * W, 0.5 * H
    pose = np.eye(4, dtype=np.float32)
    pose[2, 3] = -2.5
    rows, cols = np.mgrid[0:H, 0:W].astype(np.float32)
    uv = np.stack([cols, rows], -1).reshape(1, H * W, 2)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    return {"uv": T(uv), "pose": T(pose[None]), "intrinsics": T(K[None]),
            "object_mask": torch.ones((1, H * W), dtype=torch.bool, device=device)}


def time_render(H, W, chunk):
    import torch
    import bench
    from hashmodnffbanks_idr_amd.evaluation import render_view
    from hashmodnffbanks_idr_amd.model.implicit_differentiable_renderer import IDRNetwork
    torch.manual_seed(0)
    model = IDRNetwork(bench.idr_conf("C2")).cuda()
    inp = render_input(H, W, "cuda")
    n_warm = min(H * W, 4 * chunk)          # rows from the top of the view: background; and a band through its middle
    mid = (H // 2) * W
    for lo in (0, min(mid, H * W - n_warm)):
        part = dict(inp, uv=inp["uv"][:, lo:lo + n_warm].contiguous(),
                    object_mask=inp["object_mask"][:, lo:lo + n_warm].contiguous())
        render_view(model, part, n_warm, chunk)
    (rgb, hit), ms = _wall(lambda: render_view(model, inp, H * W, chunk))
    return ms, int(hit.sum()), (H * W + chunk - 1) // chunk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=10000)
    ap.add_argument("--no-render", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("image_metrics_time.py: no GPU - nothing is measured")
    H, W = args.height, args.width
    x, y, mask = make_pair(H, W)
    device_scores(x, y, mask)                                          # warm-up: code objects, allocator, workspace
    dev_ms, host_ms = [], []
    for _ in range(args.reps):
        dev, t = _wall(lambda: device_scores(x, y, mask))
        dev_ms.append(round(t, 3))
        print(f"device: {t:.3f} ms  {dev}", flush=True)
        host, t = _wall(lambda: host_scores(x, y, mask))
        host_ms.append(round(t, 1))
        print(f"host:   {t:.1f} ms  {host}", flush=True)
    agree = all(abs(dev[k] - host[k]) <= 1e-9 for k in ("psnr", "ssim"))
    out = {"height": H, "width": W, "device_ms": dev_ms, "host_ms": host_ms, "device_best_ms": min(dev_ms),
           "host_best_ms": min(host_ms), "device": dev, "host": host, "agree": agree}
    if not args.no_render:
        ms, n_hit, n_chunks = time_render(H, W, args.chunk)
        print(f"render_view: {ms:.0f} ms  ({n_chunks} chunks of {args.chunk}, {n_hit} of {H * W} rays meet the surface)",
              flush=True)
        out.update({"render_ms": round(ms, 1), "render_chunks": n_chunks, "render_hits": n_hit})
    line = json.dumps({"image_metrics": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not agree:
        raise SystemExit("image_metrics_time.py: the device and host scores differ beyond 1e-9")


if __name__ == "__main__":
    main()
