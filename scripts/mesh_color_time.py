"""Time of colouring an extracted mesh from the input views on the GPU (evaluation.color.color_mesh:
csrc/hm_mesh_color.hip) and of the vectorised numpy restatement on the host.

    python scripts/mesh_color_time.py [--res 512] [--views 49] [--height 1200] [--width 1600] [--erode 1] [--reps 5]
                                      [--out FILE]

No data files.  The mesh and the cameras are mesh_cull_time.py's (ops.marching_cubes of the analytic bumpy sphere at
--res; --views look_at cameras on a dome); the photographs are seeded uniform noise in [-1, 1), held on the host as
SceneDataset.rgb_images holds them (a list of [H*W, 3] fp32 tensors); the masks are the finite pixels of the device
depth maps of the same mesh (timing inputs, not a check).  After a warm-up, --reps times alternately (each repetition
after a gc.collect()), as wall clock from a synchronised device to a synchronised device:
  device  the upload of the host's images alone; the depth maps of all views (ops.mesh_depth_maps); the masks' summed-area
          tables; ops.mesh_vertex_colors of all views, images and depth maps resident: without masks (the kernel and its
          launch), with masks (plus their summed-area tables), in blend and in best mode; color_mesh as a whole, from the
          host's images to the downloaded colours: uploads, depth maps, tables, kernel, finish
  host    the same contract in vectorised numpy, a loop over the views, given the DEVICE's depth maps (downloaded; the
          raster has no vectorised numpy form and is not timed) and scipy.ndimage.binary_erosion for the masks
The host's accumulators must equal the device's bit for bit, else the script fails.  The kernel's time is put against
its work: (vertex, view) pairs per second, and the bytes its scattered reads ask for - nine 4-byte depth reads per
pair in the image and twelve 4-byte image reads per contributing pair (whole 64-byte lines move for each).  No GPU:
exits with an error instead of printing a number.  Prints a line per repetition, then one JSON line.
"""
import argparse
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from chamfer_time import _wall, bumpy_sphere  # noqa: E402  (scripts/ is sys.path[0])
from mesh_cull_time import _spread, dome_cameras  # noqa: E402


def host_vertex_colors(verts, normals, proj, centers, images, depth, masks, erode, pad, tol, min_cos, power, mode):
    """(acc [V,4] float64, n_used [V] int32, pairs in the image) of the contract in include/hashmod.h, vectorised over
    the vertices; images: per-view [H*W, 3] fp32 arrays"""
    import numpy as np
    from scipy.ndimage import binary_erosion
    H, W = depth.shape[1:]
    x, y, z = (verts[:, a].astype(np.float64) for a in range(3))
    nx, ny, nz = (normals[:, a].astype(np.float64) for a in range(3))
    nn = (nx * nx + ny * ny) + nz * nz
    acc, n_used = np.zeros((len(verts), 4)), np.zeros(len(verts), np.int32)
    in_image = 0
    square = np.ones((3, 3), bool)
    for k, P in enumerate(proj):
        with np.errstate(all="ignore"):
            p = [((P[a, 0] * x + P[a, 1] * y) + P[a, 2] * z) + P[a, 3] for a in range(3)]
            w = p[2]
            u, v = p[0] / w, p[1] / w
            c, r = np.rint(u), np.rint(v)
            keep = np.isfinite(w) & (w > 0) & (c >= 0) & (c < W) & (r >= 0) & (r < H)
        idx = np.flatnonzero(keep)
        in_image += len(idx)
        col, row = c[idx].astype(np.int64), r[idx].astype(np.int64)
        m = np.full(len(idx), -np.inf, np.float32)
        for dr in range(-pad, pad + 1):
            for dc in range(-pad, pad + 1):
                m = np.maximum(m, depth[k][np.clip(row + dr, 0, H - 1), np.clip(col + dc, 0, W - 1)])
        ok = w[idx].astype(np.float32) <= m + np.float32(tol)
        if masks is not None:
            inner = binary_erosion(masks[k], structure=square, iterations=erode, border_value=1) if erode else masks[k]
            ok &= inner[row, col]
        idx = idx[ok]
        dx, dy, dz = centers[k, 0] - x[idx], centers[k, 1] - y[idx], centers[k, 2] - z[idx]
        with np.errstate(all="ignore"):
            den = np.sqrt(nn[idx] * ((dx * dx + dy * dy) + dz * dz))
            cos = ((nx[idx] * dx + ny[idx] * dy) + nz[idx] * dz) / den
            ok = (den > 0) & np.isfinite(cos) & (cos > min_cos)
        idx, cos = idx[ok], cos[ok]
        wgt = np.ones(len(idx))
        for _ in range(power):
            wgt = wgt * cos
        fc, fr = np.floor(u[idx]), np.floor(v[idx])
        fu, fv = (u[idx] - fc)[:, None], (v[idx] - fr)[:, None]
        ca, cb = np.clip(fc.astype(np.int64), 0, W - 1), np.clip(fc.astype(np.int64) + 1, 0, W - 1)
        ra, rb = np.clip(fr.astype(np.int64), 0, H - 1), np.clip(fr.astype(np.int64) + 1, 0, H - 1)
        img = images[k]
        taa, tab = img[ra * W + ca].astype(np.float64), img[ra * W + cb].astype(np.float64)
        tba, tbb = img[rb * W + ca].astype(np.float64), img[rb * W + cb].astype(np.float64)
        val = (taa * (1.0 - fu) + tab * fu) * (1.0 - fv) + (tba * (1.0 - fu) + tbb * fu) * fv
        n_used[idx] += 1
        if mode == "blend":
            acc[idx, :3] = acc[idx, :3] + wgt[:, None] * val
            acc[idx, 3] = acc[idx, 3] + wgt
        else:
            better = wgt > acc[idx, 3]
            acc[idx[better], :3] = val[better]
            acc[idx[better], 3] = wgt[better]
    return acc, n_used, in_image


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--erode", type=int, default=1)
    ap.add_argument("--min-cos", type=float, default=0.0)
    ap.add_argument("--power", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_color_time.py: no GPU - nothing is measured")
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd.evaluation import color_mesh, view_projections

    H, W, n = args.height, args.width, args.views
    vol, spacing = bumpy_sphere(args.res)
    verts, faces, normals = ops.marching_cubes(vol, 0.0, spacing)
    verts = (verts - 1.0).contiguous()          # the lattice of [-1, 1]^3
    del vol
    if float((normals * verts).sum()) < 0:      # outward, whichever sign the extraction gives them
        normals = (-normals).contiguous()
    K, pose = dome_cameras(n, H, W)
    proj = view_projections(K, pose)
    centers = np.ascontiguousarray(pose[:, :3, 3].astype(np.float64))
    dproj, dcenters = torch.from_numpy(proj).cuda(), torch.from_numpy(centers).cuda()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    gen = torch.Generator(device="cuda").manual_seed(7)
    dimages = (torch.rand((n, H, W, 3), device="cuda", generator=gen) * 2.0 - 1.0).contiguous()
    host_images = [im.reshape(-1, 3).cpu() for im in dimages]                # as SceneDataset.rgb_images
    depth, skipped = ops.mesh_depth_maps(verts, faces, dproj, H, W)          # warm-up of the raster; the masks' source
    masks = torch.isfinite(depth)
    host_masks = masks.cpu()
    kw = dict(erode=args.erode, pad=1, tol=0.0, min_cos=args.min_cos, power=args.power)
    print(f"mesh: V {V}, F {F}; {n} views {H} x {W}; skipped {int(skipped.sum())}", flush=True)

    def kernel(mode, with_masks):
        return ops.mesh_vertex_colors(verts, normals, dproj, dcenters, dimages, depth,
                                      masks=masks if with_masks else None, mode=mode, **kw)

    def device_whole(mode):
        colors, stats = color_mesh((verts, faces, normals), K, pose, host_images, (H, W), masks=host_masks, mode=mode,
                                   device=verts.device, **kw)
        return colors.cpu(), stats

    for mode in ("blend", "best"):                                           # warm-up of every timed call
        kernel(mode, False), kernel(mode, True), device_whole(mode)
    names = ["upload_images", "raster", "table"] + [f"kernel_{m}{s}" for m in ("blend", "best") for s in ("", "_masks")] + \
        ["color_mesh_blend", "color_mesh_best"]
    t = {k: [] for k in names}
    got, whole = {}, {}
    for _ in range(args.reps):
        gc.collect()        # Python's garbage is collected here, not inside a timed window of a few milliseconds
        t["upload_images"].append(_wall(lambda: [im.to(verts.device) for im in host_images] and None)[1])
        t["raster"].append(_wall(lambda: ops.mesh_depth_maps(verts, faces, dproj, H, W))[1])
        t["table"].append(_wall(lambda: ops._mask_table(masks))[1])
        for mode in ("blend", "best"):
            t[f"kernel_{mode}"].append(_wall(lambda: kernel(mode, False))[1])
            got[mode], ms = _wall(lambda: kernel(mode, True))
            t[f"kernel_{mode}_masks"].append(ms)
            whole[mode], ms = _wall(lambda: device_whole(mode))
            t[f"color_mesh_{mode}"].append(ms)
        print({k: round(v[-1], 2) for k, v in t.items()}, flush=True)

    # the host leg: the mesh, the depth maps and the masks come down once; the images are the host's already
    (hv, hn), download_ms = _wall(lambda: (verts.cpu().numpy(), normals.cpu().numpy()))
    hdepth, depth_download_ms = _wall(lambda: depth.cpu().numpy())
    hmasks, himages = host_masks.numpy(), [im.numpy() for im in host_images]
    host = {"blend": [], "best": []}
    agree, in_image = True, 0
    for rep in range(max(1, min(args.reps, 3))):
        for mode in ("blend", "best"):
            (acc, n_used, in_image), ms = _wall(lambda: host_vertex_colors(hv, hn, proj, centers, himages, hdepth, hmasks,
                                                                           mode=mode, **kw))
            host[mode].append(ms)
            same = (np.array_equal(acc.view(np.int64), got[mode][0].cpu().numpy().view(np.int64))
                    and np.array_equal(n_used, got[mode][1].cpu().numpy()))
            agree = agree and same
            print(f"host {mode}: {ms:.0f} ms, agrees with the device bit for bit: {same}", flush=True)
    for mode in ("blend", "best"):                   # color_mesh draws its own depth maps: the same colours
        fin = ops.mesh_colors_finish(*got[mode], mode).cpu()
        agree = agree and torch.equal(fin.view(torch.int32), whole[mode][0].view(torch.int32))
    stats = whole["blend"][1]
    used = int(got["blend"][1].sum())
    print("color_mesh:", stats._replace(n_skipped=sum(stats.n_skipped)), "contributing (vertex, view) pairs", used,
          flush=True)

    best = min(t["kernel_blend"])
    out = {"res": args.res, "verts": V, "faces": F, "views": n, "H": H, "W": W, "erode": args.erode,
           "min_cos": args.min_cos, "power": args.power, "reps": args.reps, "agree": agree,
           "device_ms": {k: _spread(v) for k, v in t.items()},
           "host_ms": {"download_mesh": round(download_ms, 2), "download_depth": round(depth_download_ms, 2),
                       **{f"vertex_colors_{m}": _spread(v) for m, v in host.items()}},
           "pairs": V * n, "pairs_in_image": in_image, "pairs_contributing": used,
           "kernel_gpairs_per_s": round(V * n / best / 1e6, 2),
           "kernel_requested_gb_per_s": round((in_image * 36 + used * 48) / best / 1e6, 1),
           "n_colored": stats.n_colored}
    line = json.dumps({"mesh_color": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not agree:
        raise SystemExit("mesh_color_time.py: the host and device colours differ")


if __name__ == "__main__":
    main()
