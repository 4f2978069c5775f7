"""Time of culling an extracted mesh by camera masks and visibility on the GPU (evaluation.cull.cull_mesh:
csrc/hm_mesh_cull.hip) and of the host detour it replaces.

    python scripts/mesh_cull_time.py [--res 512] [--views 49] [--height 1200] [--width 1600] [--dilate 5] [--reps 3]
                                     [--out FILE]

No data files.  The mesh is ops.marching_cubes of chamfer_time.py's analytic bumpy sphere at --res; the cameras are
--views look_at cameras on a dome of radius 2.5 whose focal length lets the object fill three quarters of the image
height; the masks are the finite pixels of the device depth maps of the same mesh (a timing input, not a check).  After
a warm-up, --reps times alternately (each repetition after a gc.collect(), so that the host leg's garbage is not
collected inside a device window of a few milliseconds), as wall clock from a synchronised device to a synchronised
device:
  device  the summed-area tables; ops.mesh_mask_votes (tables included); ops.mesh_depth_maps of all views, per view and
          in (face, view) pairs per second; ops.mesh_visible_votes; ops.mesh_keep_vertices; cull_mesh as a whole with
          the download of its result
  host    what a user does today, for the stages that have a vectorised numpy form: the download of the mesh; the
          projection of every vertex into every view and the mask votes with scipy.ndimage.binary_dilation (a 3 x 3
          square, `dilate` iterations); the visibility lookup given the DEVICE's depth maps (downloaded; a host raster
          of 1.45 M faces into 49 views has no vectorised numpy form and is not timed); the face filter with np.unique
The host votes must equal the device's, else the script fails.  The raster has no host counterpart: its time is put
against the traffic it must move - three 16-byte projected vertices and 12 bytes of indices per (face, view) pair, and
one 4-byte atomic per covered pixel, of which twice the drawn pixels (a closed surface is crossed at least twice) is a
lower bound.  The large-face path is timed on the same surface at --coarse-res (faces of some hundred pixels) for
several thresholds `big_face`.  No GPU: exits with an error instead of printing a number.  Prints a line per
measurement, then one JSON line.
"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from chamfer_time import _wall, bumpy_sphere  # noqa: E402  (scripts/ is sys.path[0])


def dome_cameras(n, H, W, radius=2.5, fill=0.75, extent=0.66):
    """(intrinsics [n,4,4] fp32, pose [n,4,4] fp32 camera-to-world) of n cameras on the upper dome looking at the origin"""
    import numpy as np
    k = np.arange(n) + 0.5
    elev = np.arcsin(0.15 + 0.8 * k / n)
    azim = k * np.pi * (3.0 - np.sqrt(5.0))
    eyes = radius * np.stack([np.cos(elev) * np.cos(azim), np.cos(elev) * np.sin(azim), np.sin(elev)], 1)
    focal = fill * 0.5 * H * np.sqrt(radius * radius - extent * extent) / extent
    K = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    K[:, 0, 0] = K[:, 1, 1] = focal
    K[:, 0, 2], K[:, 1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    pose = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    for i, e in enumerate(eyes):
        z = -e / np.linalg.norm(e)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        pose[i, :3, 0], pose[i, :3, 1], pose[i, :3, 2], pose[i, :3, 3] = x, np.cross(z, x), z, e
    return K, pose


def host_project(verts64, P, H, W):
    """(col, row, in_image, w) of the contract's projection, vectorised"""
    import numpy as np
    x, y, z = verts64[:, 0], verts64[:, 1], verts64[:, 2]
    with np.errstate(all="ignore"):
        p = [((P[a, 0] * x + P[a, 1] * y) + P[a, 2] * z) + P[a, 3] for a in range(3)]
        w = p[2]
        c, r = np.rint(p[0] / w), np.rint(p[1] / w)
        inside = np.isfinite(w) & (w > 0) & (c >= 0) & (c < W) & (r >= 0) & (r < H)
    return np.where(inside, c, 0).astype(np.int64), np.where(inside, r, 0).astype(np.int64), inside, w


def host_mask_votes(verts, proj, masks, dilate):
    import numpy as np
    from scipy.ndimage import binary_dilation
    v64 = verts.astype(np.float64)
    n_img, n_msk = np.zeros(len(verts), np.int32), np.zeros(len(verts), np.int32)
    square = np.ones((3, 3), bool)
    for P, m in zip(proj, masks):
        col, row, inside, _ = host_project(v64, P, *m.shape)
        grown = binary_dilation(m, structure=square, iterations=dilate) if dilate else m
        n_img += inside
        n_msk += inside & grown[row, col]
    return n_img, n_msk


def host_visible_votes(verts, proj, depth, pad, tol):
    import numpy as np
    v64 = verts.astype(np.float64)
    n_vis = np.zeros(len(verts), np.int32)
    H, W = depth.shape[1:]
    for P, d in zip(proj, depth):
        col, row, inside, w = host_project(v64, P, H, W)
        m = np.full(len(verts), -np.inf, np.float32)
        for dr in range(-pad, pad + 1):
            for dc in range(-pad, pad + 1):
                m = np.maximum(m, d[np.clip(row + dr, 0, H - 1), np.clip(col + dc, 0, W - 1)])
        with np.errstate(all="ignore"):
            n_vis += inside & (w.astype(np.float32) <= m + np.float32(tol))
    return n_vis


def host_keep(verts, faces, keep):
    import numpy as np
    alive = faces[keep[faces].all(1)]
    ids, inv = np.unique(alive, return_inverse=True)
    return verts[ids], inv.reshape(-1, 3).astype(np.int32)


def _spread(ms):
    return {"best": round(min(ms), 2), "median": round(sorted(ms)[len(ms) // 2], 2), "worst": round(max(ms), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--coarse-res", type=int, default=100)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--dilate", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_cull_time.py: no GPU - nothing is measured")
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd.evaluation import cull_mesh, view_projections

    H, W, n = args.height, args.width, args.views
    vol, spacing = bumpy_sphere(args.res)
    verts, faces, normals = ops.marching_cubes(vol, 0.0, spacing)
    verts = (verts - 1.0).contiguous()          # the lattice of [-1, 1]^3
    del vol
    K, pose = dome_cameras(n, H, W)
    proj = view_projections(K, pose)
    dproj = torch.from_numpy(proj).cuda()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    depth, skipped = ops.mesh_depth_maps(verts, faces, dproj, H, W)        # warm-up of the raster; the masks' source
    masks = torch.isfinite(depth)
    drawn = int(masks.sum())
    print(f"mesh: V {V}, F {F}; {n} views {H} x {W}; drawn pixels {drawn} ({drawn / n / H / W:.3f} of the images), "
          f"{drawn / n / (F / 2):.2f} per front face; skipped {int(skipped.sum())}", flush=True)

    def device_whole():
        (v, f, nn), stats = cull_mesh((verts, faces, normals), K, pose, masks, (H, W), dilate=args.dilate)
        return v.cpu(), f.cpu(), nn.cpu(), stats

    device_whole()                                                          # warm-up of every other stage
    per = max(1, (1 << 28) // (4 * (H + 1) * (W + 1)))
    t = {k: [] for k in ("table", "mask_votes", "raster", "visible_votes", "keep", "cull_mesh", "host_download",
                         "host_mask_votes", "host_depth_download", "host_visible_votes", "host_keep")}
    agree = True
    for _ in range(args.reps):
        gc.collect()        # the host leg's garbage is collected here, not inside a timed window of a few milliseconds
        gen2 = gc.get_stats()[2]["collections"]
        t["table"].append(_wall(lambda: [ops._mask_table(masks[v0:v0 + per]) for v0 in range(0, n, per)] and None)[1])
        (n_img, n_msk), ms = _wall(lambda: ops.mesh_mask_votes(verts, dproj, masks, args.dilate))
        t["mask_votes"].append(ms)
        (depth, skipped), ms = _wall(lambda: ops.mesh_depth_maps(verts, faces, dproj, H, W))
        t["raster"].append(ms)
        n_vis, ms = _wall(lambda: ops.mesh_visible_votes(verts, dproj, depth))
        t["visible_votes"].append(ms)
        keep = (n_msk == n_img) & (n_vis >= 1)
        kept, ms = _wall(lambda: ops.mesh_keep_vertices(verts, faces, normals, keep))
        t["keep"].append(ms)
        whole, ms = _wall(device_whole)
        t["cull_mesh"].append(ms)
        full_collections = gc.get_stats()[2]["collections"] - gen2
        # the host leg
        (hv, hf), ms = _wall(lambda: (verts.cpu().numpy(), faces.cpu().numpy()))
        t["host_download"].append(ms)
        hmasks = masks.cpu().numpy()
        (h_img, h_msk), ms = _wall(lambda: host_mask_votes(hv, proj, hmasks, args.dilate))
        t["host_mask_votes"].append(ms)
        hdepth, ms = _wall(lambda: depth.cpu().numpy())
        t["host_depth_download"].append(ms)
        h_vis, ms = _wall(lambda: host_visible_votes(hv, proj, hdepth, 1, 0.0))
        t["host_visible_votes"].append(ms)
        hkeep = (h_msk == h_img) & (h_vis >= 1)
        (kv, kf), ms = _wall(lambda: host_keep(hv, hf, hkeep))
        t["host_keep"].append(ms)
        same = (np.array_equal(h_img, n_img.cpu().numpy()) and np.array_equal(h_msk, n_msk.cpu().numpy())
                and np.array_equal(h_vis, n_vis.cpu().numpy()) and np.array_equal(kv, kept[0].cpu().numpy())
                and np.array_equal(kf, kept[1].cpu().numpy()))
        agree = agree and same
        print({k: round(v[-1], 2) for k, v in t.items()}, "agree", same, "full collections of Python's garbage in the "
              "device windows", full_collections, flush=True)
        del hdepth, hmasks
    stats = whole[3]
    print("cull_mesh:", stats._replace(n_skipped=sum(stats.n_skipped)), flush=True)

    # the large-face path: the same surface at a coarse resolution, faces of some hundred pixels
    vol, sp = bumpy_sphere(args.coarse_res)
    cv, cf, _ = ops.marching_cubes(vol, 0.0, sp)
    cv = (cv - 1.0).contiguous()
    thresholds = [1, 16, 64, 256, 1024, 1 << 40]
    coarse = {th: [] for th in thresholds}
    fine = {th: [] for th in (1, 16, 64, 1 << 40)}
    ref = ops.mesh_depth_maps(cv, cf, dproj, H, W)[0]
    for th in thresholds:
        assert torch.equal(ops.mesh_depth_maps(cv, cf, dproj, H, W, big_face=th)[0].view(torch.int32),
                           ref.view(torch.int32))                           # warm-up, and the same bits
    for _ in range(args.reps):
        for th in thresholds:
            coarse[th].append(_wall(lambda: ops.mesh_depth_maps(cv, cf, dproj, H, W, big_face=th))[1])
        for th in fine:
            fine[th].append(_wall(lambda: ops.mesh_depth_maps(verts, faces, dproj, H, W, big_face=th))[1])
    coarse_drawn = int(torch.isfinite(ref).sum())
    print(f"coarse mesh: F {cf.shape[0]}, {coarse_drawn / n / (cf.shape[0] / 2):.0f} pixels per front face", flush=True)
    for th in thresholds:
        print(f"big_face {th}: coarse {_spread(coarse[th])}" + (f" fine {_spread(fine[th])}" if th in fine else ""),
              flush=True)

    raster = min(t["raster"])
    pairs = F * n
    out = {"res": args.res, "verts": V, "faces": F, "views": n, "H": H, "W": W, "dilate": args.dilate,
           "reps": args.reps, "drawn_pixels": drawn, "agree": agree,
           "device_ms": {k: _spread(v) for k, v in t.items() if not k.startswith("host_")},
           "host_ms": {k[5:]: _spread(v) for k, v in t.items() if k.startswith("host_")},
           "raster_ms_per_view": round(raster / n, 3), "raster_gpairs_per_s": round(pairs / raster / 1e6, 2),
           "raster_read_gb_per_s": round(pairs * (3 * 16 + 12) / raster / 1e6, 1),
           "raster_atomics_lower_bound_per_s": round(2 * drawn / raster * 1e3),
           "cull_stats": dict(stats._replace(n_skipped=sum(stats.n_skipped))._asdict()),
           "big_face": {"coarse_res": args.coarse_res, "coarse_faces": int(cf.shape[0]),
                        "coarse_ms": {str(th): _spread(v) for th, v in coarse.items()},
                        "fine_ms": {str(th): _spread(v) for th, v in fine.items()}}}
    line = json.dumps({"mesh_cull": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not agree:
        raise SystemExit("mesh_cull_time.py: the host and device votes or meshes differ")


if __name__ == "__main__":
    main()
