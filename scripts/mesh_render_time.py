"""Time of drawing an extracted mesh into the input views on the GPU (ops.mesh_render: csrc/hm_mesh_render.hip) beside
the depth maps of the same run (ops.mesh_depth_maps), and of scoring the coloured mesh against photographs
(evaluation.evaluate_mesh_views).

    python scripts/mesh_render_time.py [--res 512] [--views 49] [--height 1200] [--width 1600] [--reps 5] [--out FILE]

No data files.  The mesh and the cameras are mesh_cull_time.py's: ops.marching_cubes of the analytic bumpy sphere at
--res, --views look_at cameras on a dome.  The vertex colours are the positions scaled into [-1, 1]; the "photographs"
are the mesh's own render plus 0.1 inside the mask of its covered pixels (a timing input whose PSNR is known:
20 log10(2 / 0.1) = 26.02 dB), held on the host per view as a SceneDataset holds them.  After a warm-up, --reps times
alternately, as wall clock from a synchronised device to a synchronised device:
  ops.mesh_depth_maps of all views
  ops.mesh_render of all views without attributes (face ids and depth)
  ops.mesh_render of all views with 3 attributes and the weights
each in ms and in (face, view) pairs per second, and evaluate_mesh_views of all views (the upload of every photograph
and mask, the render, PSNR and SSIM) per view.  The depth of the renders must equal the depth maps bit for bit, else
the script fails.  No GPU: exits with an error instead of printing a number.  Prints a line per repetition, then one
JSON line."""
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


class _Views:
    """what evaluate_mesh_views reads of a SceneDataset"""

    def __init__(self, K, pose, images, masks, img_res):
        self.intrinsics_all, self.pose_all, self.rgb_images, self.object_masks = K, pose, images, masks
        self.img_res = img_res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_render_time.py: no GPU - nothing is measured")
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd.evaluation import evaluate_mesh_views, render_mesh, view_projections

    H, W, n = args.height, args.width, args.views
    vol, spacing = bumpy_sphere(args.res)
    verts, faces, _ = ops.marching_cubes(vol, 0.0, spacing)
    verts = (verts - 1.0).contiguous()          # the lattice of [-1, 1]^3
    del vol
    K, pose = dome_cameras(n, H, W)
    dproj = torch.from_numpy(view_projections(K, pose)).cuda()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    colors = (verts / verts.abs().max()).contiguous()
    attrs = ((colors + 1.0) / 2.0).contiguous()

    depth, _ = ops.mesh_depth_maps(verts, faces, dproj, H, W)                       # warm-ups, and the same bits
    bare = ops.mesh_render(verts, faces, dproj, H, W)
    full = ops.mesh_render(verts, faces, dproj, H, W, attrs=attrs, background=1.0, return_weights=True)
    same = all(torch.equal(r.depth.view(torch.int32), depth.view(torch.int32)) for r in (bare, full))
    drawn = int((bare.face_id >= 0).sum())
    print(f"mesh: V {V}, F {F}; {n} views {H} x {W}; drawn pixels {drawn} ({drawn / n / H / W:.3f} of the images); "
          f"depth bits equal: {same}", flush=True)
    del bare, full, depth

    Kt, pt = torch.from_numpy(K), torch.from_numpy(pose)
    images, masks = [], []
    for v in range(n):                                                          # view by view: 23 MB each on the host
        own = render_mesh((verts, faces), Kt[v:v + 1], pt[v:v + 1], (H, W), colors=colors)
        masks.append(own.coverage[0].reshape(-1).cpu())
        images.append((own.rgb[0] * 2.0 - 1.0 + 0.1 * own.coverage[0][..., None]).reshape(-1, 3).cpu())
    data = _Views(list(Kt), list(pt), images, masks, (H, W))
    scores = evaluate_mesh_views((verts, faces), data, colors=colors)               # warm-up of the metrics
    print(f"evaluate_mesh_views: PSNR {scores.psnr_mean:.4f} dB (26.0206 expected), SSIM {scores.ssim_mean:.4f}",
          flush=True)

    t = {k: [] for k in ("depth_maps", "render", "render_attrs_weights", "evaluate_mesh_views")}
    for _ in range(args.reps):
        gc.collect()
        t["depth_maps"].append(_wall(lambda: ops.mesh_depth_maps(verts, faces, dproj, H, W))[1])
        t["render"].append(_wall(lambda: ops.mesh_render(verts, faces, dproj, H, W))[1])
        t["render_attrs_weights"].append(_wall(lambda: ops.mesh_render(verts, faces, dproj, H, W, attrs=attrs,
                                                                       background=1.0, return_weights=True))[1])
        t["evaluate_mesh_views"].append(_wall(lambda: evaluate_mesh_views((verts, faces), data, colors=colors))[1])
        print({k: round(v[-1], 2) for k, v in t.items()}, flush=True)

    pairs = F * n
    out = {"res": args.res, "verts": V, "faces": F, "views": n, "H": H, "W": W, "reps": args.reps,
           "drawn_pixels": drawn, "depth_bits_equal": same, "psnr_mean": scores.psnr_mean,
           "ms": {k: _spread(v) for k, v in t.items()},
           "gpairs_per_s": {k: round(pairs / min(v) / 1e6, 2) for k, v in t.items() if k != "evaluate_mesh_views"},
           "render_over_depth_maps": round(min(t["render"]) / min(t["depth_maps"]), 2),
           "render_attrs_weights_over_depth_maps": round(min(t["render_attrs_weights"]) / min(t["depth_maps"]), 2),
           "evaluate_ms_per_view": round(min(t["evaluate_mesh_views"]) / n, 2)}
    line = json.dumps({"mesh_render": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not same or abs(scores.psnr_mean - 26.0206) > 1e-3:
        raise SystemExit("mesh_render_time.py: the render's depth differs from the depth maps, or the PSNR is off")


if __name__ == "__main__":
    main()
