"""Time and quality of baking a per-face texture atlas of a simplified mesh from the input views on the GPU
(evaluation.texture.texture_mesh: csrc/hm_mesh_texture.hip on csrc/hm_mesh_color.hip) beside vertex colours.

    python scripts/mesh_texture_time.py [--res 512] [--k 2 4] [--tex-res 8] [--views 49] [--height 1200] [--width 1600]
                                        [--reps 5] [--out FILE]

No data files.  The fine mesh and the cameras are mesh_color_time.py's (ops.marching_cubes of the analytic bumpy sphere
at --res; --views look_at cameras on a dome).  The photographs carry an analytic surface pattern: the FINE mesh is drawn
with its positions as attributes (ops.mesh_render) and every covered pixel shows pattern(position), 0.8 sin(120 x +
phase) per channel - a period of 0.052: 13 lattice spacings at --res 512 and about 35 pixels; the masks are the covered
pixels.  (Noise photographs say nothing about quality.)  Per k the fine mesh is simplified at a cell of k lattice
spacings (ops.mesh_simplify) and, after a warm-up, --reps times as wall clock from a synchronised device to a
synchronised device:
  points    ops.mesh_texture_points at --tex-res
  bake      ops.mesh_vertex_colors over the texels' points, all views resident (texel-view pairs/s), beside
  vertices  ops.mesh_vertex_colors over the mesh's own vertices (vertex-view pairs/s): the same kernel
  sampler   ops.mesh_texture_sample of all views' pixels, beside
  render    ops.mesh_render of the same views with three attributes, and with the weights alone
  texture_mesh   as a whole, from the host's images to the atlas
and once: evaluate_mesh_views textured and vertex-coloured (PSNR and SSIM against the photographs).  The host
restatement (tests/mesh_texture_cases.py) of the points and of the sampler (one view) must equal the device's bits for
the coarsest mesh, else the script fails.  No GPU: exits with an error instead of printing a number.  Prints a line per
repetition, then one JSON line."""
import argparse
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from chamfer_time import _wall, bumpy_sphere  # noqa: E402  (scripts/ is sys.path[0])
from mesh_cull_time import _spread, dome_cameras  # noqa: E402

PATTERN_FREQ = 120.0


class _Views:
    """what evaluate_mesh_views reads of a SceneDataset, the photographs and masks on the device"""

    def __init__(self, K, pose, images, masks, H, W):
        import torch
        self.img_res = [H, W]
        self.intrinsics_all = [torch.from_numpy(k) for k in K]
        self.pose_all = [torch.from_numpy(p) for p in pose]
        self.rgb_images = [im.reshape(-1, 3) for im in images]
        self.object_masks = [m.reshape(-1) for m in masks]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--k", type=float, nargs="*", default=[2.0, 4.0])
    ap.add_argument("--tex-res", type=int, default=8)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_texture_time.py: no GPU - nothing is measured")
    import mesh_texture_cases as TC
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd.evaluation import (color_mesh, evaluate_mesh_views, texture_mesh, view_projections)

    H, W, n, R = args.height, args.width, args.views, args.tex_res
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
    # the photographs: the analytic pattern at the fine mesh's surface point under every pixel, white elsewhere
    phase = torch.tensor([0.0, 1.0, 2.0], device="cuda")
    dimages = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda")
    masks = torch.empty((n, H, W), dtype=torch.bool, device="cuda")
    for v in range(n):
        r = ops.mesh_render(verts, faces, dproj[v:v + 1], H, W, attrs=verts)
        masks[v] = r.face_id[0] >= 0
        dimages[v] = torch.where(masks[v][..., None], 0.8 * torch.sin(PATTERN_FREQ * r.image[0] + phase), 1.0)
    host_images = [im.reshape(-1, 3).cpu() for im in dimages]                # as SceneDataset.rgb_images
    host_masks = masks.cpu()
    data = _Views(K, pose, dimages, masks, H, W)
    print(f"fine mesh: V {int(verts.shape[0])}, F {int(faces.shape[0])}; {n} views {H} x {W}; texture res {R}", flush=True)

    results, agree = [], True
    for k in args.k:
        mv, mf, mn, _ = ops.mesh_simplify(verts, faces, normals, cell=k * spacing[0])
        V, F = int(mv.shape[0]), int(mf.shape[0])
        mesh = (mv, mf, mn)
        depth, _ = ops.mesh_depth_maps(mv, mf, dproj, H, W)
        pts, pn, owner = ops.mesh_texture_points(mv, mf, R, mn)
        T = int(pts.shape[0])
        kw = dict(erode=1, pad=1, tol=0.0, min_cos=0.0, power=1)

        def bake():
            return ops.mesh_vertex_colors(pts, pn, dproj, dcenters, dimages, depth, masks=masks, **kw)

        def vertices():
            return ops.mesh_vertex_colors(mv, mn, dproj, dcenters, dimages, depth, masks=masks, **kw)

        def whole():
            return texture_mesh(mesh, K, pose, host_images, (H, W), res=R, masks=host_masks, device=mv.device, **kw)

        atlas, stats = whole()                                               # warm-up of every timed call
        unit = ((atlas.texels + 1.0) / 2.0).clamp(0.0, 1.0).contiguous()
        colors, _ = color_mesh(mesh, K, pose, dimages, (H, W), masks=masks, **kw)
        attrs = ((colors + 1.0) / 2.0).clamp(0.0, 1.0).contiguous()
        ren = ops.mesh_render(mv, mf, dproj, H, W, return_weights=True)
        bake(), vertices(), ops.mesh_texture_sample(unit, R, F, ren.face_id, ren.weights, 1.0)
        ops.mesh_render(mv, mf, dproj, H, W, attrs=attrs, background=1.0)
        names = ["points", "bake", "vertices", "sampler", "render_weights", "render_attrs", "texture_mesh"]
        t = {name: [] for name in names}
        for _ in range(args.reps):
            gc.collect()
            t["points"].append(_wall(lambda: ops.mesh_texture_points(mv, mf, R, mn))[1])
            t["bake"].append(_wall(bake)[1])
            t["vertices"].append(_wall(vertices)[1])
            t["sampler"].append(_wall(lambda: ops.mesh_texture_sample(unit, R, F, ren.face_id, ren.weights, 1.0))[1])
            t["render_weights"].append(_wall(lambda: ops.mesh_render(mv, mf, dproj, H, W, return_weights=True))[1])
            t["render_attrs"].append(_wall(lambda: ops.mesh_render(mv, mf, dproj, H, W, attrs=attrs, background=1.0))[1])
            t["texture_mesh"].append(_wall(whole)[1])
            print(f"k {k}:", {name: round(v[-1], 2) for name, v in t.items()}, flush=True)
        del ren
        textured = evaluate_mesh_views(mesh, data, texture=atlas)
        plain = evaluate_mesh_views(mesh, data, colors=colors)
        print(f"k {k}: V {V}, F {F}, texels {T}; {stats._replace(n_skipped=sum(stats.n_skipped))}; PSNR / SSIM textured "
              f"{textured.psnr_mean:.2f} / {textured.ssim_mean:.4f}, vertex colours {plain.psnr_mean:.2f} / "
              f"{plain.ssim_mean:.4f}", flush=True)
        results.append({"k": k, "verts": V, "faces": F, "texels": T, "n_colored": stats.n_colored,
                        "ms": {name: _spread(v) for name, v in t.items()},
                        "bake_gpairs_per_s": round(T * n / min(t["bake"]) / 1e6, 2),
                        "vertices_gpairs_per_s": round(V * n / min(t["vertices"]) / 1e6, 2),
                        "sampler_gpixels_per_s": round(n * H * W / min(t["sampler"]) / 1e6, 2),
                        "psnr_textured": round(textured.psnr_mean, 3), "ssim_textured": round(textured.ssim_mean, 4),
                        "psnr_vertex_colors": round(plain.psnr_mean, 3), "ssim_vertex_colors": round(plain.ssim_mean, 4)})
        last = (mv, mf, mn, pts, pn, owner, unit, F)

    # the host restatement against the device's bits, on the last (coarsest) mesh: the points, and one view's samples
    mv, mf, mn, pts, pn, owner, unit, F = last
    want = TC.texel_points_ref(mv.cpu().numpy(), mf.cpu().numpy(), R, mn.cpu().numpy())
    same = (np.array_equal(want[0].view(np.int32), pts.cpu().numpy().view(np.int32))
            and np.array_equal(want[1].view(np.int32), pn.cpu().numpy().view(np.int32))
            and np.array_equal(want[2], owner.cpu().numpy()))
    print("host points agree with the device bit for bit:", same, flush=True)
    agree = agree and same
    ren = ops.mesh_render(mv, mf, dproj[:1], H, W, return_weights=True)
    got = ops.mesh_texture_sample(unit, R, F, ren.face_id, ren.weights, 1.0).cpu().numpy()
    ref = TC.texture_sample_ref(unit.cpu().numpy(), R, F, ren.face_id.cpu().numpy(), ren.weights.cpu().numpy(), 1.0)
    same = np.array_equal(ref.view(np.int32), got.view(np.int32))
    print("host samples agree with the device bit for bit:", same, flush=True)
    agree = agree and same

    out = {"res": args.res, "tex_res": R, "views": n, "H": H, "W": W, "reps": args.reps, "agree": agree,
           "meshes": results}
    line = json.dumps({"mesh_texture": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not agree:
        raise SystemExit("mesh_texture_time.py: the host restatement and the device differ")


if __name__ == "__main__":
    main()
