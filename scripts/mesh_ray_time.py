"""Time of casting camera rays at an extracted mesh on the GPU (csrc/hm_mesh_ray.hip: ops.mesh_index(pad=...),
MeshIndex.ray_cast, evaluation.cast_camera_rays) beside the rasteriser, and what the depth on the tracer's rays sees
of simplification.

    python scripts/mesh_ray_time.py [--res 512] [--views 49] [--height 1200] [--width 1600] [--sweep-views 4]
                                    [--agree-views 3] [--reps 3] [--out FILE]

No data files.  The mesh and the cameras are mesh_render_time.py's: ops.marching_cubes of the analytic bumpy sphere at
--res (d its lattice spacing), --views look_at cameras on a dome.  The rays are ops.camera_rays' through the pixel
centres, cast inside the bounding sphere of radius 1 (the tracer's domain), view by view.  As wall clock from a
synchronised device to a synchronised device, after a warm-up:
  build    ops.mesh_ray_index: the default pad (ops.mesh_ray_pad) and mesh_ray_cast's default cell edge
  cast     all views in pixel order: rays/s and (ray, face) tests per ray; the same rays of --sweep-views views
           shuffled, beside those views in pixel order
  sweep    the cell edge over 1, 2, 3, 4, 6 and 8 d on --sweep-views views: build, pairs, rays/s, tests per ray
  render   ops.mesh_render's face ids and depth of all views in the same run, the reference point, and on how many
           of the pixels both cover the ray cast reports the rendered face
  agree    evaluation.depth_agreement on the rays of --agree-views views: the mesh at simplify 0 against the
           analytic field's own first zero along each ray (sphere-traced in fp64 with torch, the field being
           1.42-Lipschitz: a stand-in for a trained network's sphere-traced dists, which this script has none of), and
           the meshes simplified at cell = 2 d and 4 d against both; beyond_1d counts the rays on which the two
           depths differ by more than d (a ray that slips between two faces meets the far side: no watertightness
           is claimed)
No GPU: exits with an error instead of printing a number.  Prints a line per measurement, then one JSON line."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from chamfer_time import _wall, bumpy_sphere  # noqa: E402  (scripts/ is sys.path[0])
from mesh_cull_time import dome_cameras  # noqa: E402


def field_depth(cam, dirs, t0, t1, iters=160):
    """the first zero of the bumpy sphere's field along the unit rays within [t0, t1], by sphere tracing in fp64 with
    steps f / 1.5 (the field is 1.42-Lipschitz, so no step passes a zero); (t, hit)"""
    import torch
    o, d = cam.double(), dirs.double()
    t = t0.double().clone()
    for _ in range(iters):
        p = o + t[:, None] * d
        f = p.norm(dim=1) - 0.6 - 0.04 * torch.sin(7 * p[:, 0]) * torch.sin(6 * p[:, 1]) * torch.sin(5 * p[:, 2])
        t = torch.minimum(t + f / 1.5, t1.double())
    p = o + t[:, None] * d
    f = p.norm(dim=1) - 0.6 - 0.04 * torch.sin(7 * p[:, 0]) * torch.sin(6 * p[:, 1]) * torch.sin(5 * p[:, 2])
    hit = (f.abs() < 1e-7) & (t < t1.double())
    return torch.where(hit, t, torch.full_like(t, math.inf)).float(), hit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--sweep-views", type=int, default=4)
    ap.add_argument("--agree-views", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_ray_time.py: no GPU - nothing is measured")
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd.evaluation import depth_agreement, view_projections

    H, W, n = args.height, args.width, args.views
    vol, spacing = bumpy_sphere(args.res)
    verts, faces, normals = ops.marching_cubes(vol, 0.0, spacing)
    verts = (verts - 1.0).contiguous()          # the lattice of [-1, 1]^3
    del vol
    d = spacing[0]
    K, pose = dome_cameras(n, H, W)
    Kd, posed = torch.from_numpy(K).cuda(), torch.from_numpy(pose).cuda()
    row, col = torch.meshgrid(torch.arange(H, dtype=torch.float32, device="cuda"),
                              torch.arange(W, dtype=torch.float32, device="cuda"), indexing="ij")
    uv = torch.stack([col, row], -1).reshape(1, -1, 2).contiguous()
    V, F, N = int(verts.shape[0]), int(faces.shape[0]), H * W
    pad = ops.mesh_ray_pad(verts)
    print(f"mesh: V {V}, F {F}, d {d:.6f}, pad {pad:.3e} ({pad / d:.3f} d); {n} views {H} x {W}", flush=True)

    def rays(v):
        dirs, cam, ts, inside = ops.camera_rays(uv, posed[v:v + 1], Kd[v:v + 1], 1.0)
        inside = inside.reshape(-1)
        one, zero = torch.ones((), device="cuda"), torch.zeros((), device="cuda")
        return (cam.expand(N, 3).contiguous(), dirs.reshape(N, 3), torch.where(inside, ts[0, :, 0], one).contiguous(),
                torch.where(inside, ts[0, :, 1], zero).contiguous())

    def cast_views(index, views, shuffle=False, keep=False):
        """(ms, tests, [(t, face)]) of casting the views' rays, the rays made outside the clock"""
        ms, tests, out = 0.0, 0, []
        for v in views:
            o, dr, t0, t1 = rays(v)
            if shuffle:
                perm = torch.randperm(N, device="cuda", generator=gen)
                o, dr, t0, t1 = (x[perm].contiguous() for x in (o, dr, t0, t1))
            stats = {}
            r, t_ms = _wall(lambda: index.ray_cast(o, dr, t0, t1, return_uv=False))
            index.ray_cast(o, dr, t0, t1, return_uv=False, stats=stats)
            ms, tests = ms + t_ms, tests + stats["face_tests"]
            if keep:
                out.append(r)
        return ms, tests, out

    gen = torch.Generator(device="cuda").manual_seed(0)
    build = lambda cell=None: ops.mesh_ray_index(verts, faces, cell, pad=pad)  # noqa: E731
    index = build()
    build_ms = [round(_wall(build)[1], 2) for _ in range(args.reps)]
    idx = {"build_ms": build_ms, "pairs": index.n_pairs, "big_faces": index.n_big, "grid": index.g,
           "cell_d": round(index.h / d, 3)}
    print("index:", idx, flush=True)

    all_views, some = list(range(n)), list(range(0, n, max(1, n // args.sweep_views)))[:args.sweep_views]
    cast_views(index, some[:1])                                                       # warm-up
    ms, tests, kept = cast_views(index, all_views, keep=True)
    hits = sum(int((f >= 0).sum()) for _, f in kept)
    cast = {"ms": round(ms, 2), "mrays_per_s": round(n * N / ms / 1e3, 2), "tests_per_ray": round(tests / n / N, 2),
            "hit_share": round(hits / n / N, 4)}
    print("cast, pixel order, all views:", cast, flush=True)
    ms_o, tests_o, _ = cast_views(index, some)
    ms_s, tests_s, _ = cast_views(index, some, shuffle=True)
    order = {"views": len(some), "pixel_order_mrays_per_s": round(len(some) * N / ms_o / 1e3, 2),
             "shuffled_mrays_per_s": round(len(some) * N / ms_s / 1e3, 2),
             "tests_per_ray": (round(tests_o / len(some) / N, 2), round(tests_s / len(some) / N, 2))}
    print("cast, pixel order against shuffled:", order, flush=True)

    sweep = []
    for k in (1, 2, 3, 4, 6, 8):
        ix, b_ms = _wall(lambda: build(k * d))
        cast_views(ix, some[:1])
        ms_k, tests_k, _ = cast_views(ix, some)
        sweep.append({"cell_d": k, "build_ms": round(b_ms, 2), "pairs": ix.n_pairs, "big_faces": ix.n_big,
                      "mrays_per_s": round(len(some) * N / ms_k / 1e3, 2),
                      "tests_per_ray": round(tests_k / len(some) / N, 2)})
        print("sweep:", sweep[-1], flush=True)
        del ix
        torch.cuda.empty_cache()

    dproj = torch.from_numpy(view_projections(K, pose)).cuda()
    ops.mesh_render(verts, faces, dproj[:1], H, W)
    ren, ren_ms = _wall(lambda: ops.mesh_render(verts, faces, dproj, H, W))
    both = same = 0
    for v in all_views:
        fr, fc = ren.face_id[v].reshape(-1), kept[v][1]
        b = (fr >= 0) & (fc >= 0)
        both, same = both + int(b.sum()), same + int((b & (fr == fc)).sum())
    render = {"ms": round(ren_ms, 2), "mpixels_per_s": round(n * N / ren_ms / 1e3, 2),
              "cast_over_render": round(cast["ms"] / ren_ms, 1), "covered_by_both": both,
              "same_face_share": round(same / max(both, 1), 5)}
    print("mesh_render, face ids and depth, all views:", render, flush=True)
    del ren, kept
    torch.cuda.empty_cache()

    agree = []
    meshes = {0: (verts, faces)}
    for k in (2, 4):
        sv, sf, _, _ = ops.mesh_simplify(verts, faces, normals, cell=k * d)
        meshes[k] = (sv, sf)
    pick = list(range(0, n, max(1, n // args.agree_views)))[:args.agree_views]
    depth = {k: [] for k in meshes}
    field = []
    for v in pick:
        o, dr, t0, t1 = rays(v)
        field.append(field_depth(o, dr, t0, t1))
    for k, (mv, mf) in meshes.items():
        ix = ops.mesh_ray_index(mv, mf)
        for v in pick:
            o, dr, t0, t1 = rays(v)
            t, f = ix.ray_cast(o, dr, t0, t1, return_uv=False)
            depth[k].append((t, f >= 0))
    cat = lambda pairs: (torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs]))  # noqa: E731
    ft, fh = cat(field)
    for k in meshes:
        mt, mh = cat(depth[k])
        a = depth_agreement(mt, mh, ft, fh)
        far = lambda t, h: int(((mh & h) & ((mt.double() - t.double()).abs() > d)).sum())  # noqa: E731
        row = {"simplify_cell_d": k, "faces": int(meshes[k][1].shape[0]), "rays": a.n,
               "against_field": {"n_both": a.n_both, "iou": round(a.iou, 6), "mean_d": round(a.mean / d, 5),
                                 "median_d": round(a.median / d, 5), "max_d": round(a.max / d, 4),
                                 "beyond_1d": far(ft, fh)}}
        if k:
            b = depth_agreement(mt, mh, *cat(depth[0]))
            row["against_mesh_0"] = {"n_both": b.n_both, "iou": round(b.iou, 6), "mean_d": round(b.mean / d, 5),
                                     "median_d": round(b.median / d, 5), "max_d": round(b.max / d, 4),
                                     "beyond_1d": far(*cat(depth[0]))}
        agree.append(row)
        print("agree:", row, flush=True)

    out = {"res": args.res, "verts": V, "faces": F, "views": n, "H": H, "W": W, "pad_d": round(pad / d, 4),
           "index": idx, "cast": cast, "order": order, "sweep": sweep, "render": render, "agree": agree,
           "network_tracer": "not measured"}
    line = json.dumps({"mesh_ray": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
