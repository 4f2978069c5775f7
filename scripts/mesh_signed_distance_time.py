"""Time of the signed point-to-mesh distance on the GPU (csrc/hm_mesh_topo.hip: ops.mesh_topology,
ops.MeshIndex.signed_distance) beside the unsigned query it is built on, and what the sign makes measurable.

    python scripts/mesh_signed_distance_time.py [--res 512] [--target 2000000] [--k 2 4] [--iou-res 128] [--reps 3]
                                                [--out FILE]

No data files: the mesh and the target cloud are those of scripts/mesh_distance_time.py (ops.marching_cubes of the
analytic bumpy sphere at --res, d its lattice spacing; --target seeded vertices moved by normal noise of two spacings).
After a warm-up of every step, --reps times each, as wall clock from a synchronised device to a synchronised device:
  topology   ops.mesh_topology(mesh): the build, and the three edge counts
  query      index.query(target) with point and feature - what the signed query runs first - and
             index.signed_distance(target, topology, return_sign=True) in the same run; their difference is the sign
             pass, one lane per query
and, once,
  volume_iou of the mesh against ops.mesh_simplify at cell = k d, on an --iou-res^3 lattice (allow_open: the counts of
             the simplified mesh's edges are reported beside it)
  sdf_agreement of the analytic field the mesh was extracted from against the mesh's signed distance at the target.
No GPU: exits with an error instead of printing a number.  Prints a line per measurement, then one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--target", type=int, default=2000000)
    ap.add_argument("--k", type=float, nargs="*", default=[2.0, 4.0])
    ap.add_argument("--iou-res", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_signed_distance_time.py: no GPU - nothing is measured")
    from chamfer_time import _wall, bumpy_sphere
    from mesh_distance_time import timed
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd.evaluation import sdf_agreement, volume_iou

    vol, spacing = bumpy_sphere(args.res)
    verts, faces, normals = ops.marching_cubes(vol, 0.0, spacing)
    del vol
    torch.cuda.empty_cache()
    d = spacing[0]
    gen = torch.Generator().manual_seed(0)
    pick = torch.randint(0, verts.shape[0], (args.target,), generator=gen).cuda()
    noise = torch.randn((args.target, 3), generator=gen).cuda() * (2.0 * d)
    target = (verts[pick] + noise).contiguous()
    m = int(target.shape[0])
    print(f"mesh: V {verts.shape[0]}, F {faces.shape[0]}, d {d:.6f}; target {m}", flush=True)

    def edges(t):
        return {"boundary": t.boundary_edges, "nonmanifold": t.nonmanifold_edges, "flipped": t.flipped_edges,
                "closed": t.closed}

    topo, topo_ms = timed(lambda: ops.mesh_topology(verts, faces), args.reps)
    topology = {"build_ms": topo_ms, "build_best_ms": min(topo_ms), **edges(topo)}
    print("topology:", topology, flush=True)

    index, build_ms = timed(lambda: ops.mesh_index(verts, faces), args.reps)
    _, unsigned_ms = timed(lambda: index.query(target, return_feature=True), args.reps)
    (sd, sign), signed_ms = timed(lambda: index.signed_distance(target, topo, return_sign=True), args.reps)
    query = {"index_build_ms": build_ms, "unsigned_ms": unsigned_ms, "unsigned_best_ms": min(unsigned_ms),
             "signed_ms": signed_ms, "signed_best_ms": min(signed_ms),
             "sign_pass_ms": round(min(signed_ms) - min(unsigned_ms), 2),
             "inside_share": round(float((sign < 0).double().mean()), 5)}
    print("query:", query, flush=True)

    # the analytic field the mesh is the zero set of, against the mesh's signed distance
    # (marching_cubes puts the lattice's first point at the origin: the field's coordinates are the mesh's minus one)
    x, y, z = target[:, 0] - 1.0, target[:, 1] - 1.0, target[:, 2] - 1.0
    field = (torch.sqrt(x * x + y * y + z * z) - 0.6 - 0.04 * torch.sin(7 * x) * torch.sin(6 * y) * torch.sin(5 * z))
    agree = sdf_agreement(field.contiguous(), sd)
    banded = sdf_agreement(field.contiguous(), sd, band=d)
    agreement = {"n_used": agree.n_used, "sign_agreement": round(agree.sign_agreement, 6),
                 "mean_d": round(agree.mean / d, 5), "median_d": round(agree.median / d, 5),
                 "max_d": round(agree.max / d, 4),
                 "band_1d": {"n_used": banded.n_used, "sign_agreement": round(banded.sign_agreement, 6),
                             "mean_d": round(banded.mean / d, 5)}}
    print("sdf_agreement:", agreement, flush=True)

    iou = []
    for k in args.k:
        sv, sf, _, _ = ops.mesh_simplify(verts, faces, normals, cell=k * d)
        pair = (ops.mesh_index(sv, sf), ops.mesh_topology(sv, sf))
        (value, vol_a, vol_b, vol_both), t = _wall(lambda: volume_iou((index, topo), pair, res=args.iou_res,
                                                                      allow_open=True))
        iou.append({"k": k, "faces_out": int(sf.shape[0]), **edges(pair[1]), "iou": round(value, 6),
                    "vol_mesh": round(vol_a, 6), "vol_simplified": round(vol_b, 6), "vol_both": round(vol_both, 6),
                    "ms": round(t, 1)})
        print("volume_iou:", iou[-1], flush=True)

    out = {"res": args.res, "verts": int(verts.shape[0]), "faces": int(faces.shape[0]), "target": m,
           "topology": topology, "query": query, "sdf_agreement": agreement, "volume_iou": iou,
           "iou_res": args.iou_res}
    line = json.dumps({"mesh_signed_distance": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
