"""Time of the exact point-to-mesh distance on the GPU (csrc/hm_mesh_dist.hip: ops.mesh_index,
ops.mesh_closest_point) beside the routes it replaces, and the simplification error it can see.

    python scripts/mesh_distance_time.py [--res 512] [--target 2000000] [--k 2 4] [--reps 3] [--out FILE]

No data files: the mesh and the target cloud are those of scripts/chamfer_time.py (ops.marching_cubes of the analytic
bumpy sphere at --res, d its lattice spacing; --target seeded vertices moved by normal noise of two spacings).  After a
warm-up of every step, --reps times each, as wall clock from a synchronised device to a synchronised device:
  exact    ops.mesh_index(mesh) and index.query(target): the build, the query, the (query, face) tests per query, the
           faces listed in the grid (pairs) and in the big-face run
  sampled  today's route to "the distance to the surface": ops.mesh_sample_surface(mesh, d/8), ops.nn_index of the
           samples, its query by the target; the number of samples; and the route's floor as
           scripts/mesh_simplify_time.one_sided defines it - the distance, in d, that the mesh's own d/2 samples have
           to that cloud, where the exact route gives the rounding of fp32
  verts    ops.nn_index of the mesh's vertices and its query by the target: the cost of the same box walk with a
           point test instead of a triangle test
and, once, the error of ops.mesh_simplify at cell = k d as evaluation.chamfer.mesh_to_mesh measures it against the
original TRIANGLES (points of each mesh at density d/2; means and maxima in d), beside the figure of the sampled route
(scripts/mesh_simplify_time.one_sided against the d/8 cloud), which stops at its floor.
The exact and the sampled distances of the target are compared: the exact one is never larger (beyond fp32 rounding).
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


def timed(fn, reps):
    """(last result, [ms] * reps) after one warm-up call"""
    from chamfer_time import _wall
    fn()
    out, ms = None, []
    for _ in range(reps):
        out, t = _wall(fn)
        ms.append(round(t, 2))
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--target", type=int, default=2000000)
    ap.add_argument("--k", type=float, nargs="*", default=[2.0, 4.0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_distance_time.py: no GPU - nothing is measured")
    from chamfer_time import bumpy_sphere
    from mesh_simplify_time import one_sided
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd.evaluation import mesh_to_mesh

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

    # exact: the triangle grid
    index, build_ms = timed(lambda: ops.mesh_index(verts, faces), args.reps)
    (d2_exact, _, _), query_ms = timed(lambda: index.query(target), args.reps)
    stats = {}
    index._query(target, float("inf"), stats=stats)
    tests = stats["candidate_tests"]
    exact = {"build_ms": build_ms, "build_best_ms": min(build_ms), "query_ms": query_ms, "query_best_ms": min(query_ms),
             "tests_per_query": round(tests / m, 1), "gtests_per_s": round(tests / min(query_ms) / 1e6, 2),
             "pairs": index.n_pairs, "big_faces": index.n_big, "grid": index.g, "cell_d": round(index.h / d, 3)}
    print("exact:", exact, flush=True)

    # sampled: today's route
    samples, sample_ms = timed(lambda: ops.mesh_sample_surface(verts, faces, 0.125 * d), args.reps)
    cloud_index, cloud_build_ms = timed(lambda: ops.nn_index(samples), args.reps)
    (d2_cloud, _), cloud_query_ms = timed(lambda: cloud_index.query(target), args.reps)
    stats = {}
    cloud_index._query(target, float("inf"), stats)
    floor = one_sided(verts, faces, cloud_index, d)
    exact_floor = index.query(ops.mesh_sample_surface(verts, faces, 0.5 * d), return_point=False)[0].double().sqrt() / d
    sampled = {"samples": int(samples.shape[0]), "sample_ms": sample_ms, "build_ms": cloud_build_ms,
               "query_ms": cloud_query_ms, "total_best_ms": round(min(sample_ms) + min(cloud_build_ms)
                                                                  + min(cloud_query_ms), 2),
               "tests_per_query": round(stats["candidate_tests"] / m, 1), "floor_mean_max_d": floor,
               "exact_floor_mean_max_d": (float(f"{float(exact_floor.mean()):.3e}"),
                                          float(f"{float(exact_floor.max()):.3e}"))}
    print("sampled:", sampled, flush=True)
    gap = d2_cloud.double().sqrt() - d2_exact.double().sqrt()
    never_larger = bool(gap.min() >= -2.0 ** -22)
    compare = {"target_mean_exact_d": round(float(d2_exact.double().sqrt().mean()) / d, 5),
               "target_mean_sampled_d": round(float(d2_cloud.double().sqrt().mean()) / d, 5),
               "sampled_minus_exact_mean_max_d": (round(float(gap.mean()) / d, 5), round(float(gap.max()) / d, 5)),
               "exact_never_larger": never_larger}
    print("target:", compare, flush=True)
    del samples, cloud_index, d2_cloud
    torch.cuda.empty_cache()

    # verts: the same walk with a point test
    vert_index, vert_build_ms = timed(lambda: ops.nn_index(verts), args.reps)
    _, vert_query_ms = timed(lambda: vert_index.query(target), args.reps)
    stats = {}
    vert_index._query(target, float("inf"), stats)
    against_verts = {"build_ms": vert_build_ms, "query_ms": vert_query_ms, "query_best_ms": min(vert_query_ms),
                     "tests_per_query": round(stats["candidate_tests"] / m, 1)}
    print("verts:", against_verts, flush=True)

    # the simplification error, against the triangles and against the cloud
    cloud_index = ops.nn_index(ops.mesh_sample_surface(verts, faces, 0.125 * d))
    simplify = []
    for k in args.k:
        sv, sf, _, _ = ops.mesh_simplify(verts, faces, normals, cell=k * d)
        r = mesh_to_mesh((sv, sf), (verts, faces), 0.5 * d)
        simplify.append({"k": k, "faces_out": int(sf.shape[0]),
                         "to_original_mean_max_d": (round(r.mean_a2b / d, 5), round(r.max_a2b / d, 4)),
                         "from_original_mean_max_d": (round(r.mean_b2a / d, 5), round(r.max_b2a / d, 4)),
                         "sampled_route_mean_max_d": one_sided(sv, sf, cloud_index, d)})
        print("simplify:", simplify[-1], flush=True)

    out = {"res": args.res, "verts": int(verts.shape[0]), "faces": int(faces.shape[0]), "target": m, "exact": exact,
           "sampled": sampled, "target_distances": compare, "verts_nn": against_verts, "simplify": simplify}
    line = json.dumps({"mesh_distance": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not never_larger:
        raise SystemExit("mesh_distance_time.py: an exact distance exceeds the distance to the sampled cloud")


if __name__ == "__main__":
    main()
