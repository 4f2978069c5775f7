"""Time and quality of simplifying the fine mesh by vertex clustering - on the GPU (csrc/hm_mesh_simplify.hip,
ops.mesh_simplify) and on the host with the numpy restatement of the same contract (tests/mesh_simplify_cases.py).

    python scripts/mesh_simplify_time.py [--res 512 1024] [--k 2 4] [--reps 3] [--out FILE]

The mesh is the device mesh of get_surface_high_res_mesh(resolution, sparse=True) on the C2 network of bench.py
(geometric init, seed 0: the network setup of scripts/mesh_extract_time.py), as ops.marching_cubes_sparse returns it:
in lattice coordinates, the lattice spacing d apart.  Per mesh and k the cell is k d; after a warm-up, --reps times:
  (a) device: ops.mesh_simplify (quadric placement) + download of its four outputs
  (b) host, once: download of vertices, faces and normals + mesh_simplify_cases.simplify
both as wall clock from a synchronised device to the arrays in host memory.  The two results are compared: integer
outputs equal, positions within 2^-22 max|coord|.
Quality, for both placements: the one-sided distance from the simplified mesh to the original one, mean and maximum
over the points of ops.mesh_sample_surface(simplified, d/2) of the distance to the nearest point of
ops.mesh_sample_surface(original, d/8) (ops.nn_index), in units of d.  The distance is to a point cloud, not to the
surface: "floor" is the same figure for the original mesh's own d/2 samples, what a perfect simplification would show.
No GPU: exits with an error instead of printing a number.  Prints a line per mesh and k, then one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def fine_mesh(net, res):
    """the device (verts, faces, normals) ops.marching_cubes_sparse hands to get_surface_high_res_mesh(res, sparse),
    and the lattice spacing it was called with"""
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd.utils import plots
    kept = []
    orig = ops.marching_cubes_sparse

    def capture(sdf, axes, spacing, *a, **k):
        kept.append((orig(sdf, axes, spacing, *a, **k), float(spacing[0])))
        return kept[-1][0]

    ops.marching_cubes_sparse = capture
    try:
        if plots.get_surface_high_res_mesh(net.sdf, res, sparse=True) is None:
            raise SystemExit("get_surface_high_res_mesh found no surface")
    finally:
        ops.marching_cubes_sparse = orig
    mesh, d = kept[-1]
    return tuple(t.contiguous() for t in mesh[:3]), d


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def device_simplify(mesh, cell, placement="quadric"):
    from hashmodnffbanks_idr_amd import ops
    return tuple(t.cpu().numpy() for t in ops.mesh_simplify(*mesh, cell=cell, placement=placement))


def host_simplify(mesh, cell):
    import mesh_simplify_cases as S
    verts, faces, normals = (t.cpu().numpy() for t in mesh)
    return S.simplify(verts, faces, normals, cell)


def one_sided(verts, faces, index, d):
    """(mean, max) / d of the distances from the mesh's d/2 samples to the indexed cloud"""
    from hashmodnffbanks_idr_amd import ops
    d2, _ = index.query(ops.mesh_sample_surface(verts, faces, 0.5 * d))
    dist = d2.double().sqrt() / d
    return round(float(dist.mean()), 4), round(float(dist.max()), 4)


def time_mesh(name, mesh, d, ks, reps):
    import numpy as np
    from hashmodnffbanks_idr_amd import ops
    index = ops.nn_index(ops.mesh_sample_surface(mesh[0], mesh[1], 0.125 * d))
    floor = one_sided(mesh[0], mesh[1], index, d)
    max_coord = float(mesh[0].abs().max())
    runs = []
    for k in ks:
        cell = k * d
        for _ in range(2):                                   # warm-up: code objects, allocator
            device_simplify(mesh, cell)
        dev = []
        for _ in range(reps):
            (dv, df, dn, dm), t = _wall(lambda: device_simplify(mesh, cell))
            dev.append(round(t, 2))
        ref, host = _wall(lambda: host_simplify(mesh, cell))
        equal = bool(np.array_equal(df, ref["faces"]) and np.array_equal(dm, ref["vertex_map"])
                     and dv.shape == ref["verts"].shape
                     and np.all(np.abs(dv.astype(np.float64) - ref["verts"]) <= 2.0 ** -22 * max_coord)
                     and np.all(np.abs(dn.astype(np.float64) - ref["normals"]) <= 2.0 ** -22))
        quality = {}
        for placement in ("quadric", "mean"):
            v, f, _, _ = ops.mesh_simplify(*mesh, cell=cell, placement=placement)
            quality[placement] = one_sided(v, f, index, d)
        out = {"mesh": name, "k": k, "faces_in": int(mesh[1].shape[0]), "verts_in": int(mesh[0].shape[0]),
               "faces_out": int(len(df)), "verts_out": int(len(dv)), "device_ms": dev, "device_best_ms": min(dev),
               "host_ms": round(host, 1), "equal": equal, "floor_mean_max_d": floor,
               "quadric_mean_max_d": quality["quadric"], "mean_mean_max_d": quality["mean"]}
        runs.append(out)
        print(f"{name} k={k}: F {out['faces_in']} -> {out['faces_out']}, V {out['verts_in']} -> {out['verts_out']}; "
              f"device {min(dev):.2f} ms {dev}, host {host:.0f} ms; equal {equal}; distance to the original / d "
              f"(mean, max): quadric {quality['quadric']}, mean {quality['mean']}, floor {floor}", flush=True)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--k", type=float, nargs="*", default=[2.0, 4.0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_simplify_time.py: no GPU - nothing is measured")
    import bench
    net = bench._build("C2", "cuda", 0.0).implicit_network
    runs = []
    for res in args.res:
        mesh, d = fine_mesh(net, res)
        runs += time_mesh(f"C2_sparse_{res}", mesh, d, args.k, args.reps)
        del mesh
        torch.cuda.empty_cache()
    line = json.dumps({"runs": runs})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
