"""Time of the fine mesh's cleanup - split into components, keep the one of the largest area (evaluation/eval.py) -
on the host as before and on the GPU (csrc/hm_mesh_cc.hip, ops.mesh_largest_component).

    python scripts/mesh_components_time.py [--res 512 1024] [--reps 3] [--noise 64] [--out FILE]

The mesh is the device mesh of get_surface_high_res_mesh(resolution, sparse=True) on the C2 network of bench.py
(geometric init, seed 0: the network setup of scripts/mesh_extract_time.py), taken as ops.marching_cubes_sparse
returns it.  --noise N adds the level-0 mesh of seeded normal noise on an N^3 lattice (ops.marching_cubes), a mesh
of thousands of components; 0 skips it.  Per mesh, after a warm-up of both, --reps times alternately:
  (a) host: download of vertices, faces and normals + TriMesh.split(only_watertight=False) + argmax of the areas
  (b) device: ops.mesh_largest_component + download of its result
both as wall clock from a synchronised device to the arrays in host memory, and (b)'s three steps (labels, areas,
select) between device synchronisations in one more call.  The two results are compared (they must be equal).
No GPU: exits with an error instead of printing a number.  Prints a line per mesh, then one JSON line.
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
    """the device (verts, faces, normals) ops.marching_cubes_sparse hands to get_surface_high_res_mesh(res, sparse)"""
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd.utils import plots
    kept = []
    orig = ops.marching_cubes_sparse

    def capture(*a, **k):
        kept.append(orig(*a, **k))
        return kept[-1]

    ops.marching_cubes_sparse = capture
    try:
        if plots.get_surface_high_res_mesh(net.sdf, res, sparse=True) is None:
            raise SystemExit("get_surface_high_res_mesh found no surface")
    finally:
        ops.marching_cubes_sparse = orig
    return tuple(t.contiguous() for t in kept[-1][:3])


def noise_mesh(n):
    import torch
    from hashmodnffbanks_idr_amd import ops
    vol = torch.ones(n, n, n)
    vol[1:-1, 1:-1, 1:-1] = torch.randn((n - 2,) * 3, generator=torch.Generator().manual_seed(1))
    return ops.marching_cubes(vol.cuda(), 0.0)


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def host_cleanup(verts, faces, normals):
    import numpy as np
    from hashmodnffbanks_idr_amd.utils.plots import TriMesh
    mesh = TriMesh(verts.cpu().numpy(), faces.cpu().numpy(), normals.cpu().numpy())
    parts = mesh.split(only_watertight=False)
    best = parts[int(np.argmax([p.area for p in parts]))]
    return best.vertices, best.faces, best.vertex_normals, len(parts)


def device_cleanup(verts, faces, normals):
    from hashmodnffbanks_idr_amd import ops
    return tuple(t.cpu().numpy() for t in ops.mesh_largest_component(verts, faces, normals))


def device_steps(verts, faces, normals):
    import torch
    from hashmodnffbanks_idr_amd import ops
    label, t_label = _wall(lambda: ops.mesh_components(faces, verts.shape[0]))
    (ids, area, _), t_area = _wall(lambda: ops.mesh_component_areas(verts, faces, label))
    best = int(ids[torch.argmax(area)].item())
    _, t_select = _wall(lambda: ops.mesh_select(verts, faces, normals, label, best))
    return {"labels_ms": round(t_label, 2), "areas_ms": round(t_area, 2), "select_ms": round(t_select, 2)}


def time_mesh(name, mesh, reps):
    import numpy as np
    for _ in range(2):                                   # warm-up: code objects, allocator
        device_cleanup(*mesh)
    host, dev = [], []
    for _ in range(reps):
        (hv, hf, hn, n_parts), t = _wall(lambda: host_cleanup(*mesh))
        host.append(round(t, 1))
        (dv, df, dn), t = _wall(lambda: device_cleanup(*mesh))
        dev.append(round(t, 2))
    equal = bool(np.array_equal(hv, dv.astype(np.float64)) and np.array_equal(hf, df.astype(np.int64))
                 and np.array_equal(hn, dn.astype(np.float64)))
    out = {"mesh": name, "faces": int(mesh[1].shape[0]), "verts": int(mesh[0].shape[0]), "components": n_parts,
           "kept_faces": int(len(hf)), "host_ms": host, "device_ms": dev, "host_best_ms": min(host),
           "device_best_ms": min(dev), "equal": equal}
    out.update(device_steps(*mesh))
    print(f"{name}: F {out['faces']}, V {out['verts']}, {n_parts} components; host split + argmax {min(host):.0f} ms "
          f"{host}, device {min(dev):.2f} ms {dev} (labels {out['labels_ms']}, areas {out['areas_ms']}, select "
          f"{out['select_ms']}); equal {equal}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--noise", type=int, default=64, help="lattice size of the many-component noise mesh (0: skip)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_components_time.py: no GPU - nothing is measured")
    import bench
    runs = []
    if args.noise:
        runs.append(time_mesh(f"noise_{args.noise}", noise_mesh(args.noise), args.reps))
    if args.res:
        net = bench._build("C2", "cuda", 0.0).implicit_network
        for res in args.res:
            runs.append(time_mesh(f"C2_sparse_{res}", fine_mesh(net, res), args.reps))
            torch.cuda.empty_cache()
    line = json.dumps({"runs": runs})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
