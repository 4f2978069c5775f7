"""Time of the whole DTU evaluation of a mesh against a scan on the GPU (evaluation.chamfer.dtu_chamfer:
csrc/hm_mesh_sample.hip, csrc/hm_nn.hip, csrc/hm_nn_radius.hip, csrc/hm_dtu_filter.hip) and on the host as the
reference does it (download, numpy upsampling, sklearn radius_neighbors and the greedy loop, numpy filters, cKDTree).

    python scripts/dtu_eval_time.py [--res 512] [--target 2000000] [--cloud 10000000] [--reps 1] [--out FILE]

No data files.  Mesh, target cloud, density and max_dist are those of scripts/chamfer_time.py; the thinning radius is
the density, as in the reference.  The scan's data are synthetic: a bounding box that leaves the +x side of the mesh
out of bounds, an observation mask (voxels of 0.01) that is unset for y >= 0.3 from the centre, and a ground plane that
cuts the mesh 0.45 below its centre.  Both legs are given the same seeded shuffle (a device randperm, downloaded for the host).
After a warm-up of the device path, --reps times alternately, as wall clock from a synchronised device to the scalars
in host memory:
  (a) device: dtu_chamfer(mesh, target, ..., order=order)
  (b) host: download of vertices and faces, the upsampling rule in numpy, the shuffle, NearestNeighbors(radius,
      kd_tree, n_jobs=16).radius_neighbors and the reference's Python loop, the box, mask and plane filters in numpy,
      cKDTree(...).query(..., workers=16) both ways, the means below max_dist - as the sum of its stages' times
The host decides neighbourhood in fp64 and the device with the library's fp32 d2, so a pair within rounding of the
radius may be decided differently, and that changes the thinned cloud around it; the script counts the host's pairs
within 1e-6 relative of the radius and demands equal counts only when there is none (the tests compare bit for bit
against an fp32-exact reference).  The means must agree to 1e-4 relative in any case, else the script fails.  One
more device run reports the time of every stage and the number of thinning rounds.  No GPU: exits with an error
instead of printing a number.  Prints a line per measurement, then one JSON line.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if path not in sys.path:
        sys.path.insert(0, path)

from chamfer_time import _wall, bumpy_sphere, host_sample  # noqa: E402

COUNTS = ("n_cloud", "n_down", "n_in", "n_in_obs", "n_stl_above", "n_d2s", "n_s2d")


def synthetic_scan(centre):
    """(obs_mask uint8 numpy, bb, res, patch, plane) around the bumpy sphere of radius ~0.6 at `centre`"""
    import numpy as np
    centre = np.asarray(centre, np.float64)
    bb = centre + np.array([[-0.7, -0.7, -0.7], [0.3, 0.7, 0.7]])
    res, patch = 0.01, 0.1
    shape = tuple(int(round((bb[1][a] - bb[0][a]) / res)) + 1 for a in range(3))
    y = bb[0][1] + res * np.arange(shape[1])
    mask = np.zeros(shape, np.uint8)
    mask[:, y < centre[1] + 0.3, :] = 1
    return mask, bb, res, patch, np.array([0.0, 0.0, 1.0, 0.45 - centre[2]])


def host_dtu(verts, faces, target, order, scan, density, max_dist):
    import numpy as np
    from scipy.spatial import cKDTree
    from sklearn.neighbors import NearestNeighbors
    mask, bb, res, patch, plane = scan
    ms = {}
    t0 = time.perf_counter()

    def lap(name):
        nonlocal t0
        t1 = time.perf_counter()
        ms[name] = round((t1 - t0) * 1e3, 1)
        print(f"  host {name}: {ms[name]:.0f} ms", flush=True)
        t0 = t1

    v, f, stl = verts.cpu().numpy(), faces.cpu().numpy(), target.cpu().numpy()
    data = np.concatenate([v, host_sample(v, f, density)])[order.cpu().numpy()].astype(np.float64)
    lap("download_sample_shuffle")
    nn = NearestNeighbors(n_neighbors=1, radius=density, algorithm="kd_tree", n_jobs=16)
    nn.fit(data)
    dist, nb = nn.radius_neighbors(data, radius=density, return_distance=True)
    lap("radius_neighbors")
    keep = np.ones(len(data), dtype=np.bool_)
    for curr, idxs in enumerate(nb):
        if keep[curr]:
            keep[idxs] = 0
            keep[curr] = 1
    lap("greedy_loop")
    at_radius = int(sum(int((np.abs(d / density - 1.0) <= 1e-6).sum()) for d in dist))
    del dist, nb
    t0 = time.perf_counter()                                          # the census above is not part of the evaluation
    down = data[keep]
    inbound = ((down >= bb[0] - patch) & (down < bb[1] + patch * 2)).all(1)
    data_in = down[inbound]
    grid = np.around((data_in - bb[0]) / res).astype(np.int32)
    inside = ((grid >= 0) & (grid < np.asarray(mask.shape))).all(1)
    in_obs = np.zeros(len(data_in), np.bool_)
    g = grid[inside]
    in_obs[inside] = mask[g[:, 0], g[:, 1], g[:, 2]] != 0
    stl = stl.astype(np.float64)
    above = ((plane[0] * stl[:, 0] + plane[1] * stl[:, 1]) + plane[2] * stl[:, 2]) + plane[3] > 0
    lap("filters")
    d2s = cKDTree(stl).query(data_in[in_obs], workers=16)[0]
    s2d = cKDTree(data_in).query(stl[above], workers=16)[0]
    ka, kb = d2s < max_dist, s2d < max_dist
    acc, comp = float(d2s[ka].mean()), float(s2d[kb].mean())
    lap("nearest_neighbours")
    return {"accuracy": acc, "completeness": comp, "overall": 0.5 * (acc + comp), "n_cloud": len(data),
            "n_down": len(down), "n_in": len(data_in), "n_in_obs": int(in_obs.sum()), "n_stl_above": int(above.sum()),
            "n_d2s": int(ka.sum()), "n_s2d": int(kb.sum()), "pairs_at_radius": at_radius, "stage_ms": ms,
            "total_ms": round(sum(ms.values()), 1)}


def device_stages(verts, faces, target, order, scan_dev, density, max_dist):
    """dtu_chamfer's steps one by one, each to a synchronised device, and the thinning's rounds"""
    import torch
    from hashmodnffbanks_idr_amd import ops
    mask, bb, res, patch, plane = scan_dev
    out = {}

    def stage(name, fn):
        r, t = _wall(fn)
        out[name + "_ms"] = round(t, 2)
        return r

    cloud = stage("sample", lambda: torch.cat([verts, ops.mesh_sample_surface(verts, faces, density)]))
    data = stage("shuffle", lambda: cloud[order])
    stats = {}
    keep = stage("thin", lambda: ops.radius_downsample(data, density, stats=stats))
    out["rounds"] = stats["rounds"]
    stage("thin_grid_only", lambda: ops.NNIndex(data))
    down = stage("compact", lambda: data[keep])

    def filters():
        fl = ops.dtu_point_flags(down, mask, bb, res, patch, plane)
        above = (ops.dtu_point_flags(target, mask, bb, res, patch, plane) & ops.DTU_ABOVE_PLANE) != 0
        return down[(fl & 1) != 0], down[(fl & 3) == 3], target[above]

    data_in, in_obs, stl_above = stage("filters", filters)
    stage("accuracy_nn", lambda: ops.one_sided_distance(in_obs, target, max_dist))
    stage("completeness_nn", lambda: ops.one_sided_distance(stl_above, data_in, max_dist))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--target", type=int, default=2000000)
    ap.add_argument("--cloud", type=int, default=10000000)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dtu_eval_time.py: no GPU - nothing is measured")
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd.evaluation import dtu_chamfer

    vol, spacing = bumpy_sphere(args.res)
    verts, faces, _ = ops.marching_cubes(vol, 0.0, spacing)
    del vol
    torch.cuda.empty_cache()
    area = float(ops.mesh_surface_moments(verts, faces)[0])
    density = (area / args.cloud) ** 0.5
    max_dist = 4.0 * spacing[0]
    gen = torch.Generator().manual_seed(0)
    pick = torch.randint(0, verts.shape[0], (args.target,), generator=gen).cuda()
    noise = torch.randn((args.target, 3), generator=gen).cuda() * (2.0 * spacing[0])
    target = (verts[pick] + noise).contiguous()
    lo, hi = torch.aminmax(verts, dim=0)
    scan = synthetic_scan(((lo + hi) / 2).tolist())
    scan_dev = (torch.from_numpy(scan[0]).cuda(),) + scan[1:]
    n_cloud = int(verts.shape[0] + ops.mesh_sample_surface(verts, faces, density).shape[0])
    dgen = torch.Generator(device="cuda")
    dgen.manual_seed(1)
    order = torch.randperm(n_cloud, generator=dgen, device="cuda")
    print(f"mesh: V {verts.shape[0]}, F {faces.shape[0]}, area {area:.4f}; cloud {n_cloud}, density = radius "
          f"{density:.6f}, max_dist {max_dist:.6f}, target {args.target}, mask {scan[0].shape}", flush=True)

    def device():
        return dtu_chamfer((verts, faces), target, obs_mask=scan_dev[0], bb=scan[1], res=scan[2], plane=scan[4],
                           density=density, patch=scan[3], max_dist=max_dist, order=order)

    device()                                                         # warm-up: code objects, allocator, workspaces
    dev_ms, host_ms = [], []
    for _ in range(args.reps):
        dev, t = _wall(device)
        dev_ms.append(round(t, 1))
        print(f"device: {t:.1f} ms  {dev}", flush=True)
        host = host_dtu(verts, faces, target, order, scan, density, max_dist)
        host_ms.append(host["total_ms"])
        print(f"host:   {host['total_ms']:.0f} ms  {host}", flush=True)
    stages = device_stages(verts, faces, target, order, scan_dev, density, max_dist)
    print("device stages:", stages, flush=True)
    means = all(abs(getattr(dev, k) - host[k]) <= 1e-4 * abs(host[k]) or (math.isnan(host[k]) and math.isnan(getattr(dev, k)))
                for k in ("accuracy", "completeness", "overall"))
    counts = all(getattr(dev, k) == host[k] for k in COUNTS)
    agree = bool(means and (counts or host["pairs_at_radius"] > 0) and dev.n_cloud == host["n_cloud"])
    out = {"res": args.res, "verts": int(verts.shape[0]), "faces": int(faces.shape[0]), "target": args.target,
           "cloud": n_cloud, "density": density, "max_dist": max_dist, "device_ms": dev_ms, "host_ms": host_ms,
           "device_best_ms": min(dev_ms), "host_best_ms": min(host_ms), "device": dev._asdict(), "host": host,
           "counts_equal": counts, "agree": agree}
    out.update(stages)
    line = json.dumps({"dtu_eval": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not agree:
        raise SystemExit("dtu_eval_time.py: the device and host results differ")


if __name__ == "__main__":
    main()
