"""Time of the DTU Chamfer evaluation of a mesh against a point cloud on the GPU (evaluation.chamfer.mesh_chamfer:
csrc/hm_mesh_sample.hip, csrc/hm_nn.hip) and on the host as before (download, numpy upsampling, scipy cKDTree).

    python scripts/chamfer_time.py [--res 512] [--target 2000000] [--cloud 10000000] [--reps 2] [--out FILE]

No data files.  The mesh is ops.marching_cubes of an analytic bumpy-sphere volume at --res; the target cloud is
seeded: --target vertices of that mesh moved by normal noise of two lattice spacings; the density is chosen from the
mesh's area so that the sampled cloud has about --cloud points; max_dist is four lattice spacings.  After a warm-up of
the device path, --reps times alternately, as wall clock from a synchronised device to the scalars in host memory:
  (a) device: mesh_chamfer(mesh, target, density, max_dist)
  (b) host: download of vertices and faces, the upsampling rule vectorised in numpy, cKDTree(...).query(...,
      workers=16) both ways, the means below max_dist
The two metrics are printed side by side; the means must agree to 1e-6 relative and the counts must be equal up to the
number of distances within 1e-6 relative of max_dist (the bound of tests/test_chamfer_gpu.py, which picks a max_dist
with no such distance), else the script fails.  One more device call reports the steps between synchronisations
and the hm_nn_query launches' candidate tests per second.  No GPU: exits with an error instead of printing a number.
Prints a line per measurement, then one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def bumpy_sphere(res):
    """(volume [res]^3 fp32 on the GPU, spacing): |x| - 0.6 - 0.04 sin(7x) sin(6y) sin(5z) on [-1, 1]^3"""
    import torch
    ax = torch.linspace(-1.0, 1.0, res, device="cuda")
    x, y, z = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    vol = torch.sqrt(x * x + y * y + z * z) - 0.6 - 0.04 * torch.sin(7 * x) * torch.sin(6 * y) * torch.sin(5 * z)
    return vol.contiguous(), (2.0 / (res - 1),) * 3


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def host_sample(verts, faces, density):
    """the upsampling rule of include/hashmod.h over all faces at once: every face's (n1+1) x (n2+1) lattice is listed
    (face, i, j) and filtered by u + v < 1"""
    import numpy as np
    v = verts.astype(np.float64)[faces]
    a, v1, v2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]

    def norm(w):
        return np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])

    l1, l2 = norm(v1), norm(v2)
    A2 = norm(np.stack([v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1], v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2],
                        v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]], 1))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        thr = density * np.sqrt(l1 * l2 / A2)
        n1, n2 = np.floor(l1 / thr), np.floor(l2 / thr)
    ok = np.nonzero((A2 > 0) & (n1 >= 1) & (n2 >= 1))[0]
    n1, n2 = n1[ok], n2[ok]
    per = ((n1 + 1) * (n2 + 1)).astype(np.int64)
    start = np.cumsum(per) - per
    which = np.repeat(np.arange(len(ok)), per)
    k = np.arange(int(per.sum())) - start[which]
    w2 = (n2[which] + 1).astype(np.int64)
    u = (k // w2 + 0.5) / n1[which]
    w = (k % w2 + 0.5) / n2[which]
    keep = u + w < 1.0
    f = ok[which[keep]]
    u, w = u[keep][:, None], w[keep][:, None]
    return ((v1[f] * u + v2[f] * w) + a[f]).astype(np.float32)


def host_chamfer(verts, faces, target, density, max_dist):
    import numpy as np
    from scipy.spatial import cKDTree
    v, f, t = verts.cpu().numpy(), faces.cpu().numpy(), target.cpu().numpy()
    cloud = np.concatenate([v, host_sample(v, f, density)]).astype(np.float64)
    t = t.astype(np.float64)
    d_ab = cKDTree(t).query(cloud, workers=16)[0]
    d_ba = cKDTree(cloud).query(t, workers=16)[0]
    ka, kb = d_ab < max_dist, d_ba < max_dist
    ma, mb = float(d_ab[ka].mean()), float(d_ba[kb].mean())
    # distances so close to the cut-off that fp32 rounding of d2 may move them across it
    edge = [int((np.abs(d / max_dist - 1.0) <= 1e-6).sum()) for d in (d_ab, d_ba)]
    return {"mean_a2b": ma, "mean_b2a": mb, "overall": 0.5 * (ma + mb), "n_a2b": int(ka.sum()), "n_b2a": int(kb.sum()),
            "n_cloud": len(cloud), "at_cutoff_a2b": edge[0], "at_cutoff_b2a": edge[1]}


def device_steps(verts, faces, target, density, max_dist):
    """the device path's steps between synchronisations, and the query launches' candidate tests"""
    import math
    import numpy as np
    import torch
    from hashmodnffbanks_idr_amd import ops
    samples, t_sample = _wall(lambda: ops.mesh_sample_surface(verts, faces, density))
    cloud = torch.cat([verts, samples])
    md2 = float(np.float32(max_dist * max_dist * 1.001))
    out = {"sample_ms": round(t_sample, 2)}
    for name, src, dst in (("a2b", cloud, target), ("b2a", target, cloud)):
        index, t_build = _wall(lambda: ops.NNIndex(dst))
        stats = {}
        _, t_query = _wall(lambda: index._query(src, md2, stats))
        tests = stats["candidate_tests"]
        out.update({f"build_{name}_ms": round(t_build, 2), f"query_{name}_ms": round(t_query, 2),
                    f"tests_{name}": tests, f"tests_per_query_{name}": round(tests / src.shape[0], 1),
                    f"gtests_per_s_{name}": round(tests / t_query / 1e6, 1), f"grid_{name}": index.g,
                    f"cell_{name}": index.h})
        assert math.isfinite(t_query)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--target", type=int, default=2000000)
    ap.add_argument("--cloud", type=int, default=10000000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("chamfer_time.py: no GPU - nothing is measured")
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd.evaluation import mesh_chamfer

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
    print(f"mesh: V {verts.shape[0]}, F {faces.shape[0]}, area {area:.4f}; density {density:.6f}, max_dist "
          f"{max_dist:.6f}, target {args.target}", flush=True)

    mesh_chamfer((verts, faces), target, density, max_dist)         # warm-up: code objects, allocator, workspaces
    dev_ms, host_ms = [], []
    for _ in range(args.reps):
        dev, t = _wall(lambda: mesh_chamfer((verts, faces), target, density, max_dist))
        dev_ms.append(round(t, 1))
        print(f"device: {t:.1f} ms  {dev}", flush=True)
        host, t = _wall(lambda: host_chamfer(verts, faces, target, density, max_dist))
        host_ms.append(round(t, 0))
        print(f"host:   {t:.0f} ms  {host}", flush=True)
    steps = device_steps(verts, faces, target, density, max_dist)
    print("device steps:", steps, flush=True)
    agree = bool(all(abs(getattr(dev, k) - host[k]) <= 1e-6 * abs(host[k]) for k in ("mean_a2b", "mean_b2a", "overall"))
                 and all(abs(getattr(dev, "n_" + k) - host["n_" + k]) <= host["at_cutoff_" + k] for k in ("a2b", "b2a"))
                 and dev.n_cloud == host["n_cloud"])
    out = {"res": args.res, "verts": int(verts.shape[0]), "faces": int(faces.shape[0]), "target": args.target,
           "cloud": dev.n_cloud, "density": density, "max_dist": max_dist, "device_ms": dev_ms, "host_ms": host_ms,
           "device_best_ms": min(dev_ms), "host_best_ms": min(host_ms), "device": dict(zip(dev._fields, dev)),
           "host": host, "agree": agree}
    out.update(steps)
    line = json.dumps({"chamfer": out})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not agree:
        raise SystemExit("chamfer_time.py: the device and host metrics differ beyond 1e-6 relative")


if __name__ == "__main__":
    main()
