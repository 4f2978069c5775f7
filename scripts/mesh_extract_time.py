"""Time of mesh extraction on the GPU (csrc/hm_mesh.hip, utils/plots.get_surface_high_res_mesh).

    python scripts/mesh_extract_time.py [--sizes 256 512] [--iters 10] [--warmup 3] [--res 512] [--reps 2]
                                        [--sparse-res 1024] [--out FILE]

1. ops.marching_cubes on a sphere SDF volume (radius 0.6 in [-1,1]^3) at each size: ms per call from device events
   after warm-up (the call includes its one host read of the counts), and the kernels' bytes moved over that time
   against the 6.29 TB/s achievable HBM rate (MI355X float4 copy).  Bytes counted per lattice point: volume read by
   the classify pass (4) + code write (2), code read + vertex-base write by the vertex pass (2 + 4), code read by the
   face pass (2); per vertex 24 B of output + 2 x 7 volume reads (gradients); per face 12 B + 3 x 6 B of lookups.
2. get_surface_high_res_mesh(resolution=--res) on the C2 network of bench.py (geometric init, seed 0), split into
   SDF evaluation and marching cubes (device events around every call) and the rest (host work: components, moments,
   eigh, copies; wall clock minus the two).
3. the same call with sparse=True (ops.marching_cubes_sparse, csrc/hm_mesh_sparse.hip) beside it: after a warm-up of
   both, --reps dense and sparse calls alternate in this process, every one split as in 2.; for a sparse call
   "marching cubes" is everything of ops.marching_cubes_sparse except its SDF calls (brick bookkeeping, status, count,
   emit, sort, and the device idling over the per-round host reads).  Also the share of the aligned lattice handed
   to the SDF, the rounds and the SDF calls; the SDF time to expect is that share of the dense SDF time.  Then one
   sparse call at --sparse-res (0: skip), a lattice the dense path cannot hold.
No GPU: exits with an error instead of printing a number.  Prints a table, then one JSON line.
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

HBM_TBS = 6.29


def mc_bytes(n_points, n_verts, n_faces):
    return n_points * (4 + 2 + 2 + 4 + 2) + n_verts * (24 + 2 * 7 * 4) + n_faces * (12 + 3 * 6)


def sphere_volume(n, device):
    import torch
    x = torch.linspace(-1.0, 1.0, n, device=device)
    return (torch.sqrt(x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2) - 0.6).contiguous()


def time_mc(n, iters, warmup):
    import torch
    from hashmodnffbanks_idr_amd import ops
    vol = sphere_volume(n, "cuda")
    d = 2.0 / (n - 1)
    for _ in range(warmup):
        out = ops.marching_cubes(vol, 0.0, (d, d, d))
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        out = ops.marching_cubes(vol, 0.0, (d, d, d))
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / iters
    nv, nf = out[0].shape[0], out[1].shape[0]
    gb = mc_bytes(n ** 3, nv, nf) / 1e9
    return {"size": n, "ms": round(ms, 4), "verts": nv, "faces": nf, "gbytes": round(gb, 3),
            "tb_s": round(gb / ms, 3), "hbm_share": round(gb / ms / HBM_TBS, 3)}


class _Timed:
    """wraps a callable: device-event time of every call, summed"""

    def __init__(self, fn):
        self.fn, self.pairs = fn, []

    def __call__(self, *a, **k):
        import torch
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = self.fn(*a, **k)
        e.record()
        self.pairs.append((s, e))
        return out

    def ms(self):
        return sum(s.elapsed_time(e) for s, e in self.pairs)


class _TimedSparse(_Timed):
    """ops.marching_cubes_sparse, timed, keeping the stats of the last call"""

    def __call__(self, *a, **k):
        out = super().__call__(*a, return_stats=True, **k)
        self.stats = out[3]
        return out[:3]


def time_high_res(net, res, sparse):
    """one get_surface_high_res_mesh(res) call split into SDF, marching cubes and host time"""
    import torch
    from hashmodnffbanks_idr_amd import ops
    from hashmodnffbanks_idr_amd.utils import plots
    sdf = _Timed(net.sdf)
    mc = _Timed(ops.marching_cubes)
    mcs = _TimedSparse(ops.marching_cubes_sparse)
    orig = ops.marching_cubes, ops.marching_cubes_sparse
    ops.marching_cubes, ops.marching_cubes_sparse = mc, mcs
    try:
        t0 = time.perf_counter()
        mesh = plots.get_surface_high_res_mesh(sdf, res, sparse=sparse)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
    finally:
        ops.marching_cubes, ops.marching_cubes_sparse = orig
    if mesh is None:
        raise SystemExit("get_surface_high_res_mesh found no surface")
    # a sparse call's SDF calls lie inside ops.marching_cubes_sparse: what is left of it counts as marching cubes
    inner = sum(s.elapsed_time(e) for s, e in sdf.pairs[-mcs.stats["sdf_calls"]:]) if sparse else 0.0
    mc_ms = mc.ms() + (mcs.ms() - inner if sparse else 0.0)
    out = {"res": res, "sparse": sparse, "wall_ms": round(wall, 1), "sdf_ms": round(sdf.ms(), 1),
           "mc_ms": round(mc_ms, 2), "host_ms": round(wall - sdf.ms() - mc_ms, 1), "sdf_calls": len(sdf.pairs),
           "verts": len(mesh.vertices), "faces": len(mesh.faces)}
    if sparse:
        st = mcs.stats
        out.update(share=round(st["points"] / st["lattice_points"], 4), rounds=st["rounds"],
                   lattice_points=st["lattice_points"], bricks=st["bricks_evaluated"],
                   surface_bricks=st["surface_bricks"], fine_sdf_ms=round(inner, 1))
    return out


def _show(h):
    tail = (f"; {100 * h['share']:.1f}% of {h['lattice_points']} lattice points evaluated in {h['rounds']} rounds"
            if h["sparse"] else "")
    print(f"get_surface_high_res_mesh({h['res']}{', sparse' if h['sparse'] else ''}) C2: {h['wall_ms']:.0f} ms = SDF "
          f"{h['sdf_ms']:.0f} ms ({h['sdf_calls']} calls) + marching cubes {h['mc_ms']:.2f} ms + host "
          f"{h['host_ms']:.0f} ms; {h['verts']} verts, {h['faces']} faces{tail}", flush=True)


def time_high_res_legs(res, reps, sparse_res):
    import torch
    import bench
    from hashmodnffbanks_idr_amd.utils import plots
    net = bench._build("C2", "cuda", 0.0).implicit_network
    for sparse in (False, True):                      # warm-up: code objects, packed weights, allocator
        plots.get_surface_high_res_mesh(net.sdf, 64, sparse=sparse)
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        for sparse in (False, True):
            runs.append(time_high_res(net, res, sparse))
            _show(runs[-1])
    out = {"runs": runs}
    dense, sp = ([r for r in runs if r["sparse"] == s] for s in (False, True))
    best = lambda rs, key: min(r[key] for r in rs)
    out["summary"] = {"res": res, "dense_wall_ms": best(dense, "wall_ms"), "sparse_wall_ms": best(sp, "wall_ms"),
                      "dense_sdf_ms": best(dense, "sdf_ms"), "sparse_sdf_ms": best(sp, "sdf_ms"),
                      "share": sp[0]["share"], "sdf_ratio": round(best(sp, "sdf_ms") / best(dense, "sdf_ms"), 4),
                      "wall_ratio": round(best(sp, "wall_ms") / best(dense, "wall_ms"), 4)}
    m = out["summary"]
    print(f"sparse / dense at {res}: wall {m['wall_ratio']:.3f}, SDF {m['sdf_ratio']:.3f} (evaluated share "
          f"{m['share']:.3f})", flush=True)
    if sparse_res:
        out["sparse_large"] = time_high_res(net, sparse_res, True)
        _show(out["sparse_large"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--res", type=int, default=512, help="get_surface_high_res_mesh resolution (0: skip)")
    ap.add_argument("--reps", type=int, default=2, help="dense / sparse pairs at --res")
    ap.add_argument("--sparse-res", type=int, default=1024, help="one more sparse call at this resolution (0: skip)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_extract_time.py: no GPU - nothing is measured")
    result = {"mc": [time_mc(n, args.iters, args.warmup) for n in args.sizes]}
    for r in result["mc"]:
        print(f"marching_cubes {r['size']}^3: {r['ms']:.3f} ms/call, {r['verts']} verts, {r['faces']} faces, "
              f"{r['gbytes']:.2f} GB -> {r['tb_s']:.2f} TB/s ({100 * r['hbm_share']:.0f}% of {HBM_TBS} TB/s)",
              flush=True)
    if args.res:
        result["high_res"] = time_high_res_legs(args.res, args.reps, args.sparse_res)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
