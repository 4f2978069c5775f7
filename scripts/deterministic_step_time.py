"""ms/step of the C2 headline step (2048 rays, fp32, captured graph; bench._build / bench.synthetic_batch) with the
deterministic mode off and on.

    python scripts/deterministic_step_time.py [--pairs 3] [--steps 50] [--warmup 5] [--timeout 600]

Every measurement is a fresh child process (`--child off|on`) under its own `timeout`; the parent alternates the two
modes and stops at the first child that fails.  Prints ms/step per mode (mean of the runs, min-max spread) and the
on/off ratio, then one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(mode, steps, warmup):
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
        sys.path.insert(0, p)
    import torch
    import bench
    from hashmodnffbanks_idr_amd.model.loss import IDRLoss
    from hashmodnffbanks_idr_amd.training.graph_step import GraphedTrainStep
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    model = bench._build(bench.CFG, "cuda", 0.0)
    inp, gt = bench.synthetic_batch(1234, bench.RAYS_PER_GPU, "cuda")
    loss_fn = IDRLoss(eikonal_weight=0.1, mask_weight=100.0, alpha=50.0)
    stepper = GraphedTrainStep(model, loss_fn, ClipAdam(model.parameters(), lr=0.0, max_norm=1.0), warmup=2,
                               deterministic=(mode == "on"))
    torch.manual_seed(100)
    for _ in range(max(warmup, 3)):          # the capture happens in here
        stepper.step(inp, gt)
    assert stepper.g_fb is not None, "graph capture fell back to eager"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        stepper.step(inp, gt)
    torch.cuda.synchronize()
    print(json.dumps({"mode": mode, "ms_per_step": (time.perf_counter() - t0) / steps * 1e3}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child process")
    ap.add_argument("--child", choices=("off", "on"))
    a = ap.parse_args()
    if a.child:
        child(a.child, a.steps, a.warmup)
        return
    res = {"off": [], "on": []}
    for _ in range(a.pairs):
        for mode in ("off", "on"):
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", mode,
                   "--steps", str(a.steps), "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
                sys.exit(f"child '{mode}' failed with exit status {p.returncode}; stopping")
            res[mode].append(json.loads(p.stdout.strip().splitlines()[-1])["ms_per_step"])
    summary = {}
    for mode, v in res.items():
        summary[mode] = {"ms_per_step": round(sum(v) / len(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                         "runs": [round(x, 3) for x in v]}
        print(f"deterministic {mode:3s}: {summary[mode]['ms_per_step']:.3f} ms/step  "
              f"(runs {summary[mode]['min']:.3f} - {summary[mode]['max']:.3f})")
    summary["ratio_on_off"] = round(summary["on"]["ms_per_step"] / summary["off"]["ms_per_step"], 4)
    print(f"on / off: {summary['ratio_on_off']:.4f}")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
