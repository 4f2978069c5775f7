"""Guard statistics of the fixed leg's workload (bench.py: C2, 2048 rays, lr 0, sampler_head 0, captured step): the
tracer's guard_refined, guard_max_dev and guard_tripped after each of N steps, as one JSON line.  Two builds of the same
ABI (HM_LIB_PATH) that mark the same samples print the same line.

    python scripts/guard_steps.py [N=25]
"""
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)

if __name__ == "__main__":
    import torch
    import bench
    from hashmodnffbanks_idr_amd.model.loss import IDRLoss
    from hashmodnffbanks_idr_amd.training.graph_step import GraphedTrainStep
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 25
    dev = torch.device("cuda", 0)
    model = bench._build("C2", dev, 0.0)
    model.ray_tracer.sampler_head = 0
    inp, gt = bench.synthetic_batch(1234, bench.RAYS_PER_GPU, dev)
    torch.manual_seed(100)
    opt = ClipAdam(model.parameters(), lr=0.0, max_norm=1.0)
    stepper = GraphedTrainStep(model, IDRLoss(eikonal_weight=0.1, mask_weight=100.0, alpha=50.0), opt, None, warmup=2)
    rec = {"guard_refined": [], "guard_max_dev": [], "guard_tripped": False, "sdf_evals": []}
    for _ in range(n):
        stepper.step(inp, gt)
        torch.cuda.synchronize()
        st = model.ray_tracer.last_stats
        rec["guard_refined"].append(int(st["guard_refined"]))
        rec["guard_max_dev"].append(float(st["guard_max_dev"]))
        rec["guard_tripped"] = rec["guard_tripped"] or bool(st["guard_tripped"])
        rec["sdf_evals"].append(int(st.get("sdf_evals", 0)))
    print("GUARD " + json.dumps(rec))
