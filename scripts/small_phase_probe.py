"""Phase stamps of ONE tile of the small-tile SDF body (probe build: scripts/sdf_phase_probe.py --build; run with
HM_LIB_PATH=scripts/libhashmod_probe.so): where does the time of a small launch go that is neither matrix pipe nor weight
stream?  Workgroup 0 / thread 0 stamps the encode and, per layer, [k-loop done, k quarters added, after layer 0's barrier,
epilogue done, after the layer's barrier].

    HM_LIB_PATH=scripts/libhashmod_probe.so python scripts/small_phase_probe.py [--tile 4|8|16] [--points N]
                                                                                [--json FILE --label NAME]

Defaults: the 4-point tile on 256 points.  The headline's march rounds are --tile 16 --points 4096 (one tile per CU).
--json: the per-phase microseconds are added to FILE under NAME (profiles/small16_phase.json: parent first, then branch)."""
import argparse
import ctypes as C, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, R + "/tests", R + "/tests/golden"]
ap = argparse.ArgumentParser()
ap.add_argument("--tile", type=int, default=4, choices=(4, 8, 16))
ap.add_argument("--points", type=int, default=256)
ap.add_argument("--json")
ap.add_argument("--label", default="build")
args = ap.parse_args()
import numpy as np, torch, bench
from hashmodnffbanks_idr_amd import _lib
model = bench._build("C2", torch.device("cuda", 0), 0.0)
net = model.implicit_network
g = torch.Generator(device="cpu").manual_seed(1)
x = (torch.rand((args.points, 3), generator=g) * 2 - 1).cuda()
net.sdf_tile_points = args.tile
fn = _lib.lib().hm_probe_read
fn.restype = C.c_int
fn.argtypes = [C.c_void_p, C.c_int]
M = 100.0   # wall_clock64(): 100 MHz
runs = []
for _ in range(3):
    net.sdf(x)
torch.cuda.synchronize()
for _ in range(9):
    net.sdf(x)
    torch.cuda.synchronize()
    ts = (C.c_ulonglong * 128)()
    assert fn(ts, 128) == 0
    t = np.asarray(list(ts), dtype=np.int64)
    ph = {"encode": (t[1] - t[0]) / M, "layers": []}
    prev = t[1]
    n_mfma = int(np.count_nonzero(t[40:56]))      # layers that stamped their epilogue: all but the sdf-only last one
    for li in range(n_mfma):
        a, b, c, e, d = t[2 + 4 * li], t[3 + 4 * li], t[4 + 4 * li], t[40 + li], t[5 + 4 * li]
        ph["layers"].append({"k_loop": (a - prev) / M, "quarter_sums": (b - a) / M, "barrier0": (c - b) / M,
                             "epilogue": (e - c) / M, "barrier": (d - e) / M})
        prev = d
    ph["last_layer"] = (t[100] - prev) / M
    ph["tile"] = (t[100] - t[0]) / M
    runs.append(ph)
runs.sort(key=lambda p: p["tile"])
ph = runs[len(runs) // 2]     # the run with the median tile time
print("tile %d, %d points (median of %d launches by tile time; tile times %.2f .. %.2f us)" %
      (args.tile, args.points, len(runs), runs[0]["tile"], runs[-1]["tile"]))
print("tile start -> encode done: %.2f us" % ph["encode"])
for li, l in enumerate(ph["layers"]):
    print("layer %d: k-loop %.2f  quarter sums %.2f  barrier %.2f  epilogue %.2f  barrier %.2f" %
          (li, l["k_loop"], l["quarter_sums"], l["barrier0"], l["epilogue"], l["barrier"]))
sums = {k: sum(l[k] for l in ph["layers"]) for k in ("k_loop", "quarter_sums", "barrier0", "epilogue", "barrier")}
print("sums: k-loops %.2f  quarter sums %.2f  layer-0 barrier %.2f  epilogues %.2f  barriers %.2f" %
      (sums["k_loop"], sums["quarter_sums"], sums["barrier0"], sums["epilogue"], sums["barrier"]))
print("last layer + output: %.2f us;  whole tile %.2f us" % (ph["last_layer"], ph["tile"]))
if args.json:
    doc = json.load(open(args.json)) if os.path.exists(args.json) else {}
    ph["sums"] = sums
    ph["tile_times_us"] = [r["tile"] for r in runs]
    doc.setdefault(args.label, {})["tile%d_n%d" % (args.tile, args.points)] = ph
    json.dump(doc, open(args.json, "w"), indent=1)
