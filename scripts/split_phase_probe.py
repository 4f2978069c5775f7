"""Phase timing of ONE 64-point tile of the split-operand SDF kernel (csrc/hm_sdf_split_tile.h inside
sdf_fwd_split_kernel): 100 MHz stamps taken by workgroup 0 / thread 0 on its second tile after the point load, after the
encode, per layer at [end of its own k-loop, after the first barrier, end of its own epilogue, after the second barrier]
and at the end of the last layer.  Needs a probe build of the library:

    python scripts/split_phase_probe.py --build    (compiles csrc/*.hip, hm_sdf_split.hip with -DHM_SPLIT_PHASE_PROBE, into
                                                    scripts/libhashmod_split_probe.so; no GPU needed)
    HM_LIB_PATH=scripts/libhashmod_split_probe.so python scripts/split_phase_probe.py [--split bf16x2] [--json FILE]
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, R + "/tests", R + "/tests/golden"]
PROBE = os.path.join(R, "scripts", "libhashmod_split_probe.so")

if "--build" in sys.argv:
    from hashmodnffbanks_idr_amd import build as B
    tmp = tempfile.mkdtemp(prefix="split_probe_")
    procs, objs = [], []
    for src in B.SOURCES:
        obj = os.path.join(tmp, src.replace(".hip", ".o"))
        cmd = [B.HIPCC] + B.FLAGS + (["-DHM_SPLIT_PHASE_PROBE=1"] if src == "hm_sdf_split.hip" else []) + \
              ["-c", os.path.join(B.CSRC, src), "-o", obj]
        procs.append(subprocess.Popen(cmd))
        objs.append(obj)
    if any(p.wait() != 0 for p in procs):
        raise SystemExit("hipcc failed")
    subprocess.check_call([B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", PROBE] + objs)
    print(PROBE)
    sys.exit(0)

import numpy as np
import torch
import bench
from hashmodnffbanks_idr_amd import _lib, ops

kind = sys.argv[sys.argv.index("--split") + 1] if "--split" in sys.argv else "f16x2"
net = bench._build("C2", torch.device("cuda", 0), 0.0).implicit_network
g = torch.Generator(device="cpu").manual_seed(1)
x = (torch.rand((204800, 3), generator=g) * 2 - 1).cuda()     # 3200 tiles: 12.5 rounds of 256
net.coarse_split = kind
emb = net._hash_embedder()
pk = net.packed_weights()
for _ in range(3):
    ops.sdf_fwd_split(emb.desc, pk, x, emb.table.detach(), emb.freq_encoding.B)
torch.cuda.synchronize()
ts = (C.c_ulonglong * 128)()
fn = _lib.lib().hm_split_probe_read
fn.restype = C.c_int
fn.argtypes = [C.c_void_p, C.c_int]
assert fn(ts, 128) == 0
t = np.asarray(list(ts), dtype=np.int64)
MHZ = 100.0   # wall_clock64() = s_memrealtime: 100 MHz constant clock
n_hidden = pk.desc.n_layers - 1    # (the last layer is the VALU dot)
us = lambda a, b: round(float(t[b] - t[a]) / MHZ, 2)   # noqa: E731
rep = {"split": kind, "point_load": us(0, 1), "encode": us(1, 2), "layers": []}
prev = 2
for li in range(n_hidden):
    m, b1, e, b2 = (k + 4 * li for k in (3, 4, 5, 6))
    rep["layers"].append({"k_loop": us(prev, m), "barrier1": us(m, b1), "epilogue": us(b1, e), "barrier2": us(e, b2)})
    prev = b2
rep["last_layer"] = us(prev, 100)
rep["tile"] = us(0, 100)
rep["sums"] = {k: round(sum(l[k] for l in rep["layers"]), 2) for k in ("k_loop", "barrier1", "epilogue", "barrier2")}
rep["shader_clock_ghz"] = round(float(t[121] - t[120]) / (float(t[100] - t[0]) / MHZ) / 1e3, 3)
print("point load %.2f us, encode %.2f us" % (rep["point_load"], rep["encode"]))
for li, l in enumerate(rep["layers"]):
    print("layer %d: k-loop %.2f us  barrier %.2f  epilogue %.2f  barrier %.2f" %
          (li, l["k_loop"], l["barrier1"], l["epilogue"], l["barrier2"]))
print("last layer (VALU dot) + output: %.2f us;  whole tile %.2f us at %.3f GHz" %
      (rep["last_layer"], rep["tile"], rep["shader_clock_ghz"]))
print("sums: k-loops %(k_loop).1f  first barriers %(barrier1).1f  epilogues %(epilogue).1f  second barriers %(barrier2).1f (us)"
      % rep["sums"])
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
        json.dump(rep, f, indent=1)
