"""Phase timing of ONE tile of the pipelined GEMM (csrc/hm_gemm.hip, gemm_pipe2_body) on the six shapes of bench.py's
roofline_gemm: wall-clock stamps of workgroup 0 / thread 0 at entry, first operands in LDS, end of the K loop, after
the wave groups' exchange and after its last epilogue store has completed, and the time it spent in the K loop's
barriers.  Needs a probe build of the library:

    python scripts/gemm_phase_probe.py --build     (here: compiles csrc/*.hip, hm_gemm.hip with -DHM_GEMM_PHASE_PROBE,
                                                    into scripts/libhashmod_gemm_probe.so)
    HM_LIB_PATH=scripts/libhashmod_gemm_probe.so python scripts/gemm_phase_probe.py      (on the GPU box)

The two clock reads around every barrier of the probe build wait for the wave's outstanding LDS traffic, so its loop is
slower than the product's: read the barrier column as an upper bound.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R]
PROBE = os.path.join(R, "scripts", "libhashmod_gemm_probe.so")

if "--build" in sys.argv:
    from hashmodnffbanks_idr_amd import build as B
    with tempfile.TemporaryDirectory(prefix="gemm_probe_") as tmp:
        procs, objs = [], []
        for src in B.SOURCES:
            obj = os.path.join(tmp, src.replace(".hip", ".o"))
            cmd = [B.HIPCC] + B.FLAGS + (["-DHM_GEMM_PHASE_PROBE=1"] if src == "hm_gemm.hip" else []) + \
                  ["-c", os.path.join(B.CSRC, src), "-o", obj]
            procs.append(subprocess.Popen(cmd))
            objs.append(obj)
        if any(p.wait() != 0 for p in procs):
            raise SystemExit("hipcc failed")
        subprocess.check_call([B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", PROBE] + objs)
    print(PROBE)
    sys.exit(0)

import torch
from hashmodnffbanks_idr_amd import _lib, ops

dev = torch.device("cuda", 0)
read = _lib.lib().hm_gemm_probe_read
read.restype = C.c_int
read.argtypes = [C.c_void_p, C.c_int]
MHZ = 100.0   # wall_clock64(): 100 MHz constant clock


def phases(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = (C.c_ulonglong * 8)()
    assert read(ts, 8) == 0
    t = [int(v) for v in ts]
    d = lambda a, b: (t[b] - t[a]) / MHZ   # noqa: E731
    return d(0, 1), d(1, 2), t[5] / MHZ, d(2, 3), d(3, 4), d(0, 4)


print("%-44s %9s %9s %9s %9s %9s %9s" % ("shape (us per phase, one tile)", "1st fetch", "K loop", "(barrier)", "exchange",
                                        "epilogue", "total"))
for rows in (3072, 2048):
    x, w = torch.randn(rows, 512, device=dev), torch.randn(512, 512, device=dev)
    bias, out = torch.zeros(512, device=dev), torch.empty(rows, 512, device=dev)
    z, g = torch.randn(rows, 512, device=dev), torch.randn(rows, 512, device=dev)
    probs = [(torch.randn(2 * rows, 512, device=dev), torch.randn(2 * rows, 512, device=dev),
              torch.zeros(512, 512, device=dev)) for _ in range(8)]
    for label, fn in (
            (f"{rows} x 512 x 512 NT + Softplus", lambda: ops.gemm_ep(x, w, bias, False, True, ops.EPI_SOFTPLUS, 100.0, 20.0)),
            (f"{rows} x 512 x 512 NN plain", lambda: ops.gemm(x, w, None, False, False, out=out)),
            (f"{rows} x 512 x 512 NN + ADJOINT (not in bench)", lambda: ops.gemm_ep(x, w, None, False, False, ops.EPI_ADJOINT,
                                                                            100.0, 20.0, z=z, g=g, want_out3=True)),
            (f"grouped 8 x (512 x 512 x {2 * rows}) TN", lambda: ops.gemm_group_tn(probs))):
        print("%-44s %9.2f %9.2f %9.2f %9.2f %9.2f %9.2f" % ((label,) + phases(fn)))
