"""Did a change of csrc/hm_gemm.hip move any bit?  Runs the six shapes of bench.py's roofline_gemm and the five epilogue
modes of the chain shapes on seeded random fp32 data, once on the library in the tree and once on another build of the same
ABI (HM_LIB_PATH, e.g. the parent commit's libhashmod.so), each in a child process of its own, and compares the SHA-256 of
every output.

    HM_LIB_PATH=/path/to/other/libhashmod.so python scripts/gemm_bits_ab.py

The grouped weight-gradient shapes are compared in the deterministic mode only: their default mode adds k parts with
atomics, whose order is not reproducible from run to run on ONE build.  Exit status 1 if any output differs.
"""
import hashlib
import json
import os
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)


def child():
    import torch
    from hashmodnffbanks_idr_amd import ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    R_ = lambda *s: torch.randn(s, generator=gen, device=dev)   # noqa: E731
    out = {}

    def put(name, *ts):
        for i, t in enumerate(ts):
            if t is not None:
                out[f"{name}[{i}]"] = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()

    for rows in (3072, 2048):
        x, w = R_(rows, 512) * 0.3, R_(512, 512) * 0.2
        bias, z, g = R_(512) * 0.1, R_(rows, 512) * 0.05, R_(rows, 512)
        for tb in (True, False):
            tag = f"{rows} {'NT' if tb else 'NN'}"
            put(tag + " plain", ops.gemm(x, w, None, False, tb))
            put(tag + " softplus", *ops.gemm_ep(x, w, bias, False, tb, ops.EPI_SOFTPLUS, 100.0, 20.0))
            put(tag + " relu", *ops.gemm_ep(x, w, bias, False, tb, ops.EPI_RELU, 100.0, 20.0))
            put(tag + " s1mul", *ops.gemm_ep(x, w, None, False, tb, ops.EPI_S1MUL, 100.0, 20.0, scale=0.7071067811865476,
                                             z=z, g=g, nz=508))
            put(tag + " relumask", *ops.gemm_ep(x, w, None, False, tb, ops.EPI_RELUMASK, 100.0, 20.0, z=z, g=g, nz=512,
                                                want_c=False))
            put(tag + " adjoint", *ops.gemm_ep(x, w, None, False, tb, ops.EPI_ADJOINT, 100.0, 20.0, z=z, g=g,
                                               want_out3=True))
        probs = [(R_(2 * rows, 512), R_(2 * rows, 512), torch.zeros(512, 512, device=dev)) for _ in range(8)]
        with ops.deterministic(True):
            ops.gemm_group_tn(probs)
            put(f"{rows} plain NN deterministic", ops.gemm(x[:256], w, None, False, False))   # split K, part kernels
        put(f"grouped K={2 * rows} deterministic", *[c for _, _, c in probs])
    torch.cuda.synchronize()
    print("HASHES " + json.dumps(out))


def run(lib_path):
    env = dict(os.environ)
    env.pop("HM_LIB_PATH", None)
    if lib_path:
        env["HM_LIB_PATH"] = lib_path
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdout=subprocess.PIPE, text=True,
                       timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"child on {lib_path or 'the tree library'} failed with status {r.returncode}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("HASHES ")][-1]
    return json.loads(line[len("HASHES "):])


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
        sys.exit(0)
    other = os.environ.get("HM_LIB_PATH")
    if not other:
        raise SystemExit("set HM_LIB_PATH to the build to compare the tree library with")
    a, b = run(None), run(os.path.abspath(other))
    diff = sorted(k for k in a if a[k] != b.get(k))
    for k in diff:
        print("DIFFERS:", k)
    print(f"{len(a)} outputs, {len(diff)} differ: " + ("NOT identical" if diff or set(a) != set(b) else "bit-identical"))
    sys.exit(1 if diff or set(a) != set(b) else 0)
