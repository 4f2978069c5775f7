"""Did a change of csrc/hm_sdf_split.hip move any bit?  Runs hm_sdf_fwd_split and hm_sdf_fwd_emb_split, both kinds
(bf16x2, f16x2), the grid form in both frac modes, on the `c2`, `odd_tiles`, `w32`, `ragged` and `depth1` networks of tests/sdf_shapes.py over seeded points,
once on the library in the tree and once on another build of the same ABI (HM_LIB_PATH, e.g. the parent commit's
libhashmod.so), each in a child process of its own, and compares the SHA-256 of every output.

    HM_LIB_PATH=/path/to/other/libhashmod.so python scripts/split_bits_ab.py

Point counts: one ragged tile, and more than one tile per workgroup (64 * 257 + 5).  Exit status 1 if any output differs.
"""
import hashlib
import json
import os
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
sys.path.insert(0, os.path.join(R, "tests", "golden"))

NETS = ("c2", "odd_tiles", "w32", "ragged", "depth1")
COUNTS = (200, 64 * 257 + 5)


def child():
    import torch
    import params as P
    import sdf_shapes as S
    from helpers import make_implicit
    from hashmodnffbanks_idr_amd import ops
    out = {}
    for name in NETS:
        case = S.BY_NAME[name]
        net = make_implicit(S.grid_config(case), case.hidden, case.fvs, 11, 0.3, 0.3, skip_in=case.skip)
        net.eval()
        emb = net._hash_embedder()
        desc, table, B, frac = emb.desc, emb.table.detach(), emb.freq_encoding.B, ops.FRAC_MODES[emb.frac_mode]
        for n in COUNTS:
            x = torch.from_numpy(P.make_points(77, n, -1.05, 1.05)).cuda()
            with torch.no_grad():
                e = ops.encode_fwd(desc, x, table, B, frac)
                for kind in ("bf16x2", "f16x2"):
                    net.coarse_split = kind
                    pk = net.packed_weights()
                    for form, t in (("grid", ops.sdf_fwd_split(desc, pk, x, table, B, frac)),
                                    ("grid-trilinear", ops.sdf_fwd_split(desc, pk, x, table, B, 1)),
                                    ("emb", ops.sdf_fwd_emb_split(pk, e))):
                        out[f"{name} n={n} {kind} {form}"] = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()
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
