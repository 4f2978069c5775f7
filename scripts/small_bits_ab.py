"""Did a change of the small-tile SDF bodies (csrc/hm_sdf.hip: sdf_small_body, Tile16, Tile8) move any bit?  Runs every
launch of tests/small_tile_cases.py - hm_sdf_fwd (both frac modes) and hm_sdf_fwd_emb at tile_points 4, 8 and 16, sdf-only
and all columns, on ragged point counts and networks with idle and partly filled waves - once on the library in the tree and
once on another build of the same ABI (HM_LIB_PATH: the parent commit's libhashmod.so), each in a child process of its
own, and compares the outputs byte for byte.

    HM_LIB_PATH=/path/to/parent/libhashmod.so python scripts/small_bits_ab.py [--write-golden]

--write-golden: tests/golden/small_tile_bits.npz <- the outputs of the HM_LIB_PATH build (never the tree's), whether or not
the tree agrees; tests/test_small_tile_round_gpu.py holds the tree to them.  Exit status 1 if any output differs, 2 if a child failed."""
import os
import subprocess
import sys
import tempfile

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "tests"), os.path.join(R, "tests", "golden")]
GOLDEN = os.path.join(R, "tests", "golden", "small_tile_bits.npz")


def child(path):
    import numpy as np
    import small_tile_cases as T
    np.savez_compressed(path, **T.record())


def run(lib_path, out):
    env = dict(os.environ)
    env.pop("HM_LIB_PATH", None)
    if lib_path:
        env["HM_LIB_PATH"] = lib_path
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=env, timeout=600)
    if r.returncode != 0:
        print(f"child on {lib_path or 'the tree library'} failed with status {r.returncode}")
        sys.exit(2)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(sys.argv[sys.argv.index("--child") + 1])
        sys.exit(0)
    import numpy as np
    import small_tile_cases as T
    other = os.environ.get("HM_LIB_PATH")
    if not other:
        raise SystemExit("set HM_LIB_PATH to the build to compare the tree library with")
    with tempfile.TemporaryDirectory(prefix="small_bits_ab_") as tmp:
        pa, pb = os.path.join(tmp, "tree.npz"), os.path.join(tmp, "other.npz")
        run(None, pa)
        run(os.path.abspath(other), pb)
        a, b = np.load(pa), np.load(pb)
        diff = sorted(k for k in b.files if k not in a.files or not T.same_bits(a[k], b[k]))
        if "--write-golden" in sys.argv:
            np.savez_compressed(GOLDEN, **{k: b[k] for k in b.files})
            print(f"wrote {len(b.files)} outputs of {other} to {os.path.relpath(GOLDEN, R)}")
        n = len(b.files)
    for k in diff:
        print("DIFFERS:", k)
    ok = not diff and set(a.files) == set(b.files)
    print(f"{n} outputs, {len(diff)} differ: " + ("bit-identical" if ok else "NOT identical"))
    sys.exit(0 if ok else 1)
