"""Writes tests/golden/guard_refined_counts.json: the number of coarse samples the guard refines (tracer statistic
guard_refined) per call of tests/test_guard_gpu.py's fixtures - raytrace_init / _bumpy / _C2, training and eval mode,
sampler head 0 and 16 - on the library that is loaded.  The marking rule and the approximate values are deterministic,
so the count is a property of the build: run this on the build that is to be the reference (HM_LIB_PATH selects another
build of the same ABI), and tests/test_split_schedule_gpu.py holds every later build to it.

    python scripts/guard_refined_counts.py [out.json]
"""
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "tests"), os.path.join(R, "tests", "golden")):
    sys.path.insert(0, p)

TAGS, MODES, HEADS = ("init", "bumpy", "C2"), ("train", "eval"), (0, 16)


def key(tag, mode, head):
    return f"{tag} {mode} head {head}"


def guarded_call(tag, mode, head):
    """(outputs, statistics) of the guarded tracer call of a fixture, as tests/test_guard_gpu.py makes it"""
    import numpy as np
    import test_guard_gpu as G
    g, net = G._fixture(lambda name: np.load(os.path.join(R, "tests", "golden", name + ".npz")), tag)
    return g, net, G._call(G._tracer(g, mode, head), net, G._rays(g), True)


if __name__ == "__main__":
    out = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(R, "tests", "golden", "guard_refined_counts.json")
    counts = {}
    for tag in TAGS:
        for mode in MODES:
            for head in HEADS:
                counts[key(tag, mode, head)] = int(guarded_call(tag, mode, head)[2][1]["guard_refined"])
    rec = {"how": "python scripts/guard_refined_counts.py on the build of the commit before the select kernels went to one "
                  "wave per row (serial one-thread-per-row marking); key = fixture, mode, sampler head",
           "guard_refined": counts}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
