#!/usr/bin/env python3
"""Did the device code move?  Compares the gfx950 assembly of a git revision with the working tree's, kernel by kernel.

    python scripts/kernel_isa_diff.py [REV] [SOURCE.hip ...]      (REV: default HEAD; sources: default build.SOURCES)

Both trees are compiled with the library's own flags plus `--cuda-device-only -S` (no GPU needed).  Per source it
reports the kernels present on one side only, the kernels whose instruction stream differs and the kernels whose
`.amdhsa_kernel` descriptor (VGPR / AGPR / SGPR counts, LDS, scratch) differs, then one summary line.  Exit status 1
if any source has any of them: a refactor of host code passes with 0.

    --alias REGEX=REPLACEMENT    (repeatable) rewrite REV's symbol names with re.sub before matching, for a change that
                                 renames kernels or gives them template parameters: REV's kernel is then compared with
                                 the working tree's kernel of the new name.  Symbols are the mangled names of the
                                 assembly; the rewrite covers REV's labels and every compared line.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hashmodnffbanks_idr_amd import build  # noqa: E402

CSRC_REL = os.path.relpath(build.CSRC, ROOT)
MAX_JOBS = 16


def compile_asm(tree, src, out):
    """Assembly of tree's csrc/src, or None when that tree has no such source."""
    path = os.path.join(tree, CSRC_REL, src)
    if not os.path.exists(path):
        return None
    inc = os.path.join(build.ROOT, "include")
    flags = [os.path.join(tree, "include") if f == inc else f for f in build.FLAGS]
    cmd = [build.HIPCC] + flags + ["--cuda-device-only", "-S", path, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {path}:\n{r.stderr}")
    return out


def kernels(path, aliases=()):
    """{symbol: (instruction stream, descriptor)} of one assembly file; both are lists of comment-free lines.
    aliases: (compiled regex, replacement) pairs applied to every line first, symbol names included."""
    out = {}
    if path is None:
        return out
    name, cur, desc, in_desc = None, None, None, False
    for ln in open(path):
        for rx, to in aliases:
            ln = rx.sub(to, ln)
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m:
            name = m.group(1)
            continue
        if cur is None:
            if name is not None and ln.startswith(name + ":"):
                cur, desc = [], []
                out[name] = (cur, desc)
            continue
        if ln.startswith(".Lfunc_end"):
            name = cur = None
            continue
        s = ln.split(";")[0].rstrip()
        if not s.strip():
            continue
        if s.strip().startswith(".amdhsa_kernel "):
            in_desc = True
        elif s.strip() == ".end_amdhsa_kernel":
            in_desc = False
        elif in_desc:
            desc.append(s.strip())
        else:
            # .LBB<n>_ carries the function's ordinal in the file, which moves when the instantiation order moves
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    # a device function that is no kernel has no descriptor: keep it, its code is compared all the same
    return out


def compare(src, a, b, rev, aliases=()):
    ka, kb = kernels(a, aliases), kernels(b)
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    both = sorted(set(ka) & set(kb))
    isa = [k for k in both if ka[k][0] != kb[k][0]]
    desc = [k for k in both if ka[k][1] != kb[k][1]]
    for k in only_a:
        print(f"{src}: only in {rev}: {k}")
    for k in only_b:
        print(f"{src}: only in the working tree: {k}")
    for k in isa:
        print(f"{src}: instruction stream differs: {k} ({len(ka[k][0])} -> {len(kb[k][0])} lines)")
    for k in desc:
        changed = sorted(set(ka[k][1]) ^ set(kb[k][1]))
        print(f"{src}: descriptor differs: {k}: " + "; ".join(changed))
    same = sum(1 for k in both if k not in isa and k not in desc)
    print(f"{src}: {len(ka)} kernels in {rev}, {len(kb)} in the working tree, {same} identical, "
          f"{len(isa)} instruction streams differ, {len(desc)} descriptors differ, "
          f"{len(only_a)} only in {rev}, {len(only_b)} only in the working tree", flush=True)
    return bool(only_a or only_b or isa or desc)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rev", nargs="?", default="HEAD", help="git revision to compare the working tree with")
    ap.add_argument("sources", nargs="*", default=build.SOURCES, help="sources under csrc/ (default: all)")
    ap.add_argument("--jobs", type=int, default=min(MAX_JOBS, os.cpu_count() or 1), help=f"compiler jobs (at most {MAX_JOBS})")
    ap.add_argument("--alias", action="append", default=[], metavar="REGEX=REPLACEMENT",
                    help="rewrite the revision's (mangled) symbol names with re.sub before matching; repeatable")
    args = ap.parse_args()
    aliases = []
    for a in args.alias:
        rx, sep, to = a.partition("=")
        if not sep or not rx:
            ap.error(f"--alias {a!r}: REGEX=REPLACEMENT expected")
        aliases.append((re.compile(rx), to))
    rev = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", args.rev], text=True).strip()
    sources = [os.path.basename(s) for s in args.sources]
    with tempfile.TemporaryDirectory(prefix="kernel_isa_diff_") as tmp:
        old = os.path.join(tmp, "rev")
        os.makedirs(old)
        ar = subprocess.Popen(["git", "-C", ROOT, "archive", rev, CSRC_REL, "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", old], stdin=ar.stdout)
        if ar.wait() != 0:
            raise RuntimeError(f"git archive {rev} failed")
        with ThreadPoolExecutor(max_workers=max(1, min(MAX_JOBS, args.jobs))) as pool:
            jobs = [(src, pool.submit(compile_asm, old, src, os.path.join(tmp, "a_" + src + ".s")),
                     pool.submit(compile_asm, ROOT, src, os.path.join(tmp, "b_" + src + ".s"))) for src in sources]
            moved = [compare(src, fa.result(), fb.result(), rev, aliases) for src, fa, fb in jobs]
    n = sum(moved)
    print(f"device code {'MOVED in ' + str(n) + ' of' if n else 'identical in all'} {len(sources)} sources (against {rev})")
    return 1 if n else 0


if __name__ == "__main__":
    sys.exit(main())
