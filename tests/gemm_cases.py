"""The GEMM case matrix shared by tests/test_gemm_plan_cpu.py (the route every case must take, asserted on CPU through
hm_diag_gemm_plan) and tests/test_gemm_paths_gpu.py (the same cases run on the device against float64).

A case names the route it is meant to cover; the CPU test fails when a planner change moves it elsewhere, instead of the
GPU test silently covering another kernel."""
import ctypes
from collections import namedtuple

GENERIC, BIG, PIPE64, PIPE96 = 1, 2, 3, 4          # hm_gemm_plan_info.kernel (include/hashmod.h)
FAMILY = {GENERIC: "generic", BIG: "big", PIPE64: "pipe64", PIPE96: "pipe96"}

# Layout of one stored operand: row stride cols + pad, first element `off` floats past a 16-byte boundary.
Layout = namedtuple("Layout", "pad off")
DENSE = Layout(0, 0)
LAYOUTS = {"dense": DENSE, "pad3": Layout(3, 0), "off1": Layout(4, 1), "off2": Layout(4, 2), "off3": Layout(5, 3)}

# ep: None (hm_gemm_f32 / _det) or "relu" / "relumask" (hm_gemm_f32_ep, exact on integers)
# kernel / k_tail / split: the intended route (split: True = K over several workgroups, with det: the part kernels)
Case = namedtuple("Case", "name ta tb M N K la lb ep det acc bias kernel k_tail split")


def _case(name, ta, tb, M, N, K, kernel, k_tail=False, split=False, la=DENSE, lb=DENSE, ep=None, det=False, acc=False,
          bias=True):
    return Case(name, ta, tb, M, N, K, la, lb, ep, det, acc, bias, kernel, k_tail, split)


FORMS = {"NN": (0, 0), "NT": (0, 1), "TN": (1, 0), "TT": (1, 1)}


def stored_shape(case, which):
    """(rows, cols) of the stored A or B: A is [M, K] (ta = 0, k-contiguous) or [K, M]; B is [K, N] or [N, K] (tb = 1,
    k-contiguous)"""
    if which == "A":
        return (case.K, case.M) if case.ta else (case.M, case.K)
    return (case.N, case.K) if case.tb else (case.K, case.N)


def ld_of(case, which):
    lay = case.la if which == "A" else case.lb
    return stored_shape(case, which)[1] + lay.pad


def vec_expected(case, which):
    """the documented rule for the generic / big kernels' 16-byte loads: a k-contiguous operand whose rows start on
    16-byte boundaries and whose K range ends on a multiple of 4"""
    kc = (not case.ta) if which == "A" else bool(case.tb)
    lay = case.la if which == "A" else case.lb
    return kc and case.K % 4 == 0 and ld_of(case, which) % 4 == 0 and lay.off == 0


def instantiation(case, info):
    """the kernel template instance a planned call launches (the kernel choice at the end of hm_gemm.hip's gemm_impl)"""
    akc, bkc, ep = int(not case.ta), int(case.tb), int(case.ep is not None)
    fam = FAMILY[info.kernel]
    if info.part:
        if info.kernel in (PIPE64, PIPE96):
            return ("part-" + fam, akc, bkc)
        return ("part-generic", info.vec_a, info.vec_b)
    if info.kernel in (GENERIC, BIG):
        return (fam, info.vec_a, info.vec_b, ep)
    return (fam, akc, bkc, ep, info.k_tail)


def all_instantiations():
    """every instance hm_gemm_f32 / _ep / _det can launch"""
    out = set()
    for fam in ("generic", "big"):
        out |= {(fam, va, vb, ep) for va in (0, 1) for vb in (0, 1) for ep in (0, 1)}
    for fam in ("pipe64", "pipe96"):
        for akc in (0, 1):
            for bkc in (0, 1):
                for ep in (0, 1):
                    out.add((fam, akc, bkc, ep, 0))
                    if not (akc and bkc):          # a K tail needs an operand with k as its slow dimension
                        out.add((fam, akc, bkc, ep, 1))
        out |= {("part-" + fam, akc, bkc) for akc in (0, 1) for bkc in (0, 1)}
    out |= {("part-generic", va, vb) for va in (0, 1) for vb in (0, 1)}
    return out


def plan(case, ptr_a, ptr_b):
    """hm_diag_gemm_plan for the case with the given operand addresses"""
    from hashmodnffbanks_idr_amd import _lib
    info = _lib.GemmPlanInfo()
    _lib.check(_lib.lib().hm_diag_gemm_plan(case.ta, case.tb, case.M, case.N, case.K, ctypes.c_void_p(ptr_a),
                                            ld_of(case, "A"), ctypes.c_void_p(ptr_b), ld_of(case, "B"),
                                            int(case.ep is not None), int(case.det), ctypes.byref(info)))
    return info


def fake_ptr(case, which):
    """an address with the case's alignment (the plan reads no memory)"""
    lay = case.la if which == "A" else case.lb
    return 0x7f0000100000 + 4 * lay.off


def check_route(case, info):
    """assert that the plan is the case's intended route; returns the instantiation"""
    want = (FAMILY[case.kernel], case.k_tail, case.split, case.det and case.split)
    got = (FAMILY.get(info.kernel, info.kernel), bool(info.k_tail), info.split > 1, bool(info.part))
    assert got == want, f"{case.name}: plan {got} (split {info.split}, k_chunk {info.k_chunk}), intended {want}"
    if case.kernel in (GENERIC, BIG):
        assert (info.vec_a, info.vec_b) == (int(vec_expected(case, "A")), int(vec_expected(case, "B"))), case.name
    return instantiation(case, info)


# ---- the matrix ----------------------------------------------------------------------------------------------------
# shapes per family (M, N, K-whole, K-tail): generic = small tile grids (K = 190: below the pipelined kernel's tail
# minimum even with an epilogue); big = ceil(M/128) ceil(N/128) >= 256;
# pipe64 = 256 tiles of 64 x 64; pipe96 = 384 tiles of 64 x 64 but 256 of 96 x 64
FAMILY_SHAPES = {GENERIC: (300, 200, 100, 190), BIG: (8192, 512, 512, 445), PIPE64: (2048, 512, 512, 445),
                 PIPE96: (3072, 512, 512, 257)}


def _routes():
    cs = []
    for kern, (M, N, Kw, Kt) in FAMILY_SHAPES.items():
        f = FAMILY[kern]
        for form, (ta, tb) in FORMS.items():
            for ep in (None, "relumask", "relu"):
                # every form with and without the epilogue, K whole; accumulate without bias on the plain call
                acc = ep is None and form in ("NN", "TT")
                cs.append(_case(f"{f}-{form}-K{Kw}-{ep}", ta, tb, M, N, Kw, kern, ep=ep, acc=acc, bias=not acc or
                                form == "TT"))
                # the K tail (a pipelined kernel only where one operand has k as its slow dimension)
                tail_kern = kern if (kern in (GENERIC, BIG) or form != "NT") else GENERIC
                cs.append(_case(f"{f}-{form}-K{Kt}-{ep}", ta, tb, M, N, Kt, tail_kern, ep=ep,
                                k_tail=tail_kern in (PIPE64, PIPE96), acc=acc))
    # 100-deep K on the big tile: three 32-deep stages and a partial one
    for form, (ta, tb) in FORMS.items():
        cs.append(_case(f"big-{form}-K100", ta, tb, 8192, 512, 100, BIG, ep="relumask" if ta else None))
    # split K: atomics into a zeroed (or accumulated) C, and the deterministic part kernels + reduce
    split_shapes = {GENERIC: (256, 192, 1000), PIPE64: (256, 256, 2048), PIPE96: (2880, 512, 768)}
    for kern, (M, N, K) in split_shapes.items():
        f = FAMILY[kern]
        for form, (ta, tb) in FORMS.items():
            for det in (False, True):
                for acc in (False, True):
                    cs.append(_case(f"{f}-split-{form}-det{int(det)}-acc{int(acc)}", ta, tb, M, N, K, kern, split=True,
                                    det=det, acc=acc, bias=(form in ("NN", "TN")) != acc))
    # misaligned / padded operand views on every family, K whole and K tail, both kinds of operand
    for kern, (M, N, Kw, Kt) in FAMILY_SHAPES.items():
        f = FAMILY[kern]
        for K in (Kw, Kt):
            for form in ("NN", "TT"):
                ta, tb = FORMS[form]
                for lname in ("pad3", "off1", "off2", "off3"):
                    lay = LAYOUTS[lname]
                    cs.append(_case(f"{f}-{form}-K{K}-{lname}", ta, tb, M, N, K, kern, k_tail=kern in (PIPE64, PIPE96)
                                    and K == Kt, la=lay, lb=lay, ep="relumask" if lname == "off2" else None))
    return cs


ROUTES = _routes()


def _isolation():
    """non-finite values in one row of op(A) and one column of op(B): NN and TT at K tails, dense and padded"""
    cs = []
    for kern, (M, N, _, _) in FAMILY_SHAPES.items():
        f = FAMILY[kern]
        for form in ("NN", "TT"):
            ta, tb = FORMS[form]
            for K in (445, 257, 192, 385):
                for lname, lay in (("dense", DENSE), ("pad3", LAYOUTS["pad3"])):
                    cs.append(_case(f"{f}-{form}-K{K}-{lname}", ta, tb, M, N, K, kern, k_tail=kern in (PIPE64, PIPE96),
                                    split=kern == GENERIC and K >= 256, la=lay, lb=lay, bias=False))
    return cs


ISOLATION = _isolation()

# edge shapes on the generic kernel: M, N in {1, tile +- 1} of the 64-, 96- and 128-row tiles
EDGE_DIMS = (1, 63, 65, 95, 97, 127, 129)
EDGE_MN = [_case(f"edge-M{M}-N{N}", (M + N) % 2, (M // 2 + N) % 2, M, N, 67, GENERIC) for M in EDGE_DIMS
           for N in EDGE_DIMS]
EDGE_K = [_case(f"edge-K{K}-{form}", ta, tb, 130, 97, K, GENERIC, split=K >= 256, acc=K % 2 == 1) for K in
          (1, 2, 3, 4, 127, 129, 191, 192, 255, 257, 385, 445) for form, (ta, tb) in FORMS.items()]
# ragged last tiles of the big and pipelined kernels, and both sides of the big-tile threshold
EDGE_BIG = [
    _case("big-ragged-8193x511", 0, 1, 8193, 511, 512, BIG),
    _case("big-ragged-8100x445-K445", 0, 0, 8100, 445, 445, BIG),
    _case("pipe64-ragged-2047x511", 0, 0, 2047, 511, 512, PIPE64),
    _case("pipe96-ragged-3071x511", 1, 1, 3071, 511, 445, PIPE96, k_tail=True),
    _case("threshold-8000x512", 0, 1, 8000, 512, 512, PIPE64),
    _case("threshold-8192x512", 0, 1, 8192, 512, 512, BIG),
]
# K = 0: C = bias (or C += bias); one generic and one big-tile grid
K0 = [_case("k0-generic", 0, 0, 300, 200, 0, GENERIC), _case("k0-big", 1, 1, 8192, 512, 0, BIG)]
# subnormal operands, exact products
SUBNORMAL = [_case("subnormal-generic", 0, 1, 300, 200, 100, GENERIC),
             _case("subnormal-pipe64", 0, 0, 2048, 512, 445, PIPE64, k_tail=True)]

# epilogue outputs with a scale, one shape per family
EPILOGUE = [_case("ep-generic-NT", 0, 1, 300, 200, 100, GENERIC, ep="relu"),
            _case("ep-big-TN", 1, 0, 8192, 512, 512, BIG, ep="relu"),
            _case("ep-pipe64-NN-tail", 0, 0, 2048, 512, 445, PIPE64, k_tail=True, ep="relu"),
            _case("ep-pipe96-TT", 1, 1, 3072, 512, 512, PIPE96, ep="relu")]

ALL = ROUTES + EPILOGUE + ISOLATION + EDGE_MN + EDGE_K + EDGE_BIG + K0 + SUBNORMAL
