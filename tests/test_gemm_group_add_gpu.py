"""hm_gemm_f32_group_tn_add / _det through ops.gemm_group_tn_add: the grouped weight-gradient product over operands with
addends on row ranges, C += (A + pad(A2))^T (B + pad(B2)).

Every A, B is a view of row stride cols + 3 in a NaN-filled buffer and every addend a row slice of a larger NaN-filled
buffer, so a read outside an operand or outside an addend's range poisons the result; every C holds values beforehand,
because the product accumulates.

  deterministic mode  the result is torch.equal to ops.gemm_group_tn (the addend-free entry point) on operands added
                      beforehand with torch.add in fp32: the same single rounding per element and the same k parts.
  default mode        every element within K * 2^-24 * (|A + A2|^T |B + B2|) of C0 + (A + A2)^T (B + B2) formed in
                      float64 from the inputs (the standard dot-product bound; |C0| <= 1 is far below the products'
                      magnitude sums, so its one rounding does not show against K of them).
  integer operands    values in [-8, 8]: sums of two in [-16, 16], products <= 256, K <= 4096 of them below 2^24 - every
                      fp32 order is exact, so both modes must give the float64 result bit for bit.

Lists: `small` is K = 2 * 40 with ranges at k0 = 8 (4-aligned, not 32-aligned) over M, N in {64, 96, 33}: both addends,
only A's, none, an empty and a whole-K range, and a range of 6 - these run on the plain GEMM with the addend added
beforehand (K is no multiple of 128); its last problem, K = 128 with the same k0 = 8, runs in the grouped kernel's
addend instance.  `split` has K = 1536, M = N = 64 of the issue and the lists' shapes at K = 1536,
2048 (two k parts, a range across their boundary) and 4096 (four), which run in the grouped kernel's addend instance,
one range of 6 among them (added beforehand, same table), one problem without addends in the same table."""
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (M, N, K, (a_k0, a_rows) or None, (b_k0, b_rows) or None)
LISTS = {
    "small": [
        (64, 96, 80, (8, 24), (8, 40)),
        (96, 33, 80, (8, 32), None),
        (33, 64, 80, None, None),
        (64, 64, 80, (8, 0), (0, 80)),
        (96, 96, 80, (8, 6), None),
        (96, 33, 128, (8, 40), (8, 24)),
    ],
    "split": [
        (64, 64, 1536, (8, 40), (1024, 512)),
        (96, 33, 2048, (520, 1000), (8, 1000)),
        (33, 96, 4096, (1024, 3072), (0, 4096)),
        (64, 33, 1536, None, None),
        (33, 33, 1536, (8, 0), (1532, 4)),
        (64, 96, 1536, (8, 6), (4, 1528)),
    ],
}


def _ops():
    from hashmodnffbanks_idr_amd import ops
    return ops


def _framed(rows, cols, vals):
    """vals as a [rows, cols] view of row stride cols + 3, three rows into a NaN-filled buffer"""
    store = torch.full((rows + 6, cols + 3), float("nan"), device=DEV)
    v = store[3:3 + rows, :cols]
    v.copy_(vals)
    return v


def _draw(shape, gen, kind):
    if kind == "int":
        return torch.randint(-8, 9, shape, generator=gen, device=DEV).float()
    return torch.randn(shape, generator=gen, device=DEV)


class Built:
    def __init__(self, name, kind):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(zlib.crc32(f"group_add/{name}/{kind}".encode()))
        self.problems, self.pre, self.c0, self.ref, self.bound, self.K = [], [], [], [], [], []
        for M, N, K, ar, br in LISTS[name]:
            a, b = _framed(K, M, _draw((K, M), gen, kind)), _framed(K, N, _draw((K, N), gen, kind))
            c0 = torch.randint(-8, 9, (M, N), generator=gen, device=DEV).float() * (1.0 if kind == "int" else 0.125)
            adds, sums, pre = [], [], []
            for x, rng in ((a, ar), (b, br)):
                s64 = x.double()
                p = x
                if rng is None:
                    adds.append(None)
                else:
                    k0, rows = rng
                    x2 = _framed(rows, x.shape[1], _draw((rows, x.shape[1]), gen, kind))
                    adds.append((x2, k0))
                    s64 = s64.clone()
                    s64[k0:k0 + rows] += x2.double()
                    p = x.clone()
                    p[k0:k0 + rows] = torch.add(x[k0:k0 + rows], x2)
                sums.append(s64)
                pre.append(p)
            self.problems.append((a, b, adds[0], adds[1]))
            self.pre.append(tuple(pre))
            self.c0.append(c0)
            self.ref.append(c0.double() + sums[0].t() @ sums[1])
            self.bound.append(K * 2.0 ** -24 * (sums[0].abs().t() @ sums[1].abs()))
            self.K.append(K)

    def run(self, det, add=True):
        """fresh C windows (row stride N + 3) through the entry point with addends, or the addend-free one on the
        operands added beforehand"""
        ops = _ops()
        cs = []
        for c0 in self.c0:
            store = torch.full((c0.shape[0], c0.shape[1] + 3), 7.0, device=DEV)
            c = store[:, :c0.shape[1]]
            c.copy_(c0)
            cs.append(c)
        with ops.deterministic(det):
            if add:
                ops.gemm_group_tn_add([(a, b, c, aa, ba) for (a, b, aa, ba), c in zip(self.problems, cs)])
            else:
                ops.gemm_group_tn([(a, b, c) for (a, b), c in zip(self.pre, cs)])
        torch.cuda.synchronize()
        return cs


_BUILT = {}


def _built(name, kind):
    if (name, kind) not in _BUILT:
        _BUILT[(name, kind)] = Built(name, kind)
    return _BUILT[(name, kind)]


@pytest.mark.parametrize("name", sorted(LISTS))
def test_deterministic_bits_of_preadded_operands(name):
    b = _built(name, "randn")
    got, want = b.run(True), b.run(True, add=False)
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.isfinite(g).all(), f"{name}[{i}]: a read outside an operand or an addend's range"
        assert torch.equal(g, w), f"{name}[{i}]: {(g - w).abs().max().item():.3e} from the addend-free entry point"
    again = b.run(True)
    assert all(torch.equal(g, a) for g, a in zip(got, again)), f"{name}: not reproducible"


@pytest.mark.parametrize("name", sorted(LISTS))
def test_default_mode_within_dot_product_bound(name):
    b = _built(name, "randn")
    for i, g in enumerate(b.run(False)):
        assert torch.isfinite(g).all(), f"{name}[{i}]: a read outside an operand or an addend's range"
        err = (g.double() - b.ref[i]).abs()
        worst = (err / b.bound[i]).max().item()
        print(f"{name}[{i}] K={b.K[i]}: max err {err.max().item():.3e}, {worst:.4f} of the bound")
        assert (err <= b.bound[i]).all(), f"{name}[{i}]: {worst:.3f} of K 2^-24 |A+A2|^T |B+B2|"


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("name", sorted(LISTS))
def test_integer_operands_exact(name, det):
    b = _built(name, "int")
    for i, g in enumerate(b.run(det)):
        assert torch.equal(g.double(), b.ref[i]), \
            f"{name}[{i}]: {(g.double() - b.ref[i]).abs().max().item():.3e} from the exact result"


def test_c_frame_untouched_and_bad_addend_refused():
    ops = _ops()
    a, bm = torch.randn(1536, 64, device=DEV), torch.randn(1536, 64, device=DEV)
    store = torch.full((64, 67), 7.0, device=DEV)
    c = store[:, :64]
    c.zero_()
    ops.gemm_group_tn_add([(a, bm, c, (torch.randn(64, 64, device=DEV), 128), None)])
    torch.cuda.synchronize()
    assert (store[:, 64:] == 7.0).all()
    with pytest.raises(ValueError):
        ops.gemm_group_tn_add([(a, bm, c, (torch.randn(64, 64, device=DEV), 1500), None)])   # past K
    with pytest.raises(ValueError):
        ops.gemm_group_tn_add([(a, bm, c, (torch.randn(64, 32, device=DEV), 0), None)])      # wrong width
