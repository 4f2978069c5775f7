"""What a change of the layer schedule of the split-operand kernel (csrc/hm_sdf_split.hip: which wave owns which feature
tile, where the barriers and epilogues of a layer sit) must keep, and the wave-per-row guard select kernels
(csrc/hm_trace.hip).  A schedule can go wrong where its phases meet - a tile read before its epilogue, an epilogue over
a range that is still read, a wave without a tile at a barrier - so the networks are the shapes of tests/sdf_shapes.py
with one tile, odd tile counts, layers of different widths, adjacent skips and a single hidden layer, at point counts
around the 64-point tile, both kinds (bf16x2, f16x2) and both entry forms (hash grid, precomputed embedding rows).
scripts/split_bits_ab.py is the companion that compares two builds of the kernel bit for bit."""
import json
import os

import pytest
import torch

import params as P
import sdf_shapes as S
from helpers import make_implicit, mlp_fp64

pytestmark = pytest.mark.gpu

NETS = ["c2", "odd_tiles", "w32", "depth1", "ragged", "skip_3_4", "L2"]
KINDS = ("bf16x2", "f16x2")
FORMS = ("grid", "emb")
N = 200
COUNTS = (1, 33, 64, 65, 200)
_STATE = {}


def _state(name):
    """the case's network, 200 seeded points, their embedding rows (in a wider NaN-padded buffer), the exact-fp32 kernel's
    values and the float64 evaluation - built once per case and left unchanged"""
    if name not in _STATE:
        from hashmodnffbanks_idr_amd import ops
        case = S.BY_NAME[name]
        net = make_implicit(S.grid_config(case), case.hidden, case.fvs, 11, 0.3, 0.3, skip_in=case.skip)
        net.eval()
        emb = net._hash_embedder()
        grid = (emb.desc, emb.table.detach(), emb.freq_encoding.B, ops.FRAC_MODES[emb.frac_mode])
        x = torch.from_numpy(P.make_points(1042, N, -1.05, 1.05)).cuda()
        with torch.no_grad():
            ref32 = net.sdf(x)
            e = ops.encode_fwd(grid[0], x, grid[1], grid[2], grid[3])
            ref64 = mlp_fp64(net, e)[0][:, 0]
        _STATE[name] = dict(net=net, grid=grid, x=x, e=_strided(e), ref32=ref32, ref64=ref64, packed={})
    return _STATE[name]


def _strided(e, pad=5):
    buf = torch.full((e.shape[0], e.shape[1] + pad), float("nan"), device=e.device)
    buf[:, :e.shape[1]] = e
    return buf[:, :e.shape[1]]


def _packed(st, kind):
    if kind not in st["packed"]:
        net = st["net"]
        net.coarse_split = kind
        try:
            st["packed"][kind] = net.packed_weights()
            assert st["packed"][kind].split == kind
        finally:
            net.coarse_split = None
    return st["packed"][kind]


def _run(st, kind, form, x, e, n_dev=None):
    from hashmodnffbanks_idr_amd import ops
    pk = _packed(st, kind)
    desc, table, B, frac = st["grid"]
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device="cuda")
    with torch.no_grad():
        if form == "grid":
            return ops.sdf_fwd_split(desc, pk, x, table, B, frac, n_dev=nd)
        return ops.sdf_fwd_emb_split(pk, e, n_dev=nd)


@pytest.mark.parametrize("name", NETS)
def test_against_float64(name):
    """launches of 1, 33, 64, 65 and 200 points at the bounds of tests/test_split_gpu.py.  The fp32 kernel's own error
    that the f16x2 bounds scale with is a statistic, taken once over the case's 200 points for every launch size (one point
    is no sample of it); the split kernel's max and mean are over the points of the launch."""
    st = _state(name)
    e32 = (st["ref32"].double() - st["ref64"]).abs()
    e32_max, e32_mean = e32.max().item(), e32.mean().item()
    for kind in KINDS:
        for form in FORMS:
            for n in COUNTS:
                got = _run(st, kind, form, st["x"][:n], st["e"][:n])
                assert got.shape == (n,) and torch.isfinite(got).all()
                esp = (got.double() - st["ref64"][:n]).abs()
                d = (got - st["ref32"][:n]).abs()
                print(f"{name} {kind} {form} n={n}: vs fp64 max {esp.max().item():.3e} mean {esp.mean().item():.3e}; fp32 "
                      f"kernel vs fp64 max {e32_max:.3e} mean {e32_mean:.3e}; vs fp32 kernel max {d.max().item():.3e}")
                what = f"{kind} {form} n={n}"
                if kind == "f16x2":
                    assert esp.max().item() <= max(8 * e32_max, 2e-6), what
                    assert esp.mean().item() <= max(4 * e32_mean, 2e-7), what
                    assert d.max().item() <= 1e-5, what
                else:
                    assert esp.max().item() <= 2e-4 and esp.mean().item() <= 2e-5, what


@pytest.mark.parametrize("name", NETS)
def test_position_independence_and_determinism(name):
    """a point's value does not depend on its place in the tile, on the launch's size or on n_dev, and a call repeats"""
    st = _state(name)
    x, e = st["x"], st["e"]
    for kind in KINDS:
        for form in FORMS:
            full = _run(st, kind, form, x, e)
            assert torch.equal(_run(st, kind, form, x, e), full), f"{kind} {form}: two identical calls differ"
            rev = _run(st, kind, form, x.flip(0).contiguous(), e.flip(0))
            assert torch.equal(rev.flip(0), full), f"{kind} {form}: reversed order"
            for n in COUNTS[:-1]:
                assert torch.equal(_run(st, kind, form, x[:n], e[:n]), full[:n]), f"{kind} {form}: prefix of {n}"
            for nd in (1, 64, 65, 130):
                part = _run(st, kind, form, x, e, n_dev=nd)
                assert torch.equal(part[:nd], full[:nd]), f"{kind} {form}: n_dev = {nd}"


@pytest.mark.parametrize("name", ["w32", "odd_tiles"])
def test_more_than_one_tile_per_workgroup(name):
    """64 * 257 + 5 points are 258 tiles on 256 workgroups: two of them run a second tile (what a workgroup keeps across
    the tiles of its loop must not reach the second one); the same points as two launches of at most 256 tiles"""
    from hashmodnffbanks_idr_amd import ops
    st = _state(name)
    n, cut = 64 * 257 + 5, 64 * 256
    x = torch.from_numpy(P.make_points(1043, n, -1.05, 1.05)).cuda()
    desc, table, B, frac = st["grid"]
    with torch.no_grad():
        e = _strided(ops.encode_fwd(desc, x, table, B, frac))
    for kind in KINDS:
        for form in FORMS:
            one = _run(st, kind, form, x, e)
            two = torch.cat([_run(st, kind, form, x[:cut], e[:cut]), _run(st, kind, form, x[cut:], e[cut:])])
            assert torch.isfinite(one).all()
            assert torch.equal(one, two), f"{kind} {form}: {int((one != two).sum())} points differ"


COUNTS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "guard_refined_counts.json")


@pytest.mark.parametrize("head", [0, 16])
@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("tag", ["init", "bumpy", "C2"])
def test_guard_select_kernels(golden, tag, mode, head):
    """the wave-per-row select kernels mark what the serial walk over a row marked: the guarded call equals the unguarded
    one bit for bit, and it refines as many samples as the recorded build did (tests/golden/guard_refined_counts.json)"""
    import test_guard_gpu as G
    recorded = json.load(open(COUNTS_FILE))["guard_refined"]
    g, net = G._fixture(golden, tag)
    rays = G._rays(g)
    on = G._call(G._tracer(g, mode, head), net, rays, True)
    off = G._call(G._tracer(g, mode, head), net, rays, False)
    G._assert_same(on, off, f"{tag} {mode} head {head}")
    st = on[1]
    print(f"{tag} {mode} head {head}: refined {st['guard_refined']} (recorded {recorded[f'{tag} {mode} head {head}']}), max dev "
          f"{st['guard_max_dev']:.3e}")
    assert st["guard_refined"] == recorded[f"{tag} {mode} head {head}"]
    assert not st["guard_tripped"] and st["guard_max_dev"] <= G.TAU_TRIP
