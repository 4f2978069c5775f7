"""Quarter tiles of the 64-point fp32 SDF launch (hm_sdf_tile64.h: tiles of <= 16 points on v_mfma_f32_16x16x4_f32 that
present k to every accumulator in the order of the 64-point tile's 32x32x2 loop): the launch with quarter tiles enabled
(ops.TILE64_QUARTER) against the same launch without them (tile_points = 64), bit for bit.

The schedule rule reads the device-side count: n <= 16 G runs quarter tiles (G = the launch's grid, fixed here through
max_workgroups with the count in n_dev), everything else keeps the rule of the plain launch.  Point counts: 1, 15, 16, 17,
37, 16 G - 1, 16 G, 16 G + 1 and 32 G, on the C2 golden network, a network with a skip layer, odd tile counts (a wave that
owns ONE feature tile) and an output width of 65, a narrow one (one tile per layer: seven waves without MFMA work) and
the one-layer network; both frac modes, embedding rows as input, sdf-only output and all output columns (the last layer
on the quarter tile's MFMA loop), and permutation equivariance of the flagged launch."""
import pytest
import torch

import params as P
import sdf_shapes as S
from helpers import make_implicit

pytestmark = pytest.mark.gpu

G = 5
COUNTS = (1, 15, 16, 17, 37, 16 * G - 1, 16 * G, 16 * G + 1, 32 * G)
CAP = 32 * G            # capacity of every launch: the host sizes the grid (G) from it, the kernel reads the count
NETS = ("C2", "odd_tiles", "w32", "depth0")

_CACHE = {}


def _net(name, golden):
    if name not in _CACHE:
        if name == "C2":
            g = golden("sdf_C2")
            net = make_implicit("C2", tuple(g["hidden"].tolist()), int(g["fvs"]), int(g["seed"]), float(g["perturb"]),
                                float(g["table_scale"]))
        else:
            case = S.BY_NAME[name]
            net = make_implicit(S.grid_config(case), case.hidden, case.fvs, 11, 0.3, 0.3, skip_in=case.skip)
        net.eval()
        x = torch.from_numpy(P.make_points(4100, CAP, -1.05, 1.05)).cuda()
        _CACHE[name] = (net, x)
    return _CACHE[name]


def _count(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def _fwd(net, x, n, tile, frac, sdf_only):
    """the first n of x's CAP rows (device-side count) on G workgroups; rows n.. of the result are never written"""
    from hashmodnffbanks_idr_amd import ops
    emb = net._hash_embedder()
    out = ops.sdf_fwd(emb.desc, net.packed_weights(), x, emb.table.detach(), emb.freq_encoding.B, frac,
                      sdf_only=sdf_only, max_workgroups=G, tile_points=tile, n_dev=_count(n))
    return out[:n]


def _fwd_emb(net, e, n, tile, sdf_only):
    from hashmodnffbanks_idr_amd import ops
    return ops.sdf_fwd_emb(net.packed_weights(), e, sdf_only=sdf_only, tile_points=tile, n_dev=_count(n),
                           max_workgroups=G)[:n]


@pytest.mark.parametrize("sdf_only", [True, False], ids=["sdf", "all"])
@pytest.mark.parametrize("frac", [0, 1], ids=["reference", "trilinear"])
@pytest.mark.parametrize("name", NETS)
def test_quarter_tiles_give_the_64_point_tiles_bits(golden, name, frac, sdf_only):
    from hashmodnffbanks_idr_amd import ops
    net, x = _net(name, golden)
    with torch.no_grad():
        for n in COUNTS:
            want = _fwd(net, x, n, 64, frac, sdf_only)
            got = _fwd(net, x, n, ops.TILE64_QUARTER, frac, sdf_only)
            assert torch.isfinite(want).all()
            assert torch.equal(got, want), f"{name} frac {frac} n {n}: {int((got != want).sum())} values differ"


@pytest.mark.parametrize("sdf_only", [True, False], ids=["sdf", "all"])
@pytest.mark.parametrize("name", NETS)
def test_quarter_tiles_on_embedding_rows(golden, name, sdf_only):
    """hm_sdf_fwd_emb (row stride E + 5, NaN in the gap) with the flag against without it, and against hm_sdf_fwd"""
    from hashmodnffbanks_idr_amd import ops
    net, x = _net(name, golden)
    emb = net._hash_embedder()
    frac = ops.FRAC_MODES[emb.frac_mode]
    with torch.no_grad():
        e = ops.encode_fwd(emb.desc, x, emb.table.detach(), emb.freq_encoding.B, frac)
        buf = torch.full((e.shape[0], e.shape[1] + 5), float("nan"), device=e.device)
        buf[:, :e.shape[1]] = e
        rows = buf[:, :e.shape[1]]
        for n in COUNTS:
            want = _fwd_emb(net, rows, n, 64, sdf_only)
            got = _fwd_emb(net, rows, n, ops.TILE64_QUARTER, sdf_only)
            assert torch.equal(got, want), f"{name} n {n}: embedding rows, {int((got != want).sum())} values differ"
            assert torch.equal(got, _fwd(net, x, n, ops.TILE64_QUARTER, frac, sdf_only)), f"{name} n {n}: rows vs points"


@pytest.mark.parametrize("name", NETS)
def test_quarter_tiles_permutation_equivariance(golden, name):
    """a point's value does not depend on the quarter tile or the lane it sits in, nor on its neighbours"""
    from hashmodnffbanks_idr_amd import ops
    net, x = _net(name, golden)
    n = 16 * G - 3
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).cuda()
    xp = x.clone()
    xp[:n] = x[:n][perm]
    with torch.no_grad():
        for sdf_only in (True, False):
            s = _fwd(net, x, n, ops.TILE64_QUARTER, 0, sdf_only)
            sp = _fwd(net, xp, n, ops.TILE64_QUARTER, 0, sdf_only)
            assert torch.equal(sp, s[perm])
            for k in (1, 7, 16):     # the same points k rows on: other tiles, other lanes
                xs = torch.cat([x[k:n], x[:k], x[n:]])
                assert torch.equal(_fwd(net, xs, n, ops.TILE64_QUARTER, 0, sdf_only)[: n - k], s[k:])
