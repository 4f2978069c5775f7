"""The split-operand 64-point tile (csrc/hm_sdf_split_tile.h) outside its matrix loops, bit for bit: a point's value does
not depend on the tile or the launch it sits in, the fused encode stage equals the encoder kernel in front of the
precomputed-embedding entry point, and the one-launch split weight image equals the per-layer launches'.  Every assertion
is torch.equal: the stages under test (wave-uniform encode slots, 8-byte feature rows, bias quads fetched ahead of the
k-loop - also by the waves of a narrow layer that own one tile or none -, the per-layer epilogue instance,
hm_pack_mlp_layers_split) re-order work, never arithmetic."""
import ctypes as C

import numpy as np
import pytest
import torch

import params as P
import sdf_shapes as S
from helpers import make_implicit

pytestmark = pytest.mark.gpu

NETS = ("w32", "odd_tiles", "ragged", "depth1", "skip1")      # skip layers: all but depth1; skip1's follows layer 0
KINDS = ("bf16x2", "f16x2")
FRACS = (0, 1)                                                # HM_FRAC_REFERENCE, HM_FRAC_TRILINEAR
N_BIG = 64 * 257 + 5        # 258 tiles on 256 workgroups: workgroups 0 and 1 run a second tile, the last tile holds 5 points

_NETS, _RAW = {}, {}


def _net(name):
    if name not in _NETS:
        case = S.BY_NAME[name]
        _NETS[name] = make_implicit(S.grid_config(case), case.hidden, case.fvs, 11, 0.3, 0.3, skip_in=case.skip)
        _NETS[name].eval()
    return _NETS[name]


def _grid_and_weights(name, kind):
    """(desc, table, B, packed weights) of a table case, F = 2"""
    net = _net(name)
    emb = net._hash_embedder()
    net.coarse_split = kind
    with torch.no_grad():
        pk = net.packed_weights()
    assert pk.split == kind
    return emb.desc, emb.table.detach(), emb.freq_encoding.B, pk


def _raw(F, kind):
    """a network on a grid with F features per level, built on ops alone (the model's embedder has F = 2): L = 5 levels,
    two hidden layers of 96 and 64, the second one a skip layer"""
    from hashmodnffbanks_idr_amd import ops
    if (F, kind) not in _RAW:
        L, skip, hidden = 5, (1,), (96, 64)
        res, rows = P.level_table(L, 10, 16, 512)
        desc = ops.GridDesc(res, rows, n_features=F)
        table = torch.from_numpy(P.make_table(31, int(sum(rows)), F, 0.3)).cuda()
        B = torch.from_numpy(P.make_fourier_B(32, L, P.fourier_sigma(16, 512))).cuda()
        rs = np.random.RandomState(33)
        Ws, bs = [], []
        for din, dout in P.sdf_dims(desc.E, hidden, 9, skip):
            Ws.append(torch.from_numpy(rs.normal(0.0, np.sqrt(2.0 / dout), (dout, din)).astype(np.float32)).cuda())
            bs.append(torch.from_numpy(rs.normal(0.0, 0.05, (dout,)).astype(np.float32)).cuda())
        _RAW[(F, kind)] = (desc, table, B, ops.PackedSdf(Ws, bs, desc.E, skip, 0.1, split=kind))
    return _RAW[(F, kind)]


@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NETS)
def test_value_independent_of_tile_and_launch(name, kind, frac):
    from hashmodnffbanks_idr_amd import ops
    desc, table, B, pk = _grid_and_weights(name, kind)
    x = torch.from_numpy(P.make_points(501, N_BIG, -1.05, 1.05)).cuda()
    with torch.no_grad():
        full = ops.sdf_fwd_split(desc, pk, x, table, B, frac)
        assert torch.isfinite(full).all()
        for tile in (0, 256, 257):                  # a first tile, a workgroup's second tile, the ragged last tile
            sl = slice(64 * tile, min(64 * tile + 64, N_BIG))
            assert torch.equal(ops.sdf_fwd_split(desc, pk, x[sl], table, B, frac), full[sl]), tile
        for n in (1, 63, 64, 65):
            assert torch.equal(ops.sdf_fwd_split(desc, pk, x[:n], table, B, frac), full[:n]), n


def _edge_points(res_list, seed, n_random=300):
    """per axis: the grid lines k / res of every level (first, second, middle, last two), their negatives, +-1, just outside
    the cube, -0.0; the other two axes seeded random, plus points with all three axes on such values and random points"""
    vals = [1.0, -1.0, 1.0 + 2.0 ** -20, -1.0 - 2.0 ** -20, 1.05, -1.05, -0.0, 0.0]
    for r in res_list:
        for k in (0, 1, r // 2, r - 1, r):
            vals += [k / r, -k / r]
    vals = np.asarray(vals, np.float32)
    rs = np.random.RandomState(seed)
    pts = []
    for ax in range(3):
        p = rs.uniform(-1.0, 1.0, (len(vals), 3)).astype(np.float32)
        p[:, ax] = vals
        pts.append(p)
    pts.append(vals[rs.randint(0, len(vals), (len(vals), 3))])
    pts.append(rs.uniform(-1.05, 1.05, (n_random, 3)).astype(np.float32))
    return torch.from_numpy(np.concatenate(pts)).cuda()


def _fused_against_encoder(desc, table, B, pk, frac, fp32):
    from hashmodnffbanks_idr_amd import ops
    x = _edge_points(desc.res.tolist(), 7)
    assert bool((x == 0).any()) and bool(torch.signbit(x).logical_and(x == 0).any())       # -0.0 is in
    with torch.no_grad():
        e = ops.encode_fwd(desc, x, table, B, frac)
        assert torch.equal(ops.sdf_fwd_split(desc, pk, x, table, B, frac), ops.sdf_fwd_emb_split(pk, e))
        if fp32:
            assert torch.equal(ops.sdf_fwd(desc, pk, x, table, B, frac, sdf_only=True, tile_points=64),
                               ops.sdf_fwd_emb(pk, e, sdf_only=True, tile_points=64))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NETS)
def test_fused_encode_equals_encoder_f2(name, kind):
    """reference mode only: with F = 2 and trilinear weights the encoder kernels add the eight corners as a three-step
    lane butterfly (hm_encode.hip, dpp_sum8_pair) and the fused kernels in corner order, so the two entry points differ
    in the last bit there - before this tile was touched as after; scripts/split_bits_ab.py covers that mode build
    against build"""
    _fused_against_encoder(*_grid_and_weights(name, kind), 0, fp32=kind == "f16x2")


@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F", (1, 4))
def test_fused_encode_equals_encoder_other_f(F, kind, frac):
    _fused_against_encoder(*_raw(F, kind), frac, fp32=kind == "f16x2")


def _assert_one_launch_image_equals_per_layer(pk):
    from hashmodnffbanks_idr_amd import _lib
    for l, img in enumerate(pk.split_imgs):
        W = pk.keep[2 * l]
        out_dim, w0, w1 = pk.segs[l]
        s0, s1 = pk.split_scales[l]
        one = torch.full_like(img, 0x5a5a)
        _lib.check(_lib.lib().hm_pack_mlp_layer_split(_lib.dptr(W), W.stride(0), out_dim, w0, w1, s0, s1, pk.desc.split_kind,
                                                      _lib.dptr(one), _lib.stream_ptr(W)))
        assert torch.equal(one, img), l


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NETS + ("c2",))
def test_one_launch_split_image_equals_per_layer_launches(name, kind):
    pk = _grid_and_weights(name, kind)[3]
    assert any(s != (1.0, 1.0) for s in pk.split_scales) == bool(S.BY_NAME[name].skip)    # the skip layer's folded scale
    _assert_one_launch_image_equals_per_layer(pk)


@pytest.mark.parametrize("kind", KINDS)
def test_one_launch_split_image_other_f(kind):
    _assert_one_launch_image_equals_per_layer(_raw(4, kind)[3])


def test_split_pack_items_are_checked():
    from hashmodnffbanks_idr_amd import _lib
    items = (_lib.PackSplitItem * 1)()
    fn = _lib.lib().hm_pack_mlp_layers_split
    assert fn(C.cast(items, C.c_void_p), 1, 1, None) == -1            # NULL pointers
    assert fn(C.cast(items, C.c_void_p), 17, 1, None) == -1           # more than HM_MAX_LAYERS
    assert fn(C.cast(items, C.c_void_p), 1, 2, None) == -1            # no such kind
    assert fn(None, 0, 1, None) == 0
