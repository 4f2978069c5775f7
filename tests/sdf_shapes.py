"""The SDF network shape table shared by tests/test_sdf_shapes_cpu.py (the kernel paths each case reaches, recomputed from
the table, and the host-side acceptance of every kernel family, asked on CPU through hm_sdf_net_fits) and
tests/test_sdf_shapes_gpu.py (the same cases run on the device against float64).

A case is an ImplicitNetwork shape: hash levels L (embedding width E = 3 + 4L), the `dims` list of the constructor
(a layer that feeds a skip gets dims[l + 1] - E outputs), skip_in and the feature vector size.  fp32 / bf16 / split: whether
hm_sdf_fwd, hm_sdf_fwd_bf16 and hm_sdf_fwd_split accept the network; the CPU test asserts the library agrees."""
import ctypes
from collections import namedtuple

import params as P

Case = namedtuple("Case", "name L T hidden skip fvs fp32 bf16 split what")


def _case(name, L, hidden, skip, fvs, what, T=12, fp32=True, bf16=True, split=True):
    return Case(name, L, T, tuple(hidden), tuple(skip), fvs, fp32, bf16, split, what)


CASES = [
    _case("c2", 16, (512,) * 8, (4,), 256, "the benchmarked network: 16 tiles per layer, E = 67", T=19),
    _case("w32", 4, (32,) * 8, (4,), 31, "every layer one 32-row tile (n_tiles = 1): seven idle waves"),
    _case("odd_tiles", 8, (96, 160, 224, 96, 160, 224, 96, 160), (4,), 64,
          "3, 5 and 7 tiles: the last busy wave of the 64-point body owns ONE 32-row tile"),
    _case("ragged", 16, (512, 100, 33, 448, 250, 511, 64, 129), (4,), 256,
          "hidden out_dim 33, 129, 381, 511: no multiple of 4, k tails inside every octet / 16-block"),
    _case("depth0", 4, (), (), 8, "one linear layer (E -> 9): the embedding straight into the output layer",
          bf16=False, split=False),
    _case("depth1", 6, (128,), (), 16, "one hidden layer: the 16-bit kernels' minimum"),
    _case("depth15", 4, (64,) * 15, (8,), 15, "16 linear layers (HM_MAX_LAYERS) at width 64"),
    _case("skip1", 8, (256,) * 6, (1,), 32, "skip at layer 1: layer 0 feeds the concat"),
    _case("skip_last", 6, (192,) * 5, (5,), 40, "skip at the last linear layer: it reads cat[h, e] / sqrt2",
          bf16=False, split=False),
    _case("skip_2_5", 8, (256,) * 8, (2, 5), 64, "two skips: the embedding is read twice"),
    _case("skip_3_4", 8, (256,) * 8, (3, 4), 64, "adjacent skips: a skip layer feeds the next concat"),
    _case("no_skip", 8, (128,) * 8, (), 100, "no skip connection"),
    _case("fvs0", 8, (256,) * 4, (2,), 0, "fvs = 0: output width 1"),
    _case("fvs511", 8, (512,) * 4, (2,), 511, "fvs = 511: a 512-wide output layer"),
    _case("L2", 2, (512,) * 8, (4,), 256, "L = 2 (E = 11): one embedding octet plus a tail"),
    _case("L27", 27, (512,) * 8, (4,), 256, "L = 27 (E = 111): the widest embedding the 64-point tile holds at 512"),
    _case("L28", 28, (512,) * 8, (4,), 256, "L = 28 (E = 115): over the 160 KB tile, the module falls back",
          fp32=False, split=False),
]
BY_NAME = {c.name: c for c in CASES}


def emb_width(case):
    return 3 + 4 * case.L


def grid_config(case):
    """(L, T, base, desired) for params.make_embedder_state / ImplicitNetwork"""
    return (case.L, case.T, 16, 512)


def layer_shapes(case):
    """per linear layer: (in features, out features) as ImplicitNetwork builds them"""
    return P.sdf_dims(emb_width(case), case.hidden, 1 + case.fvs, case.skip)


def layers(case):
    """per linear layer: dict(out, n_tiles, segs=[(src, width)], post_div_sqrt2, last) in the layout PackedSdf packs
    (include/hashmod.h: segment 0 = previous layer (src 0) or the embedding (src 1), the skip layer's second segment = the
    embedding)"""
    E = emb_width(case)
    shapes = layer_shapes(case)
    out = []
    for l, (din, dout) in enumerate(shapes):
        if l == 0:
            segs = [(1, E)]
        elif l in case.skip:
            segs = [(0, shapes[l - 1][1]), (1, E)]
        else:
            segs = [(0, shapes[l - 1][1])]
        assert sum(w for _, w in segs) == din
        out.append(dict(out=dout, n_tiles=(dout + 31) // 32, segs=segs, post_div_sqrt2=int((l + 1) in case.skip),
                        last=l == len(shapes) - 1))
    return out


def wave_shares64(n_tiles):
    """32-row feature tiles each of the 8 waves of the 64-point body owns (sdf64_run: t0 = 2 wave)"""
    return [max(0, min(2, n_tiles - 2 * w)) for w in range(8)]


def wave_shares16(n_tiles):
    """16-row feature tiles each of the 8 waves of the 16- / 8- / 4-point bodies owns (sdf_small_body: u0 = 4 wave over
    2 n_tiles tiles)"""
    return [max(0, min(4, 2 * n_tiles - 4 * w)) for w in range(8)]


def descriptor(case, with_bf16=True, split_kind=0):
    """hm_mlp_desc of the case with placeholder image pointers: what hm_sdf_net_fits reads is the shape (it never
    dereferences a pointer).  split_kind: HM_SPLIT_BF16X2 (0) / HM_SPLIT_F16X2 (1), or -1 for no split image."""
    from hashmodnffbanks_idr_amd import _lib
    d = _lib.MlpDesc()
    ly = layers(case)
    d.n_layers = len(ly)
    d.beta = 0.1
    d.split_kind = split_kind
    fake = ctypes.c_void_p(256).value
    for l, L in enumerate(ly):
        x = d.layer[l]
        x.w_packed, x.bias, x.w_packed_m16 = fake, fake, fake
        x.w_packed_bf16 = fake if with_bf16 else None
        x.w_packed_split = fake if split_kind >= 0 else None
        x.out_dim, x.n_tiles = L["out"], L["n_tiles"]
        segs = L["segs"] + [(0, 0)] * (2 - len(L["segs"]))
        for s, (src, w) in enumerate(segs):
            x.seg_src[s] = src
            x.seg_octets[s] = (w + 7) // 8
            x.seg_blocks16[s] = (w + 15) // 16
        x.activation = 0 if L["last"] else 1
        x.post_div_sqrt2 = L["post_div_sqrt2"]
    return d
