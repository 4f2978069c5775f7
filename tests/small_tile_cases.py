"""The launches of the 16-, 8- and 4-point SDF tile bodies (csrc/hm_sdf.hip: sdf_small_body) shared by
tests/test_small_tile_round_gpu.py and scripts/small_bits_ab.py, which records them from another build of the library.

Networks (hash grid L = 8, so E = 35 fits under a 64-wide layer that feeds the skip):
  w64   the C2 layout (8 hidden layers, skip at 4) at width 64: four 16-row tiles, all wave 0's - waves 1..7 own none
  w160  width 160: ten 16-row tiles, wave 2 owns two of its four; the layer in front of the skip has 125 outputs
  c2    the benchmarked network, once, at 17 points
Each launch: hm_sdf_fwd in both frac modes and hm_sdf_fwd_emb on the embedding rows, sdf-only and all columns."""
import numpy as np
import torch

import params as P
import sdf_shapes as S
from helpers import make_implicit

TILES = (4, 8, 16)
COUNTS = (1, 3, 4, 5, 8, 9, 15, 16, 17, 33)     # ragged last tiles of every body
NETS = {
    "w64": S.Case("w64", 8, 19, (64,) * 8, (4,), 7, True, True, True, "waves 1..7 without a feature tile"),
    "w160": S.Case("w160", 8, 19, (160,) * 8, (4,), 7, True, True, True, "a partly filled wave"),
    "c2": S.BY_NAME["c2"],
}
FORMS = ("reference", "trilinear", "emb")

_BUILT = {}


def net(name):
    if name not in _BUILT:
        c = NETS[name]
        _BUILT[name] = make_implicit(S.grid_config(c), c.hidden, c.fvs, 11, 0.3, 0.3, skip_in=c.skip).eval()
    return _BUILT[name]


def points(n, seed=0):
    return torch.from_numpy(P.make_points(4100 + seed, n, -1.05, 1.05)).cuda()


def run(name, form, x, tile, sdf_only, max_workgroups=0):
    """one launch on the points x -> [n] or [n, out_dim]"""
    from hashmodnffbanks_idr_amd import ops
    m = net(name)
    emb = m._hash_embedder()
    desc, table, B = emb.desc, emb.table.detach(), emb.freq_encoding.B
    pk = m.packed_weights()
    with torch.no_grad():
        if form == "emb":
            e = ops.encode_fwd(desc, x, table, B, ops.FRAC_MODES[emb.frac_mode])
            return ops.sdf_fwd_emb(pk, e, sdf_only=sdf_only, tile_points=tile, max_workgroups=max_workgroups)
        return ops.sdf_fwd(desc, pk, x, table, B, 0 if form == "reference" else 1, sdf_only=sdf_only, tile_points=tile,
                           max_workgroups=max_workgroups)


def launches():
    """(key, network, form, n, tile, sdf_only) of every recorded launch"""
    for name in ("w64", "w160"):
        for tile in TILES:
            for form in FORMS:
                for n in COUNTS:
                    for sdf_only in (True, False):
                        yield f"{name}/t{tile}/{form}/n{n}/{'sdf' if sdf_only else 'all'}", name, form, n, tile, sdf_only
    for tile in TILES:
        for sdf_only in (True, False):
            yield f"c2/t{tile}/reference/n17/{'sdf' if sdf_only else 'all'}", "c2", "reference", 17, tile, sdf_only


def record():
    """{key: float32 array} of every launch, on the library that is loaded"""
    out = {}
    for key, name, form, n, tile, sdf_only in launches():
        out[key] = run(name, form, points(n), tile, sdf_only).cpu().numpy()
    torch.cuda.synchronize()
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
