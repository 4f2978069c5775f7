"""The 16-, 8- and 4-point SDF tile bodies (csrc/hm_sdf.hip: sdf_small_body) outside their matrix loops: the encode on all
threads straight from the points, the bias hand-off through LDS, ragged tiles, waves without a feature tile, a partly
filled wave, a workgroup that runs more than one tile.

(a) Every launch of tests/small_tile_cases.py returns, bit for bit, what the build of the commit BEFORE these stages were
    rewritten returned (tests/golden/small_tile_bits.npz, recorded from that build by scripts/small_bits_ab.py).
(b) A point's value does not depend on its position in the tile, on the tile's live count or on the workgroup that
    evaluates it."""
import os

import numpy as np
import pytest
import torch

import small_tile_cases as T

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small_tile_bits.npz")


@pytest.fixture(scope="module")
def recorded():
    return np.load(GOLDEN)


@pytest.mark.parametrize("tile", T.TILES)
@pytest.mark.parametrize("name", ["w64", "w160", "c2"])
def test_bits_of_the_build_before(recorded, name, tile):
    mine = [l for l in T.launches() if l[1] == name and l[4] == tile]
    assert mine and all(l[0] in recorded.files for l in mine)
    bad = []
    for key, _, form, n, _, sdf_only in mine:
        got = T.run(name, form, T.points(n), tile, sdf_only).cpu().numpy()
        assert np.isfinite(got).all(), key
        if not T.same_bits(got, recorded[key]):
            bad.append((key, float(np.abs(got.astype(np.float64) - recorded[key]).max())))
    assert not bad, f"{len(bad)} of {len(mine)} launches moved: {bad[:5]}"


@pytest.mark.parametrize("tile", T.TILES)
@pytest.mark.parametrize("form", T.FORMS)
@pytest.mark.parametrize("name", ["w64", "w160"])
def test_value_is_the_points_alone(recorded, name, form, tile):
    """33 points: as one launch (9 / 5 / 3 tiles, the last one ragged); on two and on one workgroup, whose tile loops run
    more than once; each point alone (cnt = 1, slot 0); shifted by one and reversed, which moves every point to another
    slot, tile and workgroup.  All of them give the recorded 33-point values."""
    for sdf_only in (True, False):
        x = T.points(33)
        want = torch.from_numpy(recorded[f"{name}/t{tile}/{form}/n33/{'sdf' if sdf_only else 'all'}"]).cuda()
        assert torch.equal(T.run(name, form, x, tile, sdf_only), want)
        for wgs in (2, 1):
            assert torch.equal(T.run(name, form, x, tile, sdf_only, max_workgroups=wgs), want), f"{wgs} workgroups"
        assert torch.equal(T.run(name, form, x[1:].contiguous(), tile, sdf_only), want[1:]), "shifted by one"
        assert torch.equal(T.run(name, form, x.flip(0).contiguous(), tile, sdf_only), want.flip(0)), "reversed"
        for i in (0, 5, 32):
            assert torch.equal(T.run(name, form, x[i:i + 1].contiguous(), tile, sdf_only), want[i:i + 1]), f"point {i} alone"
