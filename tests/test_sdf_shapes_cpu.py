"""The SDF shape table (tests/sdf_shapes.py) on CPU: the kernel paths its cases reach, recomputed from the table, so that an
edit of the table cannot quietly drop one, and the host-side acceptance of every fused kernel family
(hm_sdf_net_fits: the checks the launches make) for every case."""
import pytest

import sdf_shapes as S

HM_MAX_LAYERS = 16


@pytest.fixture(scope="module")
def lib():
    from hashmodnffbanks_idr_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _hidden(case):
    """the layers with an activation (every layer but the last)"""
    return [ly for ly in S.layers(case) if not ly["last"]]


def test_table_names_are_unique_and_shapes_are_valid():
    assert len(S.BY_NAME) == len(S.CASES)
    for c in S.CASES:
        assert 0 not in c.skip and all(1 <= s < len(S.layers(c)) for s in c.skip), c.name
        for ly in S.layers(c):
            assert 1 <= ly["out"] <= 512 and ly["n_tiles"] <= 16, (c.name, ly)
        assert len(S.layers(c)) <= HM_MAX_LAYERS
        assert c.what


def test_cases_cover_the_shape_dependent_paths():
    cov = set()
    for c in S.CASES:
        ly = S.layers(c)
        n = len(ly)
        E = S.emb_width(c)
        cov.add(("layers", n))
        for h in _hidden(c):
            cov.add(("hidden_tiles", h["n_tiles"]))
            cov |= {("share64", s) for s in S.wave_shares64(h["n_tiles"])}
            cov |= {("share16", s) for s in S.wave_shares16(h["n_tiles"])}
            for m in (4, 8, 16, 32):
                if h["out"] % m:
                    cov.add(("hidden_out_not_multiple_of", m))
            if not h["post_div_sqrt2"] and h["out"] % 4:
                cov.add("ragged_hidden_not_feeding_a_skip")
        if not c.skip:
            cov.add("no_skip")
        if 1 in c.skip:
            cov.add("skip_at_1")
        if n - 1 in c.skip:
            cov.add("skip_at_last")
        if len(c.skip) >= 2:
            cov.add("two_skips")
        if any(s + 1 in c.skip for s in c.skip):
            cov.add("adjacent_skips")
        cov.add(("out_width", ly[-1]["out"]))
        if E % 8 and E % 16:
            cov.add("emb_tail")
        cov.add(("E", E))
    need = {("layers", 1), ("layers", 2), ("layers", HM_MAX_LAYERS), ("hidden_tiles", 1), ("hidden_tiles", 16),
            ("share64", 0), ("share64", 1), ("share64", 2), ("share16", 0), ("share16", 2), ("share16", 4),
            ("hidden_out_not_multiple_of", 4), "ragged_hidden_not_feeding_a_skip", "no_skip", "skip_at_1",
            "skip_at_last", "two_skips", "adjacent_skips", ("out_width", 1), ("out_width", 512), "emb_tail",
            ("E", 11), ("E", 111), ("E", 115)}
    assert need <= cov, sorted(map(str, need - cov))
    # odd tile counts 3, 5, 7 in hidden layers
    odd = {h["n_tiles"] for c in S.CASES for h in _hidden(c)} & {3, 5, 7}
    assert odd == {3, 5, 7}
    # (16-row tiles come in pairs of one 32-row tile: a wave of the small bodies owns 0, 2 or 4 of them, never 1 or 3)
    assert all(s in (0, 2, 4) for c in S.CASES for h in _hidden(c) for s in S.wave_shares16(h["n_tiles"]))


def test_segment_lengths_follow_the_table():
    c = S.BY_NAME["skip_3_4"]
    d = S.descriptor(c)
    E = S.emb_width(c)
    ly = S.layers(c)
    assert [x["out"] for x in ly][2:5] == [256 - E, 256 - E, 256]
    assert (d.layer[3].seg_src[0], d.layer[3].seg_src[1]) == (0, 1)
    assert (d.layer[3].seg_octets[0], d.layer[3].seg_octets[1]) == ((256 - E + 7) // 8, (E + 7) // 8)
    assert (d.layer[4].seg_blocks16[0], d.layer[4].seg_blocks16[1]) == ((256 - E + 15) // 16, (E + 15) // 16)
    assert [d.layer[l].post_div_sqrt2 for l in range(5)] == [0, 0, 1, 1, 0]


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_kernel_families_accept_what_the_table_says(lib, case):
    """hm_sdf_net_fits runs each family's launch checks on the host: the table's fp32 / bf16 / split columns"""
    import ctypes
    from hashmodnffbanks_idr_amd import _lib
    E = S.emb_width(case)
    for family, want, kw in ((0, case.fp32, {}), (1, case.bf16, {}), (2, case.split, dict(split_kind=0)),
                             (2, case.split, dict(split_kind=1))):
        d = S.descriptor(case, **kw)
        got = lib.hm_sdf_net_fits(ctypes.byref(d), E, family)
        why = lib.hm_last_error()
        assert got == int(want), (case.name, family, got, why)
    # a descriptor without the family's image is refused (never launched on a NULL image)
    assert lib.hm_sdf_net_fits(ctypes.byref(S.descriptor(case, with_bf16=False)), E, 1) == 0
    assert lib.hm_sdf_net_fits(ctypes.byref(S.descriptor(case, split_kind=-1)), E, 2) == 0
    with pytest.raises(ValueError):
        _lib.check(lib.hm_sdf_net_fits(ctypes.byref(S.descriptor(case)), E, 3))


def _lds_regions(case, body):
    """[(name, bytes)] of the dynamic LDS regions of one tile body, in order: the formulas the launches used before the
    layout had one definition (sdf_lds64, sdf_lds16 and its 8-point half, sdf_bf16_net, sdf_split_net), written out here
    and NOT read back from the library"""
    E = S.emb_width(case)
    x_groups = 8 * max(ly["n_tiles"] for ly in S.layers(case))      # k-groups of 4 of the widest layer
    if body == "fp32_64":        # X [x_groups][64][4], EMB [2 ceil(E/8)][64][4], SX [64][4], RED [8][64], fp32
        return [("x", x_groups * 256 * 4), ("emb", (E + 7) // 8 * 2 * 256 * 4), ("sx", 64 * 4 * 4), ("red", 8 * 64 * 4)]
    if body in ("fp32_16", "fp32_8"):   # two images [x_groups][pts][4], EMB [4 ceil(E/16)][pts][4], SX [pts][4], RED [8][pts]
        pts = 16 if body == "fp32_16" else 8
        img = x_groups * pts * 4 * 4
        return [("x0", img), ("x1", img), ("emb", (E + 15) // 16 * 4 * pts * 4 * 4), ("sx", pts * 4 * 4), ("red", 8 * pts * 4)]
    if body == "bf16":           # X bf16 [x_groups/2][96][8], EMB fp32 [2 ceil(E/8)][96][4], SX [96][4], RED [5][96]
        return [("x", x_groups // 2 * 96 * 8 * 2), ("emb", (E + 7) // 8 * 2 * 96 * 4 * 4), ("sx", 96 * 4 * 4), ("red", 5 * 96 * 4)]
    assert body == "split"       # hi, lo planes [x_groups/2][64][8] and [2 ceil(E/16)][64][8] of 2 bytes, SX, RED [8][64]
    xp, ep = x_groups // 2 * 64 * 8 * 2, (E + 15) // 16 * 2 * 64 * 8 * 2
    return [("xh", xp), ("xl", xp), ("eh", ep), ("el", ep), ("sx", 64 * 4 * 4), ("red", 8 * 64 * 4)]


_LDS_BODIES = {"fp32_64": (0, 64), "fp32_16": (0, 16), "fp32_8": (0, 8), "bf16": (1, 0), "split": (2, 0)}


@pytest.mark.parametrize("body", sorted(_LDS_BODIES))
@pytest.mark.parametrize("name", ["c2", "odd_tiles", "ragged", "L2"])
def test_lds_layout_is_the_launch_size_and_ends_at_it(lib, name, body):
    """hm_diag_sdf_lds: every region of a body's layout starts where the one before it ends, the last one ends exactly at
    the byte count the launch asks for, and that count is the one the earlier host formulas gave"""
    import ctypes
    from hashmodnffbanks_idr_amd import _lib
    case = S.BY_NAME[name]
    family, tile_points = _LDS_BODIES[body]
    regions = (ctypes.c_int32 * 6)()
    _lib.check(lib.hm_diag_sdf_lds(ctypes.byref(S.descriptor(case)), S.emb_width(case), family, tile_points, regions))
    x1, emb, emb1, sx, red, total = list(regions)
    want = _lds_regions(case, body)
    # the library's offsets, one per expected region (bodies with one activation / embedding region report no second one)
    got = {"x": 0, "x0": 0, "xh": 0, "x1": x1, "xl": x1, "emb": emb, "eh": emb, "el": emb1, "sx": sx, "red": red}
    if body in ("fp32_64", "bf16"):
        assert x1 == 0
    if body != "split":
        assert emb1 == emb
    off = 0
    for region, nbytes in want:
        assert got[region] == off, (name, body, region, got[region], off)
        assert off % 16 == 0, (name, body, region)          # b128 LDS accesses need 16-byte aligned regions
        off += nbytes
    assert total == off, (name, body, total, off)
    if name == "c2":    # the benchmarked network, in plain numbers
        assert total == {"fp32_64": 152576, "fp32_16": 71424, "fp32_8": 35712, "bf16": 129408, "split": 154624}[body]


def test_fp32_lds_boundary_at_512_wide_layers(lib):
    """E = 111 (L = 27) is the widest hash-grid embedding the 64-point tile holds next to 512-wide layers"""
    import ctypes
    base = S.BY_NAME["L27"]
    for L, E, want in ((27, 111, 1), (28, 115, 0)):
        c = base._replace(L=L)
        assert S.emb_width(c) == E
        assert lib.hm_sdf_net_fits(ctypes.byref(S.descriptor(c)), E, 0) == want
    assert b"160 KB" in lib.hm_last_error()
