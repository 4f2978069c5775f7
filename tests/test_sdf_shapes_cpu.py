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


def test_fp32_lds_boundary_at_512_wide_layers(lib):
    """E = 111 (L = 27) is the widest hash-grid embedding the 64-point tile holds next to 512-wide layers"""
    import ctypes
    base = S.BY_NAME["L27"]
    for L, E, want in ((27, 111, 1), (28, 115, 0)):
        c = base._replace(L=L)
        assert S.emb_width(c) == E
        assert lib.hm_sdf_net_fits(ctypes.byref(S.descriptor(c)), E, 0) == want
    assert b"160 KB" in lib.hm_last_error()
