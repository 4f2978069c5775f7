"""The encoder case table (tests/encode_cases.py) is what it claims to be - checked with the C oracle and numpy alone,
no GPU: table sizes on the intended side of the dispatch thresholds, the exactness condition of the integer inputs,
order independence of the oracle's scatter on them, the oracle's own adjoint identity, the float64 torch restatement
against the oracle on voxel faces, and the content of the lattice point set."""
import numpy as np
import pytest
import torch

import encode_cases as EC
from oracle import c_oracle as O

ALL = tuple(EC.CASES)
MODES = tuple(EC.MODES)


def test_table_sizes_are_on_the_intended_side():
    for name in ALL:
        g = EC.grid(name)
        assert 1 <= g.L <= 32 and 1 <= g.F <= 8, name
        if name in EC.Z_CASES:
            # big-launch kernels: F = 2, table above 8 MiB (9.4 ... 16 MiB), output tile within the 160 KB of LDS
            assert g.F == 2 and EC.BIG_TABLE_BYTES + 2 ** 20 < g.table_bytes <= 16 * 2 ** 20, (name, g.table_bytes)
            assert 4 * (256 * ((g.E + 3) & ~3) + 256 * 3 + 256) <= 160 * 1024, name
            assert EC.N_BIG >= 131072 > EC.N_BELOW
        else:
            assert g.table_bytes < EC.BIG_TABLE_BYTES // 8, (name, g.table_bytes)
        if name in EC.SMALL_SCATTER:
            assert g.total_rows <= EC.SMALL_TABLE_ROWS and g.table_bytes <= EC.SMALL_TABLE_LDS, name
        if name in EC.ATOMIC_SCATTER:
            assert g.total_rows > EC.SMALL_TABLE_ROWS or g.table_bytes > EC.SMALL_TABLE_LDS, name
        assert (g.F != 2) == (name in EC.FN_CASES), name
    assert EC.grid("S_F3_edge").table_bytes == EC.SMALL_TABLE_LDS                     # exactly 48 KiB
    assert EC.grid("S_F4_over").total_rows == EC.grid("S_F3_edge").total_rows == 4096
    assert EC.grid("S_F4_over").table_bytes == 64 * 1024
    # what each z case is listed for
    assert EC.grid("Z1").L == 1 and EC.grid("Z3").L == 3 and EC.grid("Z15").L == 15
    assert EC.grid("Z17").L * 2 == 34 and EC.grid("Z32").L == 32 and EC.grid("Z32").E == 131
    assert int(EC.grid("Z15").res.max()) == 2048
    z3 = EC.grid("Z3")
    assert int(z3.rows[1]) == 90 ** 3 and z3.rows[1] & (z3.rows[1] - 1) != 0
    s1 = EC.grid("S_F1")
    assert int(s1.rows[1]) < 16 ** 3 and s1.rows[1] & (s1.rows[1] - 1) != 0      # hashed AND not a power of two
    s3 = EC.grid("S_F3")
    assert int(s3.res[0]) == 1 and int(s3.rows[0]) == 1
    # small-table scatter: n * L * C >= 4096 selects it at the largest n of the case in both modes, n = 1 and 7 stay
    # below it and take the atomic kernel on the same table
    for name in EC.FN_CASES:
        sizes = EC.fn_sizes(name)
        for mode in MODES:
            taken = [EC.small_scatter_taken(name, n, mode) for n in sizes]
            assert taken[:2] == [False, False], (name, mode)
            assert taken[-1] == (name in EC.SMALL_SCATTER), (name, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ALL)
def test_exact_inputs_condition_and_order_independence(name, mode):
    """the scatter of |d_feat| stays below 2^12 (trilinear; 2^24 in reference mode) in every cell, every value of the
    oracle's scatter is a multiple of 2^-12, and a permutation of the points leaves it bit-identical.  (A point's
    weights sum to 1 on every level, so a cell holds at most n * max|d_feat|: the bound can only be missed at
    n >= 4096, the sizes checked here.)"""
    for n in sorted({EC.default_n(name), max(EC.fn_sizes(name))}):
        _check_exact(name, mode, n)


def _check_exact(name, mode, n):
    x, d = EC.points(name, "lattice", n), EC.d_feat(name, "lattice", n, mode)
    mag = EC.scatter(name, x, np.abs(d), mode)
    print(f"{name}/{mode}: largest cell of scatter(|d_feat|) {mag.max():.0f} (bound {EC.exact_bound(mode):.0f})")
    assert mag.max() < EC.exact_bound(mode)
    ref = EC.oracle_scatter(name, "lattice", n, mode)
    assert np.array_equal(ref * 4096.0, np.round(ref * 4096.0))
    perm = np.random.RandomState(5).permutation(n)
    assert np.array_equal(EC.scatter(name, x[perm], d[perm], mode), ref)
    assert np.array_equal(EC.scatter(name, x[::-1], d[::-1], mode), ref)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ALL)
def test_exact_forward_is_a_multiple_of_2_pow_minus_12(name, mode):
    """integer tables in [-8, 8] on lattice points: |feature| <= 8 and a multiple of 2^-12 (exactly representable)"""
    g = EC.grid(name)
    ref = EC.oracle_fwd(name, "lattice", EC.N_SMALL, mode)[:, 3 + 2 * g.L:]
    assert np.abs(ref).max() <= 8.0 and np.abs(ref).max() > 0
    assert np.array_equal(ref * 4096.0, np.round(ref * 4096.0))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ALL)
def test_oracle_adjoint_identity_on_real_inputs(name, mode):
    """<d_feat, gather(T)> == <scatter(d_feat), T> with float64 sums of the oracle's fp32 results - the bound of
    test_encode_gpu.py::test_encode_bwd_table_small_table_path (1e-6 of the summed magnitudes)"""
    g = EC.grid(name)
    n = EC.N_SMALL
    feats = EC.oracle_fwd(name, "real", n, mode)[:, 3 + 2 * g.L:].astype(np.float64)
    d = EC.d_feat(name, "real", n, mode).astype(np.float64)
    sc = EC.oracle_scatter(name, "real", n, mode).astype(np.float64)
    lhs, rhs = (feats * d).sum(), (EC.table(name, False).astype(np.float64) * sc).sum()
    mag = (np.abs(feats) * np.abs(d)).sum()
    assert abs(lhs - rhs) <= 1e-6 * mag, (lhs, rhs, mag)


@pytest.mark.parametrize("name", ALL)
def test_trilinear_torch_agrees_with_the_oracle_on_faces(name):
    """same floor convention on voxel faces: with the integer table both are exact on lattice points, so the float64
    restatement equals the oracle's fp32 rows bit for bit"""
    g = EC.grid(name)
    n = EC.N_SMALL
    x = torch.from_numpy(EC.points(name, "lattice", n).copy())
    got = EC._trilinear_torch(x, torch.from_numpy(EC.table(name, True).copy()), g)
    ref = EC.oracle_fwd(name, "lattice", n, "trilinear")[:, 3 + 2 * g.L:]
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), ref.astype(np.float64))


@pytest.mark.parametrize("name", ALL)
def test_lattice_has_faces_nodes_negative_cells_and_outside_points(name):
    g = EC.grid(name)
    x = EC.points(name, "lattice", EC.default_n(name)).astype(np.float64)
    assert np.array_equal(x * 16, np.round(x * 16)) and np.abs(x).max() <= 21 / 16
    assert (x < 0).any() and (np.abs(x) > 1).any(1).any() and (np.abs(x) <= 1).all(1).any()
    for r in g.res:
        xs = x * float(r)
        assert float(np.abs(xs).max()) < 2 ** 24                     # x * res is exact in fp32
        on_face = xs == np.floor(xs)
        assert on_face.any(1).sum() >= 16 and on_face.all(1).sum() >= 5, (name, r)      # faces, nodes
        assert (~on_face).all(1).any() or r % 16 == 0, (name, r)                        # and interior points
        assert (np.floor(xs) < 0).any()


def test_real_points_carry_the_fixed_rows():
    for name in ("Z3", "S_F3", "G_F8"):
        n = EC.default_n(name)
        x = EC.points(name, "real", n)
        assert np.array_equal(x[7], (1.0, -1.0, 1.0)) and np.array_equal(x[8], (-1.0, 1.0, -1.0))
        if n >= 5000:
            assert np.array_equal(x[3009:5000], x[9:2000])           # (rows 7 and 8 are set afterwards)
        import params as P
        adv = P.adversarial_points([int(r) for r in EC.grid(name).res])
        assert np.array_equal(x[n - len(adv):], adv)
    for n in (1, 7, 63, 65):
        assert EC.points("G_F4", "real", n).shape == (n, 3) and EC.points("G_F4", "lattice", n).shape == (n, 3)


def test_oracle_accepts_the_hand_made_grid():
    """the Grid of encode_cases gives the oracle the same level table as c_oracle.Grid where both exist"""
    import params as P
    a = O.Grid(5, 12, 4, 64, F=4)
    b = EC.grid("G_F4")
    for k in ("L", "F", "total_rows", "E"):
        assert getattr(a, k) == getattr(b, k)
    for k in ("res", "rows", "row_off"):
        assert np.array_equal(getattr(a, k), getattr(b, k)) and getattr(a, k).dtype == getattr(b, k).dtype
    assert EC.CASES["Z15"][:2] == P.level_table(15, 17, 16, 2048)
