"""Host side of the brick-sparse marching cubes (csrc/hm_mesh_sparse.hip): every entry point rejects bad arguments with
a status before it launches anything, and the brick-grid helpers of ops.marching_cubes_sparse."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def L():
    from hashmodnffbanks_idr_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def _lattice(nx=16, ny=16, nz=16, n_slots=4, map_ptr=256, pool_ptr=256):
    from hashmodnffbanks_idr_amd import _lib
    return ctypes.byref(_lib.McsLattice(nx, ny, nz, n_slots, map_ptr, pool_ptr))


def test_abi_rejects_bad_arguments_with_a_status(L):
    from hashmodnffbanks_idr_amd import _lib
    fake = ctypes.c_void_p(256)

    def rejected(rc, word):
        assert rc == -1 and word in L.hm_last_error(), L.hm_last_error()

    rejected(L.hm_mcs_points_bricks(fake, 1, fake, fake, fake, 1, 4, 4, None, fake, None), b">= 2")
    rejected(L.hm_mcs_points_bricks(fake, 1, fake, fake, fake, 4, 65537, 4, None, fake, None), b"<= 65536")
    rejected(L.hm_mcs_points_bricks(fake, 1, fake, None, fake, 4, 4, 4, None, fake, None), b"NULL axis")
    rejected(L.hm_mcs_points_bricks(fake, (1 << 22) + 1, fake, fake, fake, 4, 4, 4, None, fake, None), b"n_bricks")
    rejected(L.hm_mcs_points_bricks(None, 1, fake, fake, fake, 4, 4, 4, None, fake, None), b"brick list is NULL")
    rejected(L.hm_mcs_points_index(fake, 1 << 31, fake, fake, fake, 4, 4, 4, None, fake, None), b"2^31")
    rejected(L.hm_mcs_points_index(fake, 8, fake, fake, fake, 4, 4, 4, None, None, None), b"NULL output")
    assert L.hm_mcs_points_index(None, 0, fake, fake, fake, 4, 4, 4, None, None, None) == 0    # nothing to do

    st = ctypes.c_void_p(512)
    rejected(L.hm_mcs_status(fake, 1, None, 0.0, st, None), b"lattice is NULL")
    rejected(L.hm_mcs_status(fake, 1, _lattice(nx=1), 0.0, st, None), b">= 2")
    rejected(L.hm_mcs_status(fake, 1, _lattice(map_ptr=None), 0.0, st, None), b"brick map is NULL")
    rejected(L.hm_mcs_status(fake, 1, _lattice(pool_ptr=None), 0.0, st, None), b"value pool is NULL")
    rejected(L.hm_mcs_status(fake, 1, _lattice(n_slots=-1), 0.0, st, None), b"n_slots")
    rejected(L.hm_mcs_status(fake, 1, _lattice(), float("nan"), st, None), b"level is NaN")
    rejected(L.hm_mcs_status(fake, 1, _lattice(), 0.0, None, None), b"NULL status")

    assert L.hm_mcs_workspace_bytes(0) == -1 and b"n_bricks" in L.hm_last_error()
    assert L.hm_mcs_workspace_bytes((1 << 22) + 1) == -1
    assert 6 * 512 * 10 <= L.hm_mcs_workspace_bytes(10) <= 8 * 512 * 10
    cnt = ctypes.c_void_p(512)
    rejected(L.hm_mcs_count(fake, 0, _lattice(), 0.0, fake, 1 << 20, cnt, None), b"empty brick list")
    rejected(L.hm_mcs_count(fake, 10, _lattice(), 0.0, fake, 16, cnt, None), b"workspace too small")
    rejected(L.hm_mcs_count(fake, 10, _lattice(), 0.0, fake, 1 << 20, None, None), b"NULL workspace or counts")
    sp = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    rejected(L.hm_mcs_emit(fake, 10, _lattice(), None, 0.0, sp, fake, 1 << 20, 5, 5, fake, fake, fake, fake, fake, None),
             b"list_pos")
    rejected(L.hm_mcs_emit(fake, 10, _lattice(), fake, 0.0, sp, fake, 1 << 20, 5, 5, fake, fake, fake, None, fake, None),
             b"vert_keys")
    rc = L.hm_mcs_emit(fake, 10, _lattice(), fake, 0.0, sp, fake, 1 << 20, 1 << 31, 10, fake, fake, fake, fake, fake,
                       None)
    rejected(rc, b"int32")
    with pytest.raises(ValueError, match="int32"):        # the error of hm_mc_emit
        _lib.check(rc)


def test_brick_grid_helpers():
    from hashmodnffbanks_idr_amd import ops
    g = torch.zeros(4, 3, 1, dtype=torch.bool)
    g[1, 1, 0] = True
    up = ops._grow(g, 0, 1)                     # the brick and its upper neighbours
    assert up.nonzero().tolist() == [[1, 1, 0], [1, 2, 0], [2, 1, 0], [2, 2, 0]]
    both = ops._grow(g, 1, 1)                   # its 27-neighbourhood, clipped to the grid
    assert int(both.sum()) == 9 and bool(both[0:3, 0:3, 0].all())
    assert g.sum() == 1                         # the argument is left alone
    assert ops._listed(both, 9).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8] and ops._listed(both, 9).dtype == torch.int32
