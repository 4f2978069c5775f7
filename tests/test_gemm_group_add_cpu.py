"""ops._group_tn_takes (which problems ops.gemm_group_tn_add hands to the library WITH their addends) against the library's
own rule: hm_gemm_f32_group_tn_add_det_workspace_bytes walks the items on the host only and returns -1 for an addend on
a problem the grouped kernel does not take.  If the two disagreed, such a call would fail instead of falling back."""
import ctypes

import pytest

CASES = [(K, ld) for K in (64, 80, 128, 130, 256, 1536, 4096, 6144) for ld in (64, 67, 512)] + \
        [(128, 2 ** 22 - 1), (128, 2 ** 22), (1024, 2 ** 19 - 1), (1024, 2 ** 19), (1 << 20, 512), (1 << 20, 511)]


@pytest.mark.parametrize("wide", ["a", "b"])
@pytest.mark.parametrize("K,ld", CASES)
def test_python_rule_is_the_librarys(K, ld, wide):
    from hashmodnffbanks_idr_amd import _lib, ops
    lda, ldb = (ld, 64) if wide == "a" else (64, ld)
    a, b, c = 0x7f0000100000, 0x7f4000100000, 0x7f8000100000
    item = (_lib.GemmGroupAddItem * 1)()
    # an addend of one k-group on A, with a small leading dimension of its own
    item[0] = _lib.GemmGroupAddItem(a, b, c, 64, 64, K, lda, ldb, 64, a, 0, 64, 0, 8, 12, 0, 0)
    need = _lib.lib().hm_gemm_f32_group_tn_add_det_workspace_bytes(ctypes.cast(item, ctypes.c_void_p), 1)
    assert (need >= 0) == ops._group_tn_takes(K, lda, ldb), (K, lda, ldb, need)
