"""CPU-only checks of the sparse MERGE entries: declarations and binding, the scratch formula, size refusals."""
from __future__ import annotations

import ctypes as C

NEW = ["stg_scatter_merge_sparse_device", "stg_merge_optimize_sgd_sparse_device",
       "stg_merge_optimize_adam_sparse_device", "stg_merge_sparse_scratch_bytes"]


def test_header_declares_and_python_binds_the_sparse_entries():
    import stellatrain_amd as S
    from stellatrain_amd._capi import _SIGS, header_symbols, lib
    syms = header_symbols()
    for s in NEW:
        assert s in syms and s in _SIGS and hasattr(lib(), s), s
    assert callable(S.scatter_merge_sparse) and callable(S.merge_sparse_scratch_bytes)
    assert hasattr(S.SparseSGD, "merge_optimize_sparse") and hasattr(S.SparseAdam, "merge_optimize_sparse")


def test_scratch_bytes_by_hand():
    """4 world T + 12 min(T, P) + 12 P + 16 with T = ceil(n / 4096), P = world per_rank."""
    from stellatrain_amd import merge_sparse_scratch_bytes as f
    # T = 4096, P = 1,342,176: 131,072 + 49,152 + 16,106,112 + 16
    assert f(167772, 8, 1 << 24) == 16286352
    # T = 2^20, P = 1,800: 12,582,912 + 21,600 + 21,600 + 16 -- nothing of n's size
    assert f(600, 3, 2 ** 32 - 1) == 12626128
    # T = 4 (one partial tile), P = 2: 32 + 24 + 24 + 16
    assert f(1, 2, 3 * 4096 + 5) == 96
    assert f(0, 1, 0) == 16


def test_size_refusals_need_no_device():
    from stellatrain_amd._capi import StgRankStream, lib
    L = lib()
    out = C.c_size_t(7)
    f = L.stg_merge_sparse_scratch_bytes
    assert f(1 << 29, 8, 100, C.byref(out)) == -4 and b"world * per_rank" in L.stg_last_error() and out.value == 0
    assert f((1 << 29) - 1, 8, 100, C.byref(out)) == 0 and out.value > 12 * 8 * ((1 << 29) - 1)
    assert f(4, 1, 1 << 32, C.byref(out)) == -4 and f(1 << 32, 1, 4, C.byref(out)) == -4
    assert f(4, 0, 100, C.byref(out)) == -1 and f(4, 1, 100, None) == -1
    buf = (C.c_uint8 * 64)()
    p16 = (C.addressof(buf) + 15) & ~15
    o = C.c_void_p(p16)
    ranks = (StgRankStream * 8)(*[StgRankStream(p16, p16, 0)] * 8)
    assert L.stg_scatter_merge_sparse_device(ranks, 1 << 29, 8, 100, o, o, o, None) == -4
    assert b"world * per_rank" in L.stg_last_error()
    h = C.c_void_p()
    assert L.stg_sgd_create(0, 0.1, 0.9, 0.0, 0.0, 0, 0, C.byref(h)) == 0
    assert L.stg_merge_optimize_sgd_sparse_device(h, b"w", o, 100, ranks, 1 << 29, 8, o, o, o, None) == -4
    it = C.c_uint32(9)
    assert L.stg_sgd_get_iter(h, C.byref(it)) == 0 and it.value == 0  # a refused call is no iteration
    assert L.stg_sgd_destroy(h) == 0
