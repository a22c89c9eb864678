"""CPU-only checks of the batched entries' launch counter
(``stg_merge_batch_launches``, ``merge_batch_launches``): the C-ABI
declaration, the export, the Python binding, and the argument check that runs
before any device call."""
from __future__ import annotations

import ctypes as C

NAME = "stg_merge_batch_launches"


def test_header_declares_the_counter():
    from stellatrain_amd._capi import HEADER, header_symbols
    assert NAME in header_symbols()
    txt = open(HEADER).read()
    assert "int stg_merge_batch_launches(void *stream, uint64_t *out);" in txt


def test_library_exports_the_counter():
    from stellatrain_amd._capi import lib
    assert hasattr(lib(), NAME)


def test_python_binds_the_counter():
    import stellatrain_amd as S
    from stellatrain_amd._capi import _SIGS
    assert _SIGS[NAME] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)])
    assert callable(S.merge_batch_launches)
    from stellatrain_amd import engine
    assert "merge_batch_launches" in engine.__all__


def test_null_out_is_refused_without_a_device():
    from stellatrain_amd._capi import lib
    L = lib()
    assert L.stg_merge_batch_launches(None, None) == -1  # STG_ERR_INVALID
    assert b"null" in L.stg_last_error()
