"""CPU-only checks of the dense-gradient MERGE entries: declarations and
binding, and every refusal, none of which needs a device."""
from __future__ import annotations

import ctypes as C

import pytest

INVALID, UNSUPPORTED = -1, -4


def _args():
    """A well-formed call's arguments over 16-byte aligned host words (never dereferenced by a refusal)."""
    from stellatrain_amd._capi import StgRankStream
    buf = (C.c_uint8 * 64)()
    p = (C.addressof(buf) + 15) & ~15
    ranks = (StgRankStream * 2)(StgRankStream(p, p, 0), StgRankStream(p, p, 3))
    return {"keep": buf, "ranks": ranks, "per_rank": 4, "world": 2, "n": 100, "d_grad": p, "dtype": 0, "accumulate": 0}


def _bad(field, value, code, word):
    a = _args()
    if field == "flag":
        a["ranks"][1].flag = value
    elif field == "d_val":
        a["ranks"][1].d_val = value
    else:
        a[field] = value
    return a, code, word


REFUSALS = {
    "world0": lambda: _bad("world", 0, INVALID, b"world"),
    "null_ranks": lambda: _bad("ranks", None, INVALID, b"null rank stream array"),
    "null_buffer": lambda: _bad("d_val", None, INVALID, b"null rank stream buffer"),
    "flag4": lambda: _bad("flag", 4, INVALID, b"wire flag"),
    "null_grad": lambda: _bad("d_grad", None, INVALID, b"null gradient"),
    "dtype3": lambda: _bad("dtype", 3, INVALID, b"dtype"),
    "n_2^32": lambda: _bad("n", 1 << 32, UNSUPPORTED, b"2^32"),
    "per_rank_2^32": lambda: _bad("per_rank", 1 << 32, UNSUPPORTED, b"2^32"),
    "pairs_2^32": lambda: _bad("per_rank", 1 << 31, UNSUPPORTED, b"world * per_rank"),
}


def test_header_declares_and_python_binds_the_entries():
    import stellatrain_amd as S
    from stellatrain_amd._capi import _SIGS, header_symbols, lib
    for s in ("stg_merge_grad_device", "stg_merge_grad_batch_device"):
        assert s in header_symbols() and s in _SIGS and hasattr(lib(), s), s
    assert callable(S.merge_grad) and callable(S.merge_grad_batch) and callable(S.GradTasks)
    assert C.sizeof(S.StgGradTask) == 48 and S.StgGradTask.d_grad.offset == 32


@pytest.mark.parametrize("case", list(REFUSALS) + ["grad_odd", "grad_2mod4"])
def test_refusals_need_no_device(case):
    """Each refusal with its code, alone and as task 1 of a batch (whose message names the task)."""
    from stellatrain_amd._capi import StgGradTask, lib
    L = lib()
    if case in REFUSALS:
        a, code, word = REFUSALS[case]()
    else:  # element alignment: fp16 at an odd address; fp32 at 2 mod 4 (fine for bf16)
        a, code, word = _args(), INVALID, b"misaligned"
        a["d_grad"] += 1 if case == "grad_odd" else 2
        a["dtype"] = 2 if case == "grad_odd" else 0
    order = ("ranks", "per_rank", "world", "n", "d_grad", "dtype", "accumulate")
    assert L.stg_merge_grad_device(*[a[f] for f in order], None) == code
    assert word in L.stg_last_error(), L.stg_last_error()
    good = _args()
    tasks = (StgGradTask * 2)(StgGradTask(*[good[f] for f in order]), StgGradTask(*[a[f] for f in order]))
    assert L.stg_merge_grad_batch_device(tasks, 2, None) == code
    assert L.stg_last_error().startswith(b"task 1: ") and word in L.stg_last_error()


def test_batch_null_array_and_empty_call():
    from stellatrain_amd._capi import lib
    assert lib().stg_merge_grad_batch_device(None, 3, None) == INVALID
    assert lib().stg_merge_grad_batch_device(None, 0, None) == 0
