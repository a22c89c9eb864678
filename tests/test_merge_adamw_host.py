"""CPU-only checks of the fused dense AdamW MERGE entries: declarations,
binding and struct layout, and every refusal, none of which needs a device."""
from __future__ import annotations

import ctypes as C

import pytest

INVALID, UNSUPPORTED = -1, -4
ORDER = ("ranks", "per_rank", "world", "n", "d_param", "dtype", "d_master", "d_exp_avg", "d_exp_avg_sq")
HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1, step=1, decoupled=1)


def _args():
    """A well-formed call's arguments over 16-byte aligned host words (never dereferenced by a refusal)."""
    from stellatrain_amd._capi import StgRankStream
    buf = (C.c_uint8 * 64)()
    p = (C.addressof(buf) + 15) & ~15
    ranks = (StgRankStream * 2)(StgRankStream(p, p, 0), StgRankStream(p, p, 3))
    return {"keep": buf, "ranks": ranks, "per_rank": 4, "world": 2, "n": 100, "d_param": p, "dtype": 0,
            "d_master": None, "d_exp_avg": p + 16, "d_exp_avg_sq": p + 32, "hyper": dict(HYPER)}


def _bf16(a):
    a["dtype"] = 1
    return a


# case -> (edit of the arguments, code, a word of the message)
REFUSALS = {
    "world0": (lambda a: a.update(world=0), INVALID, b"world"),
    "null_ranks": (lambda a: a.update(ranks=None), INVALID, b"null rank stream array"),
    "null_buffer": (lambda a: setattr(a["ranks"][1], "d_val", None), INVALID, b"null rank stream buffer"),
    "flag4": (lambda a: setattr(a["ranks"][1], "flag", 4), INVALID, b"wire flag"),
    "null_param": (lambda a: a.update(d_param=None), INVALID, b"null parameter"),
    "dtype3": (lambda a: a.update(dtype=3), INVALID, b"dtype"),
    "param_odd": (lambda a: a.update(d_param=a["d_param"] + 1, dtype=2), INVALID, b"misaligned"),
    "n_2^32": (lambda a: a.update(n=1 << 32), UNSUPPORTED, b"2^32"),
    "per_rank_2^32": (lambda a: a.update(per_rank=1 << 32), UNSUPPORTED, b"2^32"),
    "pairs_2^32": (lambda a: a.update(per_rank=1 << 31), UNSUPPORTED, b"world * per_rank"),
    "null_exp_avg": (lambda a: a.update(d_exp_avg=None), INVALID, b"null exp_avg"),
    "null_exp_avg_sq": (lambda a: a.update(d_exp_avg_sq=None), INVALID, b"null exp_avg"),
    "master_with_f32": (lambda a: a.update(d_master=a["d_param"]), INVALID, b"master"),
    "exp_avg_2mod4": (lambda a: _bf16(a).update(d_exp_avg=a["d_exp_avg"] + 2), INVALID, b"4 bytes"),
    "master_2mod4": (lambda a: _bf16(a).update(d_master=a["d_param"] + 2), INVALID, b"4 bytes"),
    "exp_avg_sq_phase": (lambda a: a.update(d_exp_avg_sq=a["d_exp_avg_sq"] + 4), INVALID, b"congruent"),
    "param_phase": (lambda a: a.update(d_param=a["d_param"] + 8), INVALID, b"congruent"),
    "master_phase": (lambda a: _bf16(a).update(d_master=a["d_param"] + 12), INVALID, b"congruent"),
}
HYPER_REFUSALS = {
    "step0": (dict(step=0), b"step"),
    "beta1_1": (dict(beta1=1.0), b"beta"),
    "beta2_neg": (dict(beta2=-0.1), b"beta"),
    "beta1_nan": (dict(beta1=float("nan")), b"beta"),
    "lr_neg": (dict(lr=-1e-3), b"lr"),
    "lr_inf": (dict(lr=float("inf")), b"lr"),
    "eps_nan": (dict(eps=float("nan")), b"eps"),
    "wd_neg": (dict(weight_decay=-0.1), b"weight_decay"),
    "null_hyper": (None, b"null hyper"),
}


def test_header_declares_and_python_binds_the_entries():
    import stellatrain_amd as S
    from stellatrain_amd._capi import _SIGS, header_symbols, lib
    for s in ("stg_merge_adamw_device", "stg_merge_adamw_batch_device"):
        assert s in header_symbols() and s in _SIGS and hasattr(lib(), s), s
    assert callable(S.merge_adamw) and callable(S.merge_adamw_batch) and callable(S.AdamWTasks)
    assert {"merge_adamw", "merge_adamw_batch", "AdamWTasks"} <= set(S.engine.__all__)
    T, H = S.StgAdamwTask, S.StgAdamwHyper
    assert C.sizeof(T) == 72 and (T.d_param.offset, T.dtype.offset, T.d_master.offset, T.d_exp_avg_sq.offset) == \
        (32, 40, 48, 64)
    assert C.sizeof(H) == 56 and (H.weight_decay.offset, H.step.offset, H.decoupled.offset) == (32, 40, 48)


@pytest.mark.parametrize("case", list(REFUSALS) + list(HYPER_REFUSALS))
def test_refusals_need_no_device(case):
    """Each refusal with its code, alone and as task 1 of a batch (whose message names the task)."""
    from stellatrain_amd._capi import StgAdamwHyper, StgAdamwTask, lib
    L = lib()
    a, good = _args(), _args()
    if case in REFUSALS:
        edit, code, word = REFUSALS[case]
        edit(a)
    else:
        change, word = HYPER_REFUSALS[case]
        code = INVALID
        a["hyper"] = dict(HYPER, **change) if change is not None else None
    hyper = C.byref(StgAdamwHyper(**a["hyper"])) if a["hyper"] is not None else None
    assert L.stg_merge_adamw_device(*[a[f] for f in ORDER], hyper, None) == code
    assert word in L.stg_last_error(), L.stg_last_error()
    tasks = (StgAdamwTask * 2)(StgAdamwTask(*[good[f] for f in ORDER]), StgAdamwTask(*[a[f] for f in ORDER]))
    assert L.stg_merge_adamw_batch_device(tasks, 2, hyper, None) == code
    assert word in L.stg_last_error(), L.stg_last_error()
    assert L.stg_last_error().startswith(b"task 1: ") == (case in REFUSALS)  # one hyper per call: no task to name


def test_batch_null_array_and_empty_call():
    from stellatrain_amd._capi import StgAdamwHyper, lib
    hyper = C.byref(StgAdamwHyper(**HYPER))
    assert lib().stg_merge_adamw_batch_device(None, 3, hyper, None) == INVALID
    assert lib().stg_merge_adamw_batch_device(None, 0, hyper, None) == 0
