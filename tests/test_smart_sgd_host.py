"""CPU-only checks of smart-momentum SGD: the golden file against its manifest,
the C-ABI declarations and their Python binding, and the argument check that
runs before any device call."""
from __future__ import annotations

import ctypes as C
import hashlib
import os

import numpy as np

import smart_sgd_golden as G

NEW = ["stg_sgd_set_smart_momentum", "stg_sgd_get_last", "stg_sgd_get_iter", "stg_sgd_check"]


def test_golden_matches_manifest():
    a = G.arrays()
    assert set(a) == set(G.MANIFEST["sha256"])
    for k, v in a.items():
        assert hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() == G.MANIFEST["sha256"][k], k
    assert os.path.getsize(G.NPZ) < 512 << 10
    assert [c["name"][0] for c in G.CASES] == list("abcdef")
    for c in G.CASES:
        assert max(c["lens"]) <= 20000 and 0 < c["momentum"] < 1
        calls = G.calls(c)
        assert len(calls) == c["calls"] == c["iter"]  # m_iter counts every call, whatever the name or length
        exp = G.initial_params(c)
        for nm, smart, idx, grad, after in calls:
            assert np.unique(idx).size == idx.size == grad.size == after.size  # the reference aborts on a repeat
            assert idx.size == 0 or idx.max() < c["lens"][nm]
            exp[nm][idx] = after
        touched = [np.zeros(n, bool) for n in c["lens"]]
        for s, (nm, smart, idx, *_) in enumerate(calls):
            assert smart == (s >= c["smart_from"])
            touched[nm][idx] = True
        for j in range(len(c["lens"])):
            param, mom, last = G.final_state(c, j)
            assert np.array_equal(param.view(np.uint32), exp[j].view(np.uint32))
            # last[idx] = m_iter of the last smart call that touched idx (sgd.cpp:258-259)
            want = np.zeros(c["lens"][j], np.uint32)
            for s, (nm, smart, idx, *_) in enumerate(calls):
                if nm == j and smart:
                    want[idx] = s
            assert np.array_equal(last, want)
            assert not mom[~touched[j]].any()


def test_golden_reaches_the_table_edges():
    """Case d (m = 0.5): a gap of 130 (a denormal factor) and one of 152 (past
    the first zero entry, d0 = 150); and the d0 the table is sized by."""
    d = G.case_by_name("d_")
    touch = {}
    gaps = set()
    for s, (nm, smart, idx, *_) in enumerate(G.calls(d)):
        for i in idx.tolist():
            if i in touch:
                gaps.add(s - touch[i])
            touch[i] = s
    assert {130, 152} <= gaps
    f130 = np.float32(0.5 ** 130)
    assert 0 < f130 < np.finfo(np.float32).tiny

    def d0(m):
        n = 0
        while np.float32(float(np.float32(m)) ** n) != 0:
            n += 1
        return n
    assert d0(0.5) == 150 and d0(0.9) == 987


def test_golden_differs_from_plain_momentum(oracle):
    """The goldens exercise the option: the CPU oracle's plain SGD on the same
    calls ends elsewhere in every case -- except where the option and plain
    momentum agree by construction (no case here)."""
    for c in G.CASES:
        h = oracle.sgd_new(**G.opts(c))
        p = G.initial_params(c)
        for nm, smart, idx, grad, after in G.calls(c):
            oracle.sgd_apply(h, c["names"][nm], p[nm], grad, idx)
        differs = any(not np.array_equal(p[j].view(np.uint32), G.final_state(c, j)[0].view(np.uint32))
                      for j in range(len(c["lens"])))
        oracle.sgd_free(h)
        assert differs, c["name"]


def test_header_declares_and_python_binds_the_new_entry_points():
    from stellatrain_amd._capi import _SIGS, header_symbols, lib
    syms = header_symbols()
    L = lib()
    for s in NEW:
        assert s in syms and s in _SIGS and hasattr(L, s), s
    from stellatrain_amd import SparseSGD
    for attr in ("configure", "last_buffer", "iteration", "check"):
        assert hasattr(SparseSGD, attr), attr


def test_smart_momentum_refused_without_momentum():
    """momentum 0 (the reference would read a null array) and momentum outside
    (0, 1) are refused before any device call; switching it off always works."""
    from stellatrain_amd._capi import lib
    L = lib()
    for m in (0.0, 1.0, 1.5, -0.5):
        h = C.c_void_p()
        assert L.stg_sgd_create(0, 0.1, m, 0.0, 0.0, 0, 0, C.byref(h)) == 0
        assert L.stg_sgd_set_smart_momentum(h, 1) == -1, m
        assert b"momentum" in L.stg_last_error()
        assert L.stg_sgd_set_smart_momentum(h, 0) == 0
        it = C.c_uint32(7)
        assert L.stg_sgd_get_iter(h, C.byref(it)) == 0 and it.value == 0
        assert L.stg_sgd_destroy(h) == 0
    assert L.stg_sgd_set_smart_momentum(None, 1) == -1
    assert L.stg_sgd_get_iter(None, None) == -1
    assert L.stg_sgd_check(None, None) == -1
    assert L.stg_sgd_get_last(None, b"w", None, 0, None) == -1
