"""CPU-only checks of the wire-form MERGE entry points: the C-ABI declarations
and their Python binding, the argument checks that run before any device
call, and the expected-value helper the GPU tests share
(tests/wire_merge_cases.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import wire_merge_cases as W

NEW = ["stg_scatter_merge_wire_device", "stg_merge_optimize_sgd_wire_device", "stg_merge_optimize_adam_wire_device",
       "stg_wire_decode_batch_device"]


def test_header_declares_and_python_binds_the_new_entry_points():
    from stellatrain_amd._capi import _SIGS, HEADER, header_symbols, lib
    syms = header_symbols()
    L = lib()
    for s in NEW:
        assert s in syms and s in _SIGS and hasattr(L, s), s
    txt = open(HEADER).read()
    assert "stg_rank_stream_t" in txt and "stg_wire_rx_t" in txt
    import stellatrain_amd as S
    for name in ("scatter_merge_wire", "wire_decode_batch"):
        assert callable(getattr(S, name)), name
    assert hasattr(S.SparseSGD, "merge_optimize_wire") and hasattr(S.SparseAdam, "merge_optimize_wire")


def test_struct_layouts_match_the_header():
    """stg_rank_stream_t {ptr, ptr, int} and stg_wire_rx_t {ptr, ptr, size_t, int, ptr, ptr}."""
    from stellatrain_amd._capi import StgRankStream, StgWireRx
    assert C.sizeof(StgRankStream) == 24 and StgRankStream.flag.offset == 16
    assert C.sizeof(StgWireRx) == 48 and StgWireRx.flag.offset == 24 and StgWireRx.d_idx.offset == 32


def test_argument_checks_need_no_device():
    from stellatrain_amd._capi import StgRankStream, StgWireRx, lib
    L = lib()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    p16 = (p + 15) & ~15
    good = (StgRankStream * 2)(StgRankStream(p16, p16, 1), StgRankStream(p16, p16, 3))
    out = C.c_void_p(p16)

    def merge(ranks, per_rank, world, dense, mark):
        return L.stg_scatter_merge_wire_device(ranks, per_rank, world, 100, dense, mark, out, out, out, None)

    assert merge(good, 4, 0, None, None) == -1 and b"world" in L.stg_last_error()
    assert merge(good, 4, -3, None, None) == -1
    assert merge(None, 4, 1, None, None) == -1 and b"rank" in L.stg_last_error()
    for bad in (4, -1, 7, 256):
        ranks = (StgRankStream * 2)(StgRankStream(p16, p16, 0), StgRankStream(p16, p16, bad))
        assert merge(ranks, 4, 2, out, out) == -1 and b"flag" in L.stg_last_error(), bad
    assert merge(good, 4, 2, None, out) == -1 and b"scratch" in L.stg_last_error()
    assert merge(good, 4, 2, out, None) == -1 and b"scratch" in L.stg_last_error()
    assert merge(good, 4, 2, out, C.c_void_p(p16 + 4)) == -1 and b"aligned" in L.stg_last_error()
    null = (StgRankStream * 1)(StgRankStream(None, p16, 1))
    assert merge(null, 4, 1, None, None) == -1 and b"null" in L.stg_last_error()
    odd = (StgRankStream * 1)(StgRankStream(p16 + 2, p16, 0))  # u32 indices at a 2-byte address
    assert merge(odd, 4, 1, None, None) == -1 and b"misaligned" in L.stg_last_error()

    # the fused forms check the handle and the same arguments first
    h = C.c_void_p()
    assert L.stg_sgd_create(0, 0.1, 0.9, 0.0, 0.0, 0, 0, C.byref(h)) == 0
    f = L.stg_merge_optimize_sgd_wire_device
    assert f(None, b"w", out, 100, good, 4, 1, None, None, out, out, out, None) == -1
    assert f(h, None, out, 100, good, 4, 1, None, None, out, out, out, None) == -1
    assert f(h, b"w", out, 100, good, 4, 0, None, None, out, out, out, None) == -1
    assert f(h, b"w", out, 100, None, 4, 1, None, None, out, out, out, None) == -1
    assert f(h, b"w", out, 100, good, 4, 2, None, None, out, out, out, None) == -1
    it = C.c_uint32(9)
    assert L.stg_sgd_get_iter(h, C.byref(it)) == 0 and it.value == 0  # a refused call is no iteration
    assert L.stg_sgd_destroy(h) == 0
    a = C.c_void_p()
    assert L.stg_adam_create(0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0, C.byref(a)) == 0
    f = L.stg_merge_optimize_adam_wire_device
    assert f(None, b"w", out, 100, good, 4, 1, None, None, out, out, out, None) == -1
    assert f(a, b"w", out, 100, good, 4, 0, None, None, out, out, out, None) == -1
    assert f(a, b"w", out, 100, None, 4, 1, None, None, out, out, out, None) == -1
    bad = (StgRankStream * 1)(StgRankStream(p16, p16, 8))
    assert f(a, b"w", out, 100, bad, 4, 1, None, None, out, out, out, None) == -1
    assert L.stg_adam_destroy(a) == 0

    # batched decode
    assert L.stg_wire_decode_batch_device(None, 0, None) == 0
    assert L.stg_wire_decode_batch_device(None, 2, None) == -1
    rx = (StgWireRx * 1)(StgWireRx(p16, p16, 4, 5, p16, p16))
    assert L.stg_wire_decode_batch_device(rx, 1, None) == -1 and b"flag" in L.stg_last_error()
    rx = (StgWireRx * 1)(StgWireRx(p16, None, 4, 1, p16, p16))
    assert L.stg_wire_decode_batch_device(rx, 1, None) == -1 and b"null" in L.stg_last_error()
    rx = (StgWireRx * 1)(StgWireRx(None, None, 0, 1, None, None))  # an empty stream is no work
    assert L.stg_wire_decode_batch_device(rx, 1, None) == 0


def test_misaligned_scratch_is_refused_for_world_above_one():
    """d_mark and d_dense are read as 16-byte vectors by the world > 1 emission:
    each is refused at every other phase, by every MERGE entry (the batched
    tasks included), with an error that names the buffer; world 1 looks at
    neither."""
    from stellatrain_amd._capi import StgMergeTask, StgRankStream, lib
    L = lib()
    buf = (C.c_uint8 * 128)()
    p16 = (C.addressof(buf) + 15) & ~15
    out = C.c_void_p(p16)
    two = (StgRankStream * 2)(StgRankStream(p16, p16, 1), StgRankStream(p16, p16, 3))
    one = (StgRankStream * 1)(StgRankStream(p16, p16, 0))
    h = C.c_void_p()
    assert L.stg_sgd_create(0, 0.1, 0.9, 0.0, 0.0, 0, 0, C.byref(h)) == 0
    a = C.c_void_p()
    assert L.stg_adam_create(0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0, C.byref(a)) == 0

    def entries(ranks, world, dense, mark):
        """Every MERGE entry on the same scratch arguments, before any device call."""
        task = (StgMergeTask * 1)(StgMergeTask(b"w", p16, 100, ranks, 4, world, dense, mark, p16, p16, p16))
        d, m = C.c_void_p(dense), C.c_void_p(mark)
        yield "wire", L.stg_scatter_merge_wire_device(ranks, 4, world, 100, d, m, out, out, out, None)
        yield "decoded", L.stg_scatter_merge_device(out, out, 4, world, 100, d, m, out, out, out, None)
        yield "sgd", L.stg_merge_optimize_sgd_wire_device(h, b"w", out, 100, ranks, 4, world, d, m, out, out, out, None)
        yield "sgd decoded", L.stg_merge_optimize_sgd_device(h, b"w", out, 100, out, out, 4, world, d, m, out, out, out,
                                                             None)
        yield "adam", L.stg_merge_optimize_adam_wire_device(a, b"w", out, 100, ranks, 4, world, d, m, out, out, out,
                                                            None)
        yield "sgd batch", L.stg_merge_optimize_sgd_batch_device(h, task, 1, None)
        yield "adam batch", L.stg_merge_optimize_adam_batch_device(a, task, 1, None)

    for off in (1, 4, 8, 12, 15):
        for entry, rc in entries(two, 2, p16, p16 + off):
            assert rc == -1, (entry, off)
            err = L.stg_last_error()
            assert b"mark" in err and b"aligned" in err and b"dense" not in err, (entry, off, err)
    for off in (4, 8, 12):  # a float buffer: element-aligned, not 16-byte aligned
        for entry, rc in entries(two, 2, p16 + off, p16):
            assert rc == -1, (entry, off)
            err = L.stg_last_error()
            assert b"dense" in err and b"aligned" in err and b"mark" not in err, (entry, off, err)
            assert not entry.endswith("batch") or err.startswith(b"task 0"), err
    it = C.c_uint32(9)
    assert L.stg_sgd_get_iter(h, C.byref(it)) == 0 and it.value == 0  # a refused call is no iteration
    # world 1 uses neither: the same pointers pass these checks.  (An accepted
    # call needs a device; a batched task is checked in full before any device
    # call, so the refusal that comes after this one -- the fused step's empty
    # parameter -- shows that the scratch pointers were let through.)
    for dense, mark in ((p16 + 4, p16 + 1), (None, None)):
        task = (StgMergeTask * 1)(StgMergeTask(b"w", p16, 0, one, 4, 1, dense, mark, p16, p16, p16))
        for f, o in ((L.stg_merge_optimize_sgd_batch_device, h), (L.stg_merge_optimize_adam_batch_device, a)):
            assert f(o, task, 1, None) != 0
            err = L.stg_last_error()
            assert b"empty parameter" in err and b"aligned" not in err, err
    assert L.stg_sgd_destroy(h) == 0 and L.stg_adam_destroy(a) == 0


def test_python_validation_needs_no_device():
    import pytest
    import torch
    from stellatrain_amd import scatter_merge_wire
    i16, i32, f32 = (torch.zeros(8, dtype=d) for d in (torch.int16, torch.int32, torch.float32))
    with pytest.raises(ValueError, match="flag"):
        scatter_merge_wire([(i32, f32, 4)], 8, 100)
    with pytest.raises(ValueError, match="dtypes"):
        scatter_merge_wire([(i32, f32, 1)], 8, 100)
    with pytest.raises(ValueError, match="dtypes"):
        scatter_merge_wire([(i16, f32, 3)], 8, 100)
    with pytest.raises(ValueError, match="contiguous"):
        scatter_merge_wire([(i16[::2], f32, 1)], 4, 100)
    with pytest.raises(ValueError, match="shorter"):
        scatter_merge_wire([(i16, f32, 1)], 9, 100)
    with pytest.raises(ValueError, match="at least one"):
        scatter_merge_wire([], 8, 100)


def test_expected_value_helper(oracle):
    """The oracle pair on hand-made wire bytes: sign extension drops a block
    index >= 0x8000, the tail zero-extends, the last occurrence wins, the tail's
    fp16 word is read as an integer."""
    per_rank, n = 10, 60000  # block part: pairs 0..7, tail: 8, 9
    wi = np.array([5, 0x8005, 7, 7, 9, 0xffff, 5, 11, 0x8005, 9], np.uint16)
    wv = np.array([0x3c00, 0x4000, 0x4200, 0x4400, 0xc000, 0x3c00, 0x3800, 0x7bff, 0x0003, 0x0004], np.uint16)
    idx, val, oi, ov, st = W.expected(oracle, [(wi, wv, 3)], per_rank, n)
    assert idx.tolist() == [5, 0xffff8005, 7, 7, 9, 0xffffffff, 5, 11, 0x8005, 9]
    assert val.tolist() == [1.0, 2.0, 3.0, 4.0, -2.0, 1.0, 0.5, 65504.0, 3.0, 4.0]
    assert oi.tolist() == [5, 7, 9, 11, 0x8005] and ov.tolist() == [0.5, 4.0, 4.0, 65504.0, 3.0]
    assert st == {"dups": 3, "dropped": 2, "tail": 2}
    # two ranks: rank-ordered sum over the union, divided by the world
    w2 = np.array([0x8005, 5], np.uint16)  # per_rank 2: both tail
    v2 = np.array([2.0, 8.0], np.float32)
    w3 = np.array([5, 6], np.uint16)
    v3 = np.array([1.0, 3.0], np.float32)
    _, _, oi, ov, st = W.expected(oracle, [(w2, v2, 1), (w3, v3, 1)], 2, n)
    assert oi.tolist() == [5, 6, 0x8005] and ov.tolist() == [4.5, 1.5, 1.0]
    assert st == {"dups": 0, "dropped": 0, "tail": 4}


def test_every_gpu_case_is_non_trivial(oracle):
    """No GPU case passes vacuously: each has a non-empty union and exercises
    duplicates, dropped indices or tail survivors; every (family, flag, world)
    group exercises all three, and so does every flag at every per_rank >= 9
    across its families."""
    group = {}
    for family, per_rank, flag, world in W.all_cases():
        n = W.n_of(flag)
        streams = W.make_streams(oracle, family, per_rank, flag, world)
        for wi, wv, f in streams:
            assert wi.size == wv.size == per_rank and f == flag
            assert wi.dtype == (np.uint16 if flag & 1 else np.uint32)
            assert wv.dtype == (np.uint16 if flag & 2 else np.float32)
        idx, val, oi, ov, st = W.expected(oracle, streams, per_rank, n)
        case = (family, per_rank, flag, world)
        assert idx.size == val.size == per_rank * world, case
        assert 0 < oi.size <= per_rank * world and np.all(np.diff(oi.astype(np.int64)) > 0) and oi.max() < n, case
        assert st["dups"] + st["dropped"] + st["tail"] > 0, case
        assert oi.size == per_rank * world - st["dups"] - st["dropped"] or world > 1, case
        g = group.setdefault((family, flag, world), {"dups": 0, "dropped": 0, "tail": 0})
        for k in g:
            g[k] += st[k]
        if family == "raw" and flag & 1 and per_rank >= 9:
            assert st["dropped"] >= W.wend(per_rank) * world, case  # every block index is past n
        if family == "encoded" and flag & 1 and per_rank >= 1023:
            assert st["dups"] > 0 and 32767 in oi, case  # the saturated indices
    for key, g in group.items():
        family, flag, world = key
        if family == "encoded" and flag & 1:  # a saturated index stays below n: nothing to drop
            assert g["dups"] and g["tail"], key
        else:
            assert all(g.values()), (key, g)
