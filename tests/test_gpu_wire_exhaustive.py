"""GPU parity of every path that writes or reads the 16-bit wire forms against
the x86 instructions of the reference's casts, on the inputs where a cast can
go wrong: every binary16 word, every float32 rounding boundary, NaNs over the
payload range, the edges of the index and tail casts (tests/wire_tables.py).

Expected values come from ``oracle.IsaWire`` -- the instructions executed on
the CPU (oracle/isa_wire.cpp), which share no text with csrc/wire_dev.h; what
comes before the cast (thresholdv16) or after it (MERGE, the SGD step) is the
oracle's.  tests/test_wire_isa_host.py pins the tables, the yardstick and the
conditions section D relies on.

A. wire_encode / wire_encode_batch         every byte
B. wire_decode / wire_decode_batch         every bit, the 2,046 NaN words included
C. the readers that fuse the decode        scatter_merge_wire (copy-through, election,
                                           world 4), merge_optimize_wire, merge_optimize_batch
D. the writers that fuse the encode        thresholdv16's wire emission (one bucket,
                                           batched), the one-call send path
"""
from __future__ import annotations

import numpy as np
import pytest

import wire_tables as T
from parity import assert_same_f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def isa():
    from oracle.oracle import IsaWire
    return IsaWire()


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.itemsize == 2 else a.view(np.uint32)


def _up(torch, gpu, a):
    """A numpy array on the device, int16 / int32 typed for the unsigned forms."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(gpu)


def _same_bytes(got, exp, what):
    g, e = _u(got.cpu().numpy()), _u(exp)
    assert g.shape == e.shape, what
    bad = np.flatnonzero(g != e)
    assert not bad.size, (what, f"{bad.size} of {e.size} differ, first at {int(bad[0])}: got "
                          f"0x{int(g[bad[0]]):x}, expected 0x{int(e[bad[0]]):x}")


# ---------------------------------------------------------------------------
# A. encode
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [2, 3])
def test_a_encode_every_rounding_boundary(gpu, isa, flag):
    import torch
    from stellatrain_amd import wire_encode
    idx, val = T.boundary_stream()
    assert T.simd_end(val.size) >= T.f32_boundary().size >= 640000
    ei, ev = isa.encode(idx, val, flag)
    gi, gv = wire_encode(_up(torch, gpu, idx), _up(torch, gpu, val), flag)
    _same_bytes(gi, ei, f"indices, flag {flag}")
    _same_bytes(gv, ev, f"values, flag {flag}")


def test_a_encode_batch_tail_streams(gpu, isa):
    """TAIL_F32 and IDX_U32 at block and at tail positions, streams of 1-9, 16
    and 17 pairs, every flag, in one batched call."""
    import torch
    from stellatrain_amd import wire_encode_batch
    items, expect, names = [], [], []
    for flag in (0, 1, 2, 3):
        for j, (idx, val) in enumerate(T.encode_tail_cases() + (T.table_block_stream(),)):
            m = idx.size
            io = torch.full((m,), -1, dtype=torch.int16 if flag & 1 else torch.int32, device=gpu)
            vo = torch.full((m,), -1, dtype=torch.int16 if flag & 2 else torch.float32, device=gpu)
            items.append((_up(torch, gpu, idx), _up(torch, gpu, val), flag, io, vo))
            expect.append(isa.encode(idx, val, flag))
            names.append(f"stream {j} ({m} pairs), flag {flag}")
    wire_encode_batch(items)
    torch.cuda.synchronize()
    for (_, _, _, io, vo), (ei, ev), name in zip(items, expect, names):
        _same_bytes(io, ei, "indices of " + name)
        _same_bytes(vo, ev, "values of " + name)


# ---------------------------------------------------------------------------
# B. decode: no arithmetic on this path, so no exemptions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [1, 2, 3])
def test_b_decode_every_word(gpu, isa, flag):
    import torch
    from stellatrain_amd import wire_decode
    wi, wv = T.wide_forms(*T.f16_all_stream(), flag)
    assert T.simd_end(wi.size) >= 65536
    ei, ev = isa.decode(wi, wv, flag)
    if flag & 2:
        assert int(np.isnan(ev).sum()) == T.F16_NAN_WORDS == 2046
    gi, gv = wire_decode(_up(torch, gpu, wi), _up(torch, gpu, wv), flag)
    _same_bytes(gi, ei, f"indices, flag {flag}")
    _same_bytes(gv, ev, f"values, flag {flag}")


def test_b_decode_batch_tail_streams(gpu, isa):
    import torch
    from stellatrain_amd import wire_decode_batch
    items, expect, names = [], [], []
    for flag in (0, 1, 2, 3):
        for j, (w16i, w16v) in enumerate(T.decode_tail_cases() + (T.f16_all_stream(),)):
            wi, wv = T.wide_forms(w16i, w16v, flag)
            m = wi.size
            io = torch.full((m,), -1, dtype=torch.int32, device=gpu)
            vo = torch.full((m,), -1, dtype=torch.float32, device=gpu)
            items.append((_up(torch, gpu, wi), _up(torch, gpu, wv), flag, io, vo))
            expect.append(isa.decode(wi, wv, flag))
            names.append(f"stream {j} ({m} pairs), flag {flag}")
    wire_decode_batch(items)
    torch.cuda.synchronize()
    for (_, _, _, io, vo), (ei, ev), name in zip(items, expect, names):
        _same_bytes(io, ei, "indices of " + name)
        _same_bytes(vo, ev, "values of " + name)


# ---------------------------------------------------------------------------
# C. readers that fuse the decode
# ---------------------------------------------------------------------------
TAIL_WORDS = np.array([0, 1, 0x3C00, 0x7BFF, 0x7C01, 0x8000, 0xFC00, 0xFFFF], np.uint16)  # a tail reads them as integers


def _rank(words, idx, tail_idx, flag):
    """One rank stream: `words` at indices `idx` in the block part (a multiple
    of 8 pairs), then a tail of 8 pairs (TAIL_WORDS at tail_idx)."""
    assert words.size % 8 == 0 and words.size == idx.size and len(tail_idx) == 8
    wv = np.concatenate([words, TAIL_WORDS]).astype(np.uint16)
    ix = np.concatenate([idx, np.asarray(tail_idx)]).astype(np.int64)
    wi = ix.astype(np.uint16) if flag & 1 else ix.astype(np.uint32)
    assert T.simd_end(wv.size) == words.size
    return np.ascontiguousarray(wi), wv, flag


def _nan_words(streams):
    return sum(int(np.count_nonzero((wv[:T.simd_end(wv.size)] & 0x7FFF) > 0x7C00)) for _, wv, _ in streams)


def _full(repeat=False):
    """Every word as a value word, u32 indices counting up (flag 2)."""
    wi, wv, f = _rank(T.F16_ALL, np.arange(65536), 65536 + np.arange(8), 2)
    if repeat:
        wi[3] = wi[1000]   # pair 3 loses to pair 1000: the stream is no longer duplicate-free
    return dict(streams=[(wi, wv, f)], per_rank=65544, n=65549, nan=2046)


def _half(h):
    """32,768 words with u16 indices (flag 3); the tail's indices are >= 32,768."""
    w = T.F16_ALL[h * 32768:(h + 1) * 32768]
    return dict(streams=[_rank(w, np.arange(32768), 32768 + 100 * h + np.arange(8), 3)], per_rank=32776, n=40000,
                nan=1023)


def _quarters_u32():
    """World 4, flag 2: four quarter streams on disjoint indices: every sum is v + 0."""
    s = [_rank(T.F16_ALL[q * 16384:(q + 1) * 16384], q * 16384 + np.arange(16384), 65536 + 8 * q + np.arange(8), 2)
         for q in range(4)]
    return dict(streams=s, per_rank=16392, n=65536 + 32 + 5, nan=2046)


def _pair_u16(h):
    """World 2, flag 3: the two quarters of half h on disjoint u16 indices."""
    s = [_rank(T.F16_ALL[(2 * h + q) * 16384:(2 * h + q + 1) * 16384], q * 16384 + np.arange(16384),
               32768 + 8 * q + np.arange(8), 3) for q in range(2)]
    return dict(streams=s, per_rank=16392, n=40000, nan=1023)


def _merged(isa, oracle, case):
    """IsaWire.decode per rank, then the oracle's merge: (idx ascending, val)."""
    assert _nan_words(case["streams"]) == case["nan"]
    dec = [isa.decode(wi, wv, f) for wi, wv, f in case["streams"]]
    idx = np.concatenate([d[0] for d in dec])
    val = np.concatenate([d[1] for d in dec])
    assert idx.max() < case["n"] and all(d[0].size == case["per_rank"] for d in dec)
    ei, ev = oracle.merge_decompress(idx, val, case["per_rank"], len(dec), case["n"])
    assert int(np.isnan(ev).sum()) == case["nan"]
    return ei, ev


def _sorted_stream(oi, ov, cnt):
    c = int(cnt.cpu().numpy().view(np.uint32)[0])
    assert c != 0xFFFFFFFF
    i = oi.cpu().numpy().view(np.uint32)[:c]
    v = ov.cpu().numpy()[:c]
    o = np.argsort(i, kind="stable")
    return i[o], v[o]


def _check_stream(got, ei, ev, nan, what):
    """Indices equal; a position whose expected value is NaN holds a NaN (of any
    payload: the merge's add picks it), every other one the same bits; and the
    NaNs are exactly the stream's NaN words."""
    assert np.array_equal(got[0], ei), what
    assert_same_f32(got[1], ev, what)
    assert int(np.isnan(got[1]).sum()) == nan, what


def _dev(torch, gpu, case):
    return [(_up(torch, gpu, wi), _up(torch, gpu, wv), f) for wi, wv, f in case["streams"]]


@pytest.mark.parametrize("which", ["full", "full+repeat", "half0", "half1", "world4", "pair0", "pair1"])
def test_c_scatter_merge_wire(gpu, oracle, isa, which):
    """World 1 without a repeat copies through; with one it elects through the
    tickets (win_keep_t, wire_val_wp); world > 1 marks and sums (scatter_mark_w)."""
    import torch
    from stellatrain_amd import scatter_merge_wire
    from stellatrain_amd.engine import scatter_merge_check
    case = {"full": _full, "full+repeat": lambda: _full(True), "half0": lambda: _half(0), "half1": lambda: _half(1),
            "world4": _quarters_u32, "pair0": lambda: _pair_u16(0), "pair1": lambda: _pair_u16(1)}[which]()
    ei, ev = _merged(isa, oracle, case)
    world = len(case["streams"])
    assert ei.size == case["per_rank"] * world - (which == "full+repeat")
    dense = torch.zeros(case["n"], dtype=torch.float32, device=gpu)
    mark = torch.zeros(case["n"], dtype=torch.uint8, device=gpu)
    got = _sorted_stream(*scatter_merge_wire(_dev(torch, gpu, case), case["per_rank"], case["n"], dense=dense,
                                             mark=mark))
    _check_stream(got, ei, ev, case["nan"], which)
    scatter_merge_check()
    assert not bool(dense.view(torch.int32).any()) and not bool(mark.any())


def _sgd_expected(oracle, h, name, p0, ei, ev):
    po = p0.copy()
    oracle.sgd_apply(h, name, po, ev, ei)
    return po


def _check_param(p, po, ei, ev, what):
    """The stepped parameter: NaN exactly where the merged value is NaN,
    bit-exact everywhere else (untouched elements included)."""
    got = p.cpu().numpy()
    assert_same_f32(got, po, what)
    assert np.array_equal(np.flatnonzero(np.isnan(got)), ei[np.isnan(ev)]), what


P0 = (np.arange(65600, dtype=np.float32) % np.float32(251) - np.float32(125)) * np.float32(0.03125)


@pytest.mark.parametrize("which", ["full", "full+repeat", "half1"])
def test_c_merge_optimize_wire_sgd(gpu, oracle, isa, which):
    import torch
    from stellatrain_amd import SparseSGD
    from stellatrain_amd.engine import scatter_merge_check
    case = {"full": _full, "full+repeat": lambda: _full(True), "half1": lambda: _half(1)}[which]()
    ei, ev = _merged(isa, oracle, case)
    opt, h = SparseSGD(lr=0.05), oracle.sgd_new(lr=0.05)
    try:
        p0 = P0[:case["n"]].copy()
        po = _sgd_expected(oracle, h, "w", p0, ei, ev)
        p = torch.from_numpy(p0).to(gpu)
        got = _sorted_stream(*opt.merge_optimize_wire(p, "w", _dev(torch, gpu, case), case["per_rank"]))
        _check_stream(got, ei, ev, case["nan"], which)
        _check_param(p, po, ei, ev, which)
        opt.check()
        scatter_merge_check()
    finally:
        oracle.sgd_free(h)


def test_c_merge_optimize_batch_sgd(gpu, oracle, isa):
    """Two world-1 tasks (merge_batch.hip) and two world-2 tasks
    (merge_batch_world.hip) in one call."""
    import torch
    from stellatrain_amd import SparseSGD
    from stellatrain_amd.engine import scatter_merge_check
    cases = {"f": _full(True), "h": _half(0), "p0": _pair_u16(0), "p1": _pair_u16(1)}
    opt, h = SparseSGD(lr=0.05), oracle.sgd_new(lr=0.05)
    try:
        items, exp = [], []
        for name, case in cases.items():
            ei, ev = _merged(isa, oracle, case)
            p0 = P0[:case["n"]].copy()
            exp.append((name, case, ei, ev, _sgd_expected(oracle, h, name, p0, ei, ev)))
            items.append((torch.from_numpy(p0).to(gpu), name, _dev(torch, gpu, case), case["per_rank"]))
        outs = opt.merge_optimize_batch(items)
        assert len(outs) == 4
        for (p, *_), out, (name, case, ei, ev, po) in zip(items, outs, exp):
            _check_stream(_sorted_stream(*out), ei, ev, case["nan"], name)
            _check_param(p, po, ei, ev, name)
        opt.check()
        scatter_merge_check()
    finally:
        oracle.sgd_free(h)


# ---------------------------------------------------------------------------
# D. writers that fuse the encode
# ---------------------------------------------------------------------------
def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _wire_bufs(torch, gpu, cap, flag):
    di = torch.full((cap,), -1, dtype=torch.int16 if flag & 1 else torch.int32, device=gpu)
    dv = torch.full((cap,), -1, dtype=torch.int16 if flag & 2 else torch.float32, device=gpu)
    return di, dv


def _run_fused(gpu, oracle, isa, seqs, flag):
    """One batched call per step over the keys of `seqs`; count, both wire
    arrays and the key's state against the oracle's compress + IsaWire.encode."""
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    comp = ThresholdvCompressor16()
    calls = max(len(s[3]) for s in seqs)
    ties = 0
    for it in range(calls):
        live = [s for s in seqs if it < len(s[3])]
        items, exp = [], []
        for key, n, k, bands, sb in live:
            x, co, io, vo, after, _ = T.bucket_sequence(oracle, key, n, k, bands, sb)[it]
            di, dv = _wire_bufs(torch, gpu, k, flag)
            items.append((key, torch.from_numpy(x.copy()).to(gpu), k, di, dv, 0))  # (the shared row is read-only)
            exp.append((co, isa.encode(io[:co], vo[:co], flag), after))
            ties += int(T.is_tie(vo[:T.simd_end(co)]).sum())
        counts = comp.compress_batch_async(items, wire_flags=[flag] * len(items))
        torch.cuda.synchronize()
        got = counts.cpu().numpy().tolist()
        for (key, _, k, di, dv, _), (co, (ei, ev), after), cg in zip(items, exp, got):
            what = f"call {it}, key {key}, flag {flag}"
            assert cg == co, what
            _same_bytes(di[:co], ei, "indices: " + what)
            _same_bytes(dv[:co], ev, "values: " + what)
            assert _bits(comp.state(key)) == _bits(after), what
    comp.check_device()
    assert ties >= 64 * calls


@pytest.mark.parametrize("flag", [2, 3])
@pytest.mark.parametrize("seq", T.D_ONE, ids=[s[0] + ":" + "-".join(s[3]) for s in T.D_ONE])
def test_d_fused_one_bucket(gpu, oracle, isa, seq, flag):
    """One key per band, and normal -> sub -> top -> normal on one key (the
    regime-B fill's emission sites see ties, subnormals and the carry)."""
    _run_fused(gpu, oracle, isa, [seq], flag)


@pytest.mark.parametrize("flag", [2, 3])
def test_d_fused_batched(gpu, oracle, isa, flag):
    """The three bands as three keys of one batched launch."""
    _run_fused(gpu, oracle, isa, list(T.D_BATCH), flag)


@pytest.mark.parametrize("mode", ["engine", "items"])
def test_d_send_two_sources(gpu, oracle, isa, mode):
    """The one-call send path at flag 3 with N = 2 sources: boundary values in
    grad[0], zeros in the second source, so the gathered bucket is again made
    of boundary values.  grad[0], count, wire arrays and state."""
    import torch
    from stellatrain_amd import CodecEngine, ThresholdvCompressor16
    seqs = T.send_sequences(oracle)
    eng = CodecEngine() if mode == "engine" else None
    comp = eng.compressor() if eng else ThresholdvCompressor16()
    for it in range(max(len(s[3]) for s in seqs)):
        live = [s for s in seqs if it < len(s[3])]
        rows = [T.bucket_sequence(oracle, *s)[it] for s in live]
        g = [[torch.from_numpy(T.boundary_bucket(s[1], s[4], it, s[3][it])).to(gpu),
              torch.zeros(s[1], dtype=torch.float32, device=gpu)] for s in live]
        if eng:
            streams, counts = eng.send_buckets([(s[0], gs) for s, gs in zip(live, g)], fp16_values=True)
            outs = [(wi, wv) for wi, wv, fl in streams]
            assert all(fl == 3 and wi.numel() == s[2] for (wi, wv, fl), s in zip(streams, live))
        else:
            outs = [_wire_bufs(torch, gpu, s[2], 3) for s in live]
            counts = comp.merge_send_batch_async([(s[0], gs, s[2], di, dv, None, 3)
                                                  for s, gs, (di, dv) in zip(live, g, outs)])
        torch.cuda.synchronize()
        got = counts.cpu().numpy().tolist()
        for s, gs, (di, dv), (x, co, io, vo, after, _), cg in zip(live, g, outs, rows, got):
            what = f"call {it}, key {s[0]} ({mode})"
            assert cg == co, what
            _same_bytes(gs[0], x, "grad[0]: " + what)
            ei, ev = isa.encode(io[:co], vo[:co], 3)
            _same_bytes(di[:co], ei, "indices: " + what)
            _same_bytes(dv[:co], ev, "values: " + what)
            assert _bits(comp.state(s[0])) == _bits(after), what
    comp.check_device()
