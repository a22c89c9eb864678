"""GPU parity of the compress entry points at every pointer phase, at tiny
buckets and at the edges of the kernels' chunks.

The other compress tests hand the kernels freshly allocated (256-byte aligned)
buffers of exactly k slots.  Here source, index and value buffers are carved
out of sentinel-filled allocations at chosen 16-byte phases (tests/geometry.py):
the emitters' scalar branches, top-k's element-wise source reads and the
16-byte source loads at dword phases run, and a store past either end of an
output is seen.  Every comparison is bit for bit with the oracle (count, whole
stream, state); after every call the guards of source, index and value buffer
are intact and, without error feedback, the source is unchanged.  The tables
are pinned by tests/test_geometry_host.py.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import geometry as G
from geometry import assert_guards, carve
from parity import assert_same_stream, assert_topk_values, bits, canon_nan

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(torch, view, x):
    view.copy_(torch.from_numpy(np.array(x, np.float32)))


def _outputs(torch, gpu, k, phases):
    return carve(torch, gpu, k, torch.int32, phases[1]), carve(torch, gpu, k, torch.float32, phases[2])


def _check_call(what, src, x, idx, val, cg, co, io, vo, src_expect=None):
    """One call's results: count, stream, guards, and the source (unchanged
    unless `src_expect` says what error feedback leaves)."""
    assert int(cg) == co, (what, int(cg), co)
    assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, co, what)
    assert_guards(idx, f"{what}: idx")
    assert_guards(val, f"{what}: val")
    assert_guards(src, f"{what}: src")
    want = x if src_expect is None else src_expect
    assert np.array_equal(bits(src.cpu().numpy()), bits(want)), f"{what}: source bucket differs"


def _same_state(got, exp, what):
    assert got is not None, what
    g, e = np.array(got, np.float32).ravel(), np.array(exp, np.float32).ravel()
    assert canon_nan(g).tolist() == canon_nan(e).tolist(), (what, got, exp)


def _tv16_key_sequence(torch, gpu, comp, key, seq, k, phases, off=0, what=""):
    """One thresholdv16 key through the calls of `seq` (geometry.tv16_sequence)."""
    n = seq[0][0].size
    src = carve(torch, gpu, n, torch.float32, phases[0])
    idx, val = _outputs(torch, gpu, k, phases)
    for it, (x, co, io, vo, st, _head, _regime) in enumerate(seq):
        _load(torch, src, x)
        idx.zero_()
        val.zero_()
        cg = comp.compress(key, src, k, idx, val, off)
        _check_call(f"{what} n={n} k={k} phases={phases} call {it}", src, x, idx, val, cg, co, io, vo)
        _same_state(comp.state(key), st, (what, n, k, it))
    return src, idx, val


# ---------------------------------------------------------------------------
# A. thresholdv16, one-bucket calls
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("phases", G.TRIPLES_A, ids=lambda p: "-".join(map(str, p)))
@pytest.mark.parametrize("size", range(len(G.SIZES_A)), ids=[str(n) for n, _ in G.SIZES_A])
def test_thresholdv16_phases(gpu, oracle, size, phases):
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    n, k = G.SIZES_A[size]
    seq = G.tv16_sequence(oracle, n, k, G.BUCKET_A + size, G.SCALES8)
    comp = ThresholdvCompressor16()
    _tv16_key_sequence(torch, gpu, comp, "a@w", seq, k, phases, what="A")
    comp.check_device()


def test_thresholdv16_phases_idx_offset(gpu, oracle):
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    (n, k), phases, off = G.OFFSET_RUN_A
    seq = G.tv16_sequence(oracle, n, k, G.BUCKET_A + G.SIZES_A.index((n, k)), G.SCALES8, off=off)
    comp = ThresholdvCompressor16()
    _tv16_key_sequence(torch, gpu, comp, "a@w", seq, k, phases, off=off, what="A+offset")
    comp.check_device()


# ---------------------------------------------------------------------------
# B. every way of finishing and ordering the fill, in a child process each
# ---------------------------------------------------------------------------
def _production(out):
    assert out["scan_ranked"][1] > 0, out  # ranked with ties in the scan launch
    assert out["stale"] == 0, out
    assert out["paths"][3] == 0, out       # never the literal heap
    leader, crew, leader_lit, crew_lit = out["wide"]
    assert crew > 0 and leader_lit == 0 and crew_lit == 0, out


def _lfin_only(out):
    assert out["stale"] == 0, out
    plain, tied, viol, notake = out["lfin"]
    assert tied > 0, out
    assert out["paths"][3] == 0, out
    leader, crew, leader_lit, crew_lit = out["wide"]
    assert crew > 0 and leader_lit == 0 and crew_lit == 0, out


def _batched_lone_fill(out):
    none, by_start, shadow, literal = out["paths"]
    assert by_start > 0 and literal == 0, out


def _orderer_alone(out):
    none, by_start, shadow, literal = out["paths"]
    assert by_start > 0 and literal == 0, out
    assert out["lfin"] == [0, 0, 0, 0], out


def _shadow(out):
    none, by_start, shadow, literal = out["paths"]
    assert by_start == 0 and shadow > 0 and literal == 0, out


def _literal(out):
    none, by_start, shadow, literal = out["paths"]
    assert by_start == 0 and shadow == 0 and literal > 0, out
    assert out["wide"] == [0, 0, 0, 0], out


def _leader(out):
    none, by_start, shadow, literal = out["paths"]
    leader, crew, leader_lit, crew_lit = out["wide"]
    assert by_start == 0 and shadow == 0 and literal == 0, out
    assert leader > 0 and crew > 0 and leader_lit == 0 and crew_lit == 0, out


def _crew(out):
    none, by_start, shadow, literal = out["paths"]
    leader, crew, leader_lit, crew_lit = out["wide"]
    assert literal == 0 and leader == 0 and crew > 0 and crew_lit == 0, out


# mode -> (environment, the path-counter assertions tests/test_gpu_fill_modes.py makes for it)
FILL_MODES = {
    "production": ({}, _production),
    "lfin_only": ({"STG_TV16_LF2": "0"}, _lfin_only),
    "batched_lone_fill": ({"STG_TV16_LFIN": "0"}, _batched_lone_fill),
    "orderer_alone": ({"STG_TV16_LFIN_RANKERS": "0", "STG_TV16_LF2": "0"}, _orderer_alone),
    "shadow_heap": ({"STG_DEBUG_TV16_FILL": "1"}, _shadow),
    "literal_heap": ({"STG_DEBUG_TV16_FILL": "2"}, _literal),
    "leader": ({"STG_DEBUG_TV16_FILL": "3"}, _leader),
    "crew": ({"STG_DEBUG_TV16_FILL": "4"}, _crew),
}


@pytest.mark.parametrize("phases", G.TRIPLES_CHILD, ids=lambda p: "-".join(map(str, p)))
@pytest.mark.parametrize("mode", list(FILL_MODES))
def test_fill_modes_phases(gpu, mode, phases):
    """tests/phase_child.py checks every call against the oracle with carved
    buffers; the counters show that the forced path is the one that ran."""
    env, expect = FILL_MODES[mode]
    env = dict(os.environ, **{"STG_DEBUG_TV16_FILL": "0", **env})
    r = subprocess.run([sys.executable, os.path.join(HERE, "phase_child.py"), *map(str, phases)],
                       capture_output=True, text=True, timeout=110, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    assert out["phases"] == list(phases)
    print(line)  # the counters, whole, beside a failed assertion
    expect(out)


# ---------------------------------------------------------------------------
# C. batched launches
# ---------------------------------------------------------------------------
def test_thresholdv16_batch_phases(gpu, oracle):
    """Nine buckets, a phase triple each, one key twice (the launch splits)."""
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    items = tuple(b[:5] for b in G.BATCH_C)
    seq = G.tv16_batch_sequence(oracle, items, G.SCALES, G.BUCKET_C)
    comp = ThresholdvCompressor16()
    bufs = [(carve(torch, gpu, n, torch.float32, ph[0]),) + _outputs(torch, gpu, k, ph)
            for _, n, k, _, _, ph in G.BATCH_C]
    for it, row in enumerate(seq):
        for (src, idx, val), r in zip(bufs, row):
            _load(torch, src, r[0])
            idx.zero_()
            val.zero_()
        counts = comp.compress_batch_async(
            [(key, src, k, idx, val, off) for (key, _, k, _, off, _), (src, idx, val) in zip(G.BATCH_C, bufs)])
        torch.cuda.synchronize()
        counts = counts.cpu().numpy()
        last = {}
        for j, ((key, n, k, _, off, ph), (src, idx, val), (x, co, io, vo, st, *_)) in enumerate(zip(G.BATCH_C, bufs, row)):
            _check_call(f"C call {it} bucket {j} ({key}, n={n}, phases={ph})", src, x, idx, val, counts[j], co, io, vo)
            last[key] = st
        for key, st in last.items():
            _same_state(comp.state(key), st, (it, key))
    comp.check_device()


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.itemsize == 2 else a.view(np.uint32)


def test_thresholdv16_wire_batch_phases(gpu, oracle):
    """The wire-form emission, every flag, the 16-bit outputs at 2-byte phases:
    the bytes of oracle.wire_encode of the oracle's stream."""
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    items = tuple((key, n, k, dist, off) for key, n, k, dist, _, off, _ in G.WIRE_C)
    seq = G.tv16_batch_sequence(oracle, items, G.SCALES, G.BUCKET_W)
    comp = ThresholdvCompressor16()
    bufs = []
    for _, n, k, _, flag, _, ph in G.WIRE_C:
        bufs.append((carve(torch, gpu, n, torch.float32, ph[0]),
                     carve(torch, gpu, k, torch.int16 if flag & 1 else torch.int32, ph[1]),
                     carve(torch, gpu, k, torch.int16 if flag & 2 else torch.float32, ph[2])))
    flags = [b[4] for b in G.WIRE_C]
    for it, row in enumerate(seq):
        for (src, di, dv), r in zip(bufs, row):
            _load(torch, src, r[0])
            di.fill_(-1)
            dv.fill_(-1)
        counts = comp.compress_batch_async(
            [(key, src, k, di, dv, off) for (key, _, k, _, _, off, _), (src, di, dv) in zip(G.WIRE_C, bufs)],
            wire_flags=flags)
        torch.cuda.synchronize()
        counts = counts.cpu().numpy()
        for j, ((key, n, k, _, flag, off, ph), (src, di, dv), (x, co, io, vo, st, *_)) in enumerate(zip(G.WIRE_C, bufs, row)):
            what = f"wire call {it} bucket {j} ({key}, n={n}, flag={flag}, phases={ph})"
            assert int(counts[j]) == co, what
            oi, ov = oracle.wire_encode(io[:co], vo[:co], flag)
            assert np.array_equal(_u(di.cpu().numpy())[:co], _u(oi)), what
            assert np.array_equal(_u(dv.cpu().numpy())[:co], _u(ov)), what
            for v, name in ((di, "idx"), (dv, "val"), (src, "src")):
                assert_guards(v, f"{what}: {name}")
            assert np.array_equal(bits(src.cpu().numpy()), bits(x)), f"{what}: source bucket differs"
            _same_state(comp.state(key), st, what)
    comp.check_device()


def test_thresholdv16_residual_batch_phases(gpu, oracle):
    """MERGE compress with error feedback: the residuals at every dword phase
    end as the oracle's copy-then-zero (compress.cpp:178-185), the bucket too."""
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    items = tuple((key, n, k, G.D1, 0) for key, n, k, _, _ in G.RESID_C)
    seq = G.tv16_batch_sequence(oracle, items, G.SCALES4, G.BUCKET_R)
    comp = ThresholdvCompressor16()
    bufs = [(carve(torch, gpu, n, torch.float32, ph[0]),) + _outputs(torch, gpu, k, ph) +
            (carve(torch, gpu, n, torch.float32, rp),) for _, n, k, ph, rp in G.RESID_C]
    for it, row in enumerate(seq):
        for (src, idx, val, res), r in zip(bufs, row):
            _load(torch, src, r[0])
            idx.zero_()  # compress.cpp:60-64: unwritten slots hold index 0
            val.zero_()
            res.fill_(7.0)
        counts = comp.compress_batch_async(
            [(key, src, k, idx, val) for (key, _, k, _, _), (src, idx, val, _) in zip(G.RESID_C, bufs)],
            residuals=[b[3] for b in bufs])
        torch.cuda.synchronize()
        counts = counts.cpu().numpy()
        for j, ((key, n, k, ph, rp), (src, idx, val, res), (x, co, io, vo, st, *_)) in enumerate(zip(G.RESID_C, bufs, row)):
            what = f"resid call {it} bucket {j} (n={n}, phases={ph}, residual phase {rp})"
            expect = np.array(x, np.float32)
            expect[io[:k]] = 0.0
            _check_call(what, src, x, idx, val, counts[j], co, io, vo, src_expect=expect)
            assert np.array_equal(bits(res.cpu().numpy()), bits(expect)), f"{what}: residual differs"
            assert_guards(res, f"{what}: residual")
            _same_state(comp.state(key), st, what)
    comp.check_device()


# ---------------------------------------------------------------------------
# D. threshold-v and top-k
# ---------------------------------------------------------------------------
def _tv_key_sequence(torch, gpu, comp, seq, k, phases, what, keep):
    """Threshold-v keys its state by the source pointer: one carved source per
    sequence, kept alive in `keep` so that no later one gets its address."""
    n = seq[0][0].size
    src = carve(torch, gpu, n, torch.float32, phases[0])
    idx, val = _outputs(torch, gpu, k, phases)
    keep.append(src)
    for it, (x, co, io, vo, t_after, _above) in enumerate(seq):
        _load(torch, src, x)
        idx.zero_()
        val.zero_()
        cg = comp.compress("ignored", src, k, idx, val)
        _check_call(f"{what} n={n} k={k} phases={phases} call {it}", src, x, idx, val, cg, co, io, vo)
        _same_state(comp.state("", key_ptr=src.data_ptr())[:1], [t_after], (what, n, k, it))


@pytest.mark.parametrize("phases", G.TRIPLES_D, ids=lambda p: "-".join(map(str, p)))
@pytest.mark.parametrize("size", range(len(G.TV_D)), ids=[str(n) for n, _ in G.TV_D])
def test_thresholdv_phases(gpu, oracle, size, phases):
    import torch
    from stellatrain_amd import ThresholdvCompressor
    n, k = G.TV_D[size]
    seq = G.tv_sequence(oracle, n, k, G.BUCKET_D + size, G.SCALES_TV)
    comp = ThresholdvCompressor()
    _tv_key_sequence(torch, gpu, comp, seq, k, phases, "D", [])
    comp.check_device()


def _topk_key_calls(torch, gpu, oracle, comp, key, n, k, bucket, phases, exact, what, calls=2):
    """A key's first call and the hinted single-read calls after it (topk1.hip)."""
    src = carve(torch, gpu, n, torch.float32, phases[0])
    idx, val = _outputs(torch, gpu, k, phases)
    off = 77 if exact else 0
    for it in range(calls):
        x, co, io, vo = G.topk_call(oracle, n, k, bucket, it, exact, off)
        _load(torch, src, x)
        idx.zero_()
        val.zero_()
        cg = comp.compress(key, src, k, idx, val, off)
        w = f"{what} n={n} k={k} phases={phases} call {it}"
        assert cg == co == k, w
        if exact:
            assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, k, w)
        else:
            np.testing.assert_array_equal(idx.cpu().numpy(), np.arange(k))
            assert_topk_values(val.cpu().numpy(), vo[:k])
        for v, name in ((idx, "idx"), (val, "val"), (src, "src")):
            assert_guards(v, f"{w}: {name}")
        assert np.array_equal(bits(src.cpu().numpy()), bits(x)), f"{w}: source bucket differs"
    return src


@pytest.mark.parametrize("phases", G.TRIPLES_D, ids=lambda p: "-".join(map(str, p)))
@pytest.mark.parametrize("size", range(len(G.TOPK_D)), ids=[f"{n}-{k}" for n, k in G.TOPK_D])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "bug_compat"])
def test_topk_phases(gpu, oracle, exact, size, phases):
    import torch
    from stellatrain_amd import TopkCompressor
    n, k = G.TOPK_D[size]
    comp = TopkCompressor(exact=exact)
    _topk_key_calls(torch, gpu, oracle, comp, "t@w", n, k, G.BUCKET_D + 5 + size, phases, exact, "D")
    comp.check_device()


# ---------------------------------------------------------------------------
# E. tiny buckets and sizes at the edges of the kernels' geometry
# ---------------------------------------------------------------------------
E_CASES = ([("thresholdv16", f) for f in G.FAMILIES] + [("thresholdv", f) for f in G.TV_FAMILIES] +
           [("topk_exact", f) for f in G.FAMILIES] + [("topk", "tiny")])


@pytest.mark.parametrize("phases", G.TRIPLES_E, ids=lambda p: "-".join(map(str, p)))
@pytest.mark.parametrize("codec,family", E_CASES, ids=[f"{c}-{f}" for c, f in E_CASES])
def test_size_family(gpu, oracle, codec, family, phases):
    import torch
    from stellatrain_amd import make_compressor
    comp = make_compressor(codec)
    keep = []
    for j, (n, k) in enumerate(G.family_cases(codec, family)):
        bucket = G.family_bucket(family, j)
        what = f"E {codec} {family}"
        if codec == "thresholdv16":
            seq = G.tv16_sequence(oracle, n, k, bucket, G.SCALES4)
            keep.append(_tv16_key_sequence(torch, gpu, comp, f"e{j}@w", seq, k, phases, what=what))
        elif codec == "thresholdv":
            _tv_key_sequence(torch, gpu, comp, G.tv_sequence(oracle, n, k, bucket, G.SCALES_TV4), k, phases, what, keep)
        else:
            # (the hinted second call at the tiny sizes only: section D has it at size)
            keep.append(_topk_key_calls(torch, gpu, oracle, comp, f"e{j}@w", n, k, bucket, phases,
                                        codec == "topk_exact", what, calls=2 if family == "tiny" else 1))
    comp.check_device()
