"""GPU parity on buckets whose large values cluster by position
(tests/layered.py).

Every other input of the suite is spatially stationary, so a 512-line chunk, an
8,192-element tile or a heap subtree never holds more of the large values
than its neighbours.  Here some chunks overflow their lists while the ones
beside them are empty, the output limit falls inside an overflowing chunk, all
qualifying lines sit in the first or the last chunk, and the regime-B pops are
parents, children and siblings of each other in the heap, with long runs of
equal sums.  tests/test_layered_host.py asserts, with the oracle alone, that
the inputs do that; tests/test_oracle_golden_layered.py pins the oracle to the
reference on them.  Every comparison here is bit for bit against the oracle:
count, whole stream in order, state bits, residual, parameters and optimizer
state.  Only the shipped top-k mode, whose order the reference leaves open,
compares values as a multiset (assert_topk_values).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import layered as ly
import publish_cases as P
import wire_merge_cases as W
from chain_helpers import Optim, debug_words, merged, oracle_send, state_bits, u
from geometry import assert_guards, carve
from parity import assert_same_stream, assert_topk_values, fbits
from stellatrain_amd.synth import D1, seed_for, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MID, BIG = ly.SIZES[1], ly.SIZES[2]
ENTRY_KINDS = ("front", "ramp", "moving")


def _same_words(got, exp, what):
    """Equal 16- or 32-bit words; a mismatch names how many differ, where the
    first and the last of them are and what stands there."""
    got, exp = u(got), u(exp)
    assert got.dtype == exp.dtype and got.size == exp.size, what
    bad = np.flatnonzero(got != exp)
    if bad.size:
        f, l = int(bad[0]), int(bad[-1])
        raise AssertionError(f"{what}: {bad.size} of {exp.size} words differ, positions {f} .. {l}; got "
                             f"{got[f:f + 4].tolist()} .. {got[max(l - 3, 0):l + 1].tolist()}, expected "
                             f"{exp[f:f + 4].tolist()} .. {exp[max(l - 3, 0):l + 1].tolist()}")


def _x(kind, n, it):
    return ly.layered_input(kind, n, ly.seed_bucket_of(kind), it)


@pytest.fixture(scope="module")
def chain(oracle):
    """chain(kind, n): the oracle's CALLS calls on one key, computed once:
    [(x, count, idx, val, state after, threshold before)]."""
    memo = {}

    def get(kind, n):
        if (kind, n) not in memo:
            h = oracle.tv16_new()
            rows = []
            for it in range(ly.CALLS):
                x = _x(kind, n, it) if kind != "plain" else synth(n, seed_for(ly.SEED_BUCKET + 99, it), D1)
                tb = oracle.tv16_state(h, "c")
                co, io, vo = oracle.tv16_compress(h, "c", x, ly.K[n])
                rows.append((x, co, io, vo, oracle.tv16_state(h, "c"), tb[0] if tb else None))
            oracle.tv16_free(h)
            memo[(kind, n)] = rows
        return memo[(kind, n)]
    return get


# ---------------------------------------------------------------------------
# thresholdv16, one-bucket calls
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", ly.SIZES)
@pytest.mark.parametrize("kind", ly.KINDS)
def test_tv16_one_bucket(gpu, oracle, chain, kind, n):
    """CALLS calls on one key; exactly k slots, carved so that a store past
    them is seen.  Prints per call which fill way ran (debug words 44-59)."""
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    comp = ThresholdvCompressor16()
    k = ly.K[n]
    d = torch.empty(n, dtype=torch.float32, device=gpu)
    w0 = debug_words(comp, gpu)
    for it, (x, co, io, vo, so, tb) in enumerate(chain(kind, n)):
        d.copy_(torch.from_numpy(x))
        idx = carve(torch, gpu, k, torch.int32, 0)
        val = carve(torch, gpu, k, torch.float32, 0)
        idx.zero_()
        val.zero_()
        cnt = comp.compress("5@weight", d, k, idx, val)
        regime = "-" if tb is None else "B" if so[0] < tb else "A"
        what = f"{kind}, n {n}, call {it}, regime {regime}"
        assert cnt == co, what
        assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, co, what)
        assert state_bits(comp.state("5@weight")) == state_bits(so), what
        assert_guards(idx, "idx: " + what)
        assert_guards(val, "val: " + what)
        assert np.array_equal(u(d.cpu().numpy()), u(x)), "the bucket changed: " + what
        w1 = debug_words(comp, gpu)
        dw = [a - b for a, b in zip(w1, w0)]
        w0 = w1
        print(json.dumps({"kind": kind, "n": n, "it": it, "regime": regime, "scan_ranked": dw[44:46], "lfin": dw[48:52],
                          "leader": dw[52], "crew": dw[53], "leader_literal": dw[54], "crew_literal": dw[55],
                          "paths": dw[56:60]}))
    comp.check_device()


# ---------------------------------------------------------------------------
# thresholdv16, batched: overflowing, empty and ordinary chunks in one launch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [MID, BIG])
def test_tv16_batched(gpu, oracle, chain, n):
    """One launch per call holds one key of each kind and one plain D1 key."""
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    comp = ThresholdvCompressor16()
    kinds = ly.KINDS + ("plain",)
    k = ly.K[n]
    src = [torch.empty(n, dtype=torch.float32, device=gpu) for _ in kinds]
    for it in range(ly.CALLS):
        items = []
        for j, kind in enumerate(kinds):
            src[j].copy_(torch.from_numpy(chain(kind, n)[it][0]))
            items.append((f"{kind}@weight", src[j], k, torch.full((k,), -1, dtype=torch.int32, device=gpu),
                          torch.full((k,), -1, dtype=torch.float32, device=gpu)))
        counts = comp.compress_batch_async(items)
        torch.cuda.synchronize()
        got = counts.cpu().numpy().tolist()
        for j, kind in enumerate(kinds):
            x, co, io, vo, so, _ = chain(kind, n)[it]
            what = f"batched, n {n}, launch {it}, key {kind}"
            assert got[j] == co, what
            assert_same_stream(items[j][3].cpu().numpy().view(np.uint32), items[j][4].cpu().numpy(), io, vo, co, what)
            assert state_bits(comp.state(f"{kind}@weight")) == state_bits(so), what
            assert np.array_equal(u(src[j].cpu().numpy()), u(x)), "bucket: " + what
    comp.check_device()
    w = debug_words(comp, gpu)
    print(json.dumps({"batched": n, "scan_ranked": w[44:46], "lfin": w[48:52], "wide": w[52:56], "paths": w[56:60]}))


# ---------------------------------------------------------------------------
# the other entry points
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ENTRY_KINDS)
def test_merge_compress_with_error_feedback(gpu, oracle, kind):
    """The MERGE compress with the residual carried into the next call's
    bucket: what was not sent accumulates where the large values are."""
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    comp = ThresholdvCompressor16()
    ho = oracle.tv16_new()
    n, k = MID, ly.K[MID]
    d = torch.empty(n, dtype=torch.float32, device=gpu)
    res_d = torch.zeros(n, dtype=torch.float32, device=gpu)
    res = np.zeros(n, np.float32)
    try:
        for it in range(ly.CALLS):
            x = (_x(kind, n, it) + res).astype(np.float32)
            co, io, vo = oracle.tv16_compress(ho, "r@weight", x, k)
            res = x.copy()
            res[io[:k]] = 0  # all k slots (compress.cpp:178-179)
            d.copy_(torch.from_numpy(x))
            di = torch.full((k,), -1, dtype=torch.int32, device=gpu)
            dv = torch.full((k,), -1, dtype=torch.float32, device=gpu)
            counts = comp.compress_batch_async([("r@weight", d, k, di, dv)], residuals=[res_d])
            torch.cuda.synchronize()
            what = f"error feedback, {kind}, call {it}"
            assert counts.cpu().numpy().tolist() == [co], what
            assert_same_stream(di.cpu().numpy().view(np.uint32), dv.cpu().numpy(), io, vo, co, what)
            assert state_bits(comp.state("r@weight")) == state_bits(oracle.tv16_state(ho, "r@weight")), what
            assert np.array_equal(u(d.cpu().numpy()), u(res)), "bucket: " + what
            assert np.array_equal(u(res_d.cpu().numpy()), u(res)), "residual: " + what
        comp.check_device()
    finally:
        oracle.tv16_free(ho)


@pytest.mark.parametrize("kind", ENTRY_KINDS)
def test_wire_emission(gpu, oracle, chain, kind):
    """Four keys on the same inputs, one per wire flag, in one launch: four
    buckets that make the same decisions at the same time, so a window miss
    puts all four into the crew at once."""
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    comp = ThresholdvCompressor16()
    n, k = MID, ly.K[MID]
    d = torch.empty(n, dtype=torch.float32, device=gpu)
    for it, (x, co, io, vo, so, _) in enumerate(chain(kind, n)):
        d.copy_(torch.from_numpy(x))
        items = [(f"w{f}@weight", d, k, torch.full((k,), -1, dtype=torch.int16 if f & 1 else torch.int32, device=gpu),
                  torch.full((k,), -1, dtype=torch.int16 if f & 2 else torch.float32, device=gpu)) for f in range(4)]
        counts = comp.compress_batch_async(items, wire_flags=[0, 1, 2, 3])
        torch.cuda.synchronize()
        assert counts.cpu().numpy().tolist() == [co] * 4, (kind, it)
        for f in range(4):
            wi, wv = oracle.wire_encode(io[:co], vo[:co], f)
            what = f"wire flag {f}, {kind}, call {it}"
            _same_words(items[f][3].cpu().numpy()[:co], wi, "indices: " + what)
            _same_words(items[f][4].cpu().numpy()[:co], wv, "values: " + what)
            assert state_bits(comp.state(f"w{f}@weight")) == state_bits(so), what
    comp.check_device()


def _other(kind):
    return "back" if kind != "back" else "front"


@pytest.mark.parametrize("kind", ENTRY_KINDS)
def test_gather_fused(gpu, oracle, kind):
    """N = 2 sources whose hot regions differ (the second is `back`), and a
    residual: the sum has two hot regions, the later calls three."""
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    comp = ThresholdvCompressor16()
    ho = oracle.tv16_new()
    n, k = MID, ly.K[MID]
    res_d = torch.zeros(n, dtype=torch.float32, device=gpu)
    res = np.zeros(n, np.float32)
    try:
        for it in range(ly.CALLS):
            srcs = [_x(kind, n, it), _x(_other(kind), n, it)]
            g = [torch.from_numpy(s).to(gpu) for s in srcs]
            di = torch.zeros(k, dtype=torch.int32, device=gpu)
            dv = torch.zeros(k, dtype=torch.float32, device=gpu)
            cnt = comp.merge_gather_compress_async("g@weight", g, k, di, dv, residual=res_d)
            torch.cuda.synchronize()
            x = ((srcs[0] + res).astype(np.float32) + srcs[1]).astype(np.float32)
            co, io, vo = oracle.tv16_compress(ho, "g@weight", x, k)
            res = x.copy()
            res[io[:k]] = 0
            what = f"fused gather, {kind}, call {it}"
            assert int(cnt.item()) == co, what
            assert_same_stream(di.cpu().numpy().view(np.uint32), dv.cpu().numpy(), io, vo, co, what)
            assert state_bits(comp.state("g@weight")) == state_bits(oracle.tv16_state(ho, "g@weight")), what
            assert np.array_equal(u(g[0].cpu().numpy()), u(res)), "grad[0]: " + what
            assert np.array_equal(u(res_d.cpu().numpy()), u(res)), "residual: " + what
        comp.check_device()
    finally:
        oracle.tv16_free(ho)


@pytest.mark.parametrize("fp16_values", [False, True])
def test_send_buckets(gpu, oracle, fp16_values):
    """CodecEngine.send_buckets: one tensor per kind, two sources each and a
    residual; grad[0], residual, wire bytes, count and state."""
    import torch
    from stellatrain_amd import CodecEngine, wire_flag
    eng = CodecEngine()
    eng.configure_compression_ratio(0.99)
    ho = oracle.tv16_new()
    n, k = MID, ly.K[MID]
    flag = wire_flag(n, fp16_values)
    keys = [f"{kind}@weight" for kind in ENTRY_KINDS]
    g = [[torch.zeros(n, dtype=torch.float32, device=gpu) for _ in range(2)] for _ in ENTRY_KINDS]
    res = [torch.zeros(n, dtype=torch.float32, device=gpu) for _ in ENTRY_KINDS]
    res_np = [np.zeros(n, np.float32) for _ in ENTRY_KINDS]
    try:
        for it in range(ly.CALLS):
            srcs = [[_x(kind, n, it), _x(_other(kind), n, it)] for kind in ENTRY_KINDS]
            for j in range(len(keys)):
                for t, x in zip(g[j], srcs[j]):
                    t.copy_(torch.from_numpy(x))
            streams, counts = eng.send_buckets([(keys[j], g[j], res[j]) for j in range(len(keys))],
                                               fp16_values=fp16_values)
            torch.cuda.synchronize()
            cg = counts.cpu().numpy().tolist()
            for j, kind in enumerate(ENTRY_KINDS):
                what = f"send, {kind}, call {it}, flag {flag}"
                x, co, wi, wv = oracle_send(oracle, ho, keys[j], srcs[j], res_np[j], k, flag)
                res_np[j] = x.copy()
                di, dv, fl = streams[j]
                assert fl == flag and di.numel() == k and cg[j] == co, what
                assert np.array_equal(u(g[j][0].cpu().numpy()), u(x)), "grad[0]: " + what
                assert np.array_equal(u(res[j].cpu().numpy()), u(x)), "residual: " + what
                assert np.array_equal(u(di.cpu().numpy())[:co], u(wi)), "wire indices: " + what
                assert np.array_equal(u(dv.cpu().numpy())[:co], u(wv)), "wire values: " + what
                assert state_bits(eng.compressor().state(keys[j])) == state_bits(oracle.tv16_state(ho, keys[j])), what
        eng.compressor().check_device()
    finally:
        oracle.tv16_free(ho)


# ---------------------------------------------------------------------------
# the forced fill modes, each in a fresh child process
# ---------------------------------------------------------------------------
_child_failed = []


@pytest.mark.parametrize("env", [{}, {"STG_DEBUG_TV16_FILL": "1"}, {"STG_DEBUG_TV16_FILL": "2"},
                                 {"STG_DEBUG_TV16_FILL": "3"}, {"STG_DEBUG_TV16_FILL": "4"}, {"STG_TV16_LFIN": "0"},
                                 {"STG_TV16_LF2": "0"}],
                         ids=["production", "shadow_heap", "literal_heap", "leader", "crew", "no_lfin", "no_lf2"])
def test_tv16_fill_modes(gpu, env):
    """ramp and plateau at 2^18 + 5 floats, one-bucket calls and a batched
    launch of both, under every forced fill mode (tests/fill_mode_child.py
    lists them) and without the one-bucket and the in-scan finish.  A child
    that failed stops the ones after it."""
    assert not _child_failed, f"not started: an earlier child failed ({_child_failed[0]})"
    full = dict(os.environ, **{"STG_DEBUG_TV16_FILL": "0", **env})
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "layered_fill_child.py")], capture_output=True,
                           text=True, timeout=110, env=full)
    except subprocess.TimeoutExpired:
        _child_failed.append(env)
        raise
    if r.returncode != 0:
        _child_failed.append(env)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps(out))
    assert out["ok"] and out["calls"] == 4 * ly.CALLS, out
    none, by_start, shadow, literal = out["paths"]
    leader, crew, leader_lit, crew_lit = out["wide"]
    mode = env.get("STG_DEBUG_TV16_FILL")
    if mode == "1":
        assert by_start == 0, out
    elif mode == "2":
        assert literal > 0 and by_start == 0 and shadow == 0 and out["wide"] == [0, 0, 0, 0], out
    elif mode == "3":
        # (with candidates this close in the heap the leader may give every call
        # up to the literal heap, word 54: DESIGN.md section 6d item 15)
        assert by_start == 0 and shadow == 0 and leader + leader_lit > 0, out
    elif mode == "4":
        assert leader == 0 and crew > 0, out
    elif "STG_TV16_LFIN" in env:
        assert out["lfin"] == [0, 0, 0, 0], out


# ---------------------------------------------------------------------------
# threshold-v
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", ly.TV_SIZES)
@pytest.mark.parametrize("kind", ly.TV_KINDS)
def test_thresholdv(gpu, oracle, kind, n):
    """front and back at 2^20 + 13 put all k qualifiers, more than a range
    lists, into the first or the last of 65 ranges."""
    import torch
    from stellatrain_amd import ThresholdvCompressor
    comp = ThresholdvCompressor()
    ho = oracle.tv_new()
    k = ly.K[n]
    d = torch.empty(n, dtype=torch.float32, device=gpu)
    try:
        for it in range(ly.CALLS):
            x = _x(kind, n, it)
            co, io, vo = oracle.tv_compress(ho, 1, x, k)
            d.copy_(torch.from_numpy(x))
            idx = carve(torch, gpu, k, torch.int32, 0)
            val = carve(torch, gpu, k, torch.float32, 0)
            idx.zero_()
            val.zero_()
            what = f"threshold-v, {kind}, n {n}, call {it}"
            assert comp.compress("ignored", d, k, idx, val) == co, what
            assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, co, what)
            assert fbits(comp.state("", key_ptr=d.data_ptr())[0]) == fbits(oracle.tv_state(ho, 1)), what
            assert_guards(idx, "idx: " + what)
            assert_guards(val, "val: " + what)
        comp.check_device()
    finally:
        oracle.tv_free(ho)


# ---------------------------------------------------------------------------
# top-k
# ---------------------------------------------------------------------------
def _topk_call(gpu, oracle, comp, key, x, k, bug_compat, what):
    import torch
    co, io, vo = oracle.topk_compress(x, k, bug_compat=bug_compat)
    idx = torch.zeros(k, dtype=torch.int32, device=gpu)
    val = torch.zeros(k, dtype=torch.float32, device=gpu)
    assert comp.compress(key, torch.from_numpy(x).to(gpu), k, idx, val, 0) == co, what
    if bug_compat:
        np.testing.assert_array_equal(idx.cpu().numpy(), np.arange(k), what)
        assert_topk_values(val.cpu().numpy(), vo)
    else:
        assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, k, what)


@pytest.mark.parametrize("kind", ly.TOPK_KINDS)
@pytest.mark.parametrize("bug_compat", [False, True], ids=["exact", "shipped"])
def test_topk(gpu, oracle, bug_compat, kind):
    """A first call and the hinted calls after it, at 9 and at 129 tiles: the
    elements at or above the k-th magnitude fill a few tiles far past the
    1,024 a tile lists and leave the others empty."""
    from stellatrain_amd import TopkCompressor
    for n in ly.TOPK_SIZES:
        comp = TopkCompressor(exact=not bug_compat)
        for it in range(ly.TOPK_CALLS):
            _topk_call(gpu, oracle, comp, "w", _x(kind, n, it), ly.K[n], bug_compat, f"top-k, {kind}, n {n}, call {it}")
        comp.check_device()
        w = debug_words(comp, gpu)
        print(json.dumps({"topk": kind, "n": n, "exact": not bug_compat, "band_hits": w[38], "select": w[39]}))


@pytest.mark.parametrize("bug_compat", [False, True], ids=["exact", "shipped"])
def test_topk_interleaved_keys(gpu, oracle, bug_compat):
    """Two keys whose hot regions differ, interleaved on one workspace."""
    from stellatrain_amd import TopkCompressor
    comp = TopkCompressor(exact=not bug_compat)
    n = BIG
    for it in range(ly.TOPK_CALLS):
        for kind in ("front", "back"):
            _topk_call(gpu, oracle, comp, kind, _x(kind, n, it), ly.K[n], bug_compat,
                       f"top-k interleaved, {kind}, call {it}")
    comp.check_device()


# ---------------------------------------------------------------------------
# receive side: a closed loop of 2 and of 3 ranks
# ---------------------------------------------------------------------------
LOOPS = {"shared_front": ("front", "front", "front"), "shared_moving": ("moving", "moving", "moving"),
         "disjoint": ("front", "back", "straddle")}


def _rank_input(kind, q, n, it):
    """Rank q's gradient: the kind's hot region, the rank's own values."""
    return ly.layered_input(kind, n, ly.seed_bucket_of(kind) + 100 * (q + 1), it)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("loop", list(LOOPS))
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_closed_loop(gpu, oracle, opt, loop, world):
    """Each rank sends (send_buckets with a residual); every rank's wire
    output goes, in place, to scatter_merge_wire, to merge_optimize_wire on one
    parameter and through merge_optimize_batch on a twin, then publish_params
    to a bfloat16 replica.  The indices are contiguous runs: full 4,096-mark
    tiles that hold a rank's whole stream beside empty ones, the ranks' runs the
    same (shared) or apart (disjoint).  Streams, merged stream, parameters, optimizer state and the
    replica against the oracle chain."""
    import torch
    from stellatrain_amd import CodecEngine, MergeTasks, PublishTasks, publish_params, scatter_merge_wire, wire_flag
    from stellatrain_amd.engine import scatter_merge_check
    n = MID
    k = ly.merge_k(n, world)
    flag = wire_flag(n)
    kinds = LOOPS[loop][:world]
    eng = [CodecEngine() for _ in range(world)]
    for e in eng:
        e.configure_compression_ratio(0.99)
    one, many = Optim(oracle, opt), Optim(oracle, opt)
    ho = [oracle.tv16_new() for _ in range(world)]
    p0 = synth(n, seed_for(ly.SEED_BUCKET + 98, 0), D1) * np.float32(100)
    po_one, po_many = p0.copy(), p0.copy()
    pd_one, pd_many = torch.from_numpy(p0).to(gpu), torch.from_numpy(p0).to(gpu)
    rep = pd_many.to(torch.bfloat16)
    g = [[torch.zeros(n, dtype=torch.float32, device=gpu)] for _ in range(world)]
    res = [torch.zeros(n, dtype=torch.float32, device=gpu) for _ in range(world)]
    res_np = [np.zeros(n, np.float32) for _ in range(world)]
    try:
        for it in range(ly.CALLS):
            srcs, sent = [], []
            for q in range(world):
                srcs.append([_rank_input(kinds[q], q, n, it)])
                g[q][0].copy_(torch.from_numpy(srcs[q][0]))
                sent.append(eng[q].send_buckets([("c@weight", g[q], res[q])], world=world))
            torch.cuda.synchronize()
            wire = []
            for q in range(world):
                what = f"closed loop {loop}, world {world}, call {it}, rank {q}"
                x, co, wi, wv = oracle_send(oracle, ho[q], "c@weight", srcs[q], res_np[q], k, flag)
                res_np[q] = x.copy()
                assert int(sent[q][1].cpu().numpy()[0]) == co == k, what
                assert np.array_equal(u(res[q].cpu().numpy()), u(x)), "residual: " + what
                assert np.array_equal(u(sent[q][0][0][0].cpu().numpy())[:co], u(wi)), "wire indices: " + what
                assert np.array_equal(u(sent[q][0][0][1].cpu().numpy())[:co], u(wv)), "wire values: " + what
                assert state_bits(eng[q].compressor().state("c@weight")) == \
                    state_bits(oracle.tv16_state(ho[q], "c@weight")), what
                wire.append((wi, wv, flag))
            what = f"closed loop {loop}, {opt}, world {world}, call {it}"
            ei, ev = W.expected(oracle, wire, k, n)[2:4]
            streams = [(sent[q][0][0][0][:k], sent[q][0][0][1][:k], flag) for q in range(world)]
            gi, gv = merged(scatter_merge_wire(streams, k, n))
            assert np.array_equal(gi, ei) and np.array_equal(gv, u(ev)), "scatter_merge_wire: " + what
            gi, gv = merged(one.dev.merge_optimize_wire(pd_one, "c@weight", streams, k))
            assert np.array_equal(gi, ei) and np.array_equal(gv, u(ev)), "merge_optimize_wire: " + what
            tasks = MergeTasks([(pd_many, "c@weight", streams, k)])
            gi, gv = merged(many.dev.merge_optimize_batch(tasks)[0])
            assert np.array_equal(gi, ei) and np.array_equal(gv, u(ev)), "merge_optimize_batch: " + what
            publish_params(PublishTasks.from_merge(tasks, [[rep]]))
            torch.cuda.synchronize()
            one.apply_oracle("c@weight", po_one, ev, ei)
            many.apply_oracle("c@weight", po_many, ev, ei)
            one.compare("c@weight", pd_one, po_one, "alone: " + what)
            many.compare("c@weight", pd_many, po_many, "batch: " + what)
            assert np.array_equal(rep.view(torch.int16).cpu().numpy().view(np.uint16), P.f32_to_bf16_bits(po_many)), \
                "replica: " + what
            # the runs: whole tiles of 4,096 marks beside empty ones
            per_tile = np.bincount(ei.astype(np.int64) // 4096, minlength=-(-n // 4096))
            assert per_tile.max() >= k // 2 and np.count_nonzero(per_tile) <= 2 * world, what
        scatter_merge_check()
        one.check()
        many.check()
        for e in eng:
            e.compressor().check_device()
    finally:
        for h in ho:
            oracle.tv16_free(h)
        one.close()
        many.close()
