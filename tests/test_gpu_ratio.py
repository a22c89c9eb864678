"""GPU parity when a key's k changes between calls (tests/ratio_cases.py).

The engine moves the compression ratio at run time and recomputes k per task,
while a key's threshold, increment, top-k hint and every buffer sized by an
earlier per_rank persist.  Each test walks one key (or one name) through
ratio changes -- 0.99, 0.9, 0.999, 0.5, 0.99, 0, 0.99 -- and compares every
call with the oracle bit for bit: count, the whole stream in order, state
bits, residual and bucket, parameters and optimizer state.  No tolerance
anywhere.  tests/test_oracle_golden_ratio.py pins the oracle to the reference
on the same table and asserts that the table reaches the fill's limits.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import publish_cases as P
import ratio_cases as rc
import wire_merge_cases as W
from chain_helpers import OPTS, Optim, debug_words, merged, oracle_send, state_bits, u
from geometry import assert_guards, carve
from parity import assert_same_stream, assert_topk_values, fbits
from stellatrain_amd.synth import D1, D3, seed_for, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# fill path counters (debug words): finished from the scan's window list ...
WINDOW_WORDS = (44, 45, 48, 49, 52, 56, 57, 58)
# ... or past it: the crew (53), the literal heap (59)
WIDE_WORDS = (53, 59)


# ---------------------------------------------------------------------------
# thresholdv16, one-bucket path
# ---------------------------------------------------------------------------
def _one_key(gpu, oracle, n, dist=D1, param=0, bucket=rc.SEED_BUCKET, ratios=None, window_rule=True):
    """The schedule on one key and one handle; returns the per-call report."""
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    comp = ThresholdvCompressor16()
    ho = oracle.tv16_new()
    key = "5@weight"
    d = torch.empty(n, dtype=torch.float32, device=gpu)
    report, wrong = [], []
    w0 = debug_words(comp, gpu)
    try:
        for it, r, k in rc.schedule(n, ratios=ratios):
            x = rc.ratio_input(n, it, dist, param, bucket)
            tb = oracle.tv16_state(ho, key)
            co, io, vo = oracle.tv16_compress(ho, key, x, k)
            so = oracle.tv16_state(ho, key)
            d.copy_(torch.from_numpy(x))
            idx = torch.zeros(k, dtype=torch.int32, device=gpu)
            val = torch.zeros(k, dtype=torch.float32, device=gpu)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cnt = comp.compress(key, d, k, idx, val)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            what = f"n {n}, call {it}: ratio {r}, k {k}"
            assert cnt == co, what
            assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, co, what)
            assert state_bits(comp.state(key)) == state_bits(so), what
            assert np.array_equal(u(d.cpu().numpy()), u(x)), "the bucket changed: " + what
            w1 = debug_words(comp, gpu)
            dw = [a - b for a, b in zip(w1, w0)]
            w0 = w1
            row = {"it": it, "ratio": r, "k": k, "ms": round(ms, 3), "regime": "-"}
            if tb is not None:
                row["regime"] = "B" if so[0] < tb[0] else "A"
            if row["regime"] == "B":
                q, head, m, window = rc.fill_probe(oracle, x, k, tb[0], co)
                win_fin, wide_fin = sum(dw[i] for i in WINDOW_WORDS), sum(dw[i] for i in WIDE_WORDS)
                row.update(M=m, window=window, past=m + 2 > window, scan_ranked=dw[44:46], lfin=dw[48:52],
                           leader=dw[52], crew=dw[53], leader_literal=dw[54], crew_literal=dw[55], paths=dw[56:60])
                # A window of M + 2 lines or more holds the pops, the entry
                # after them and a tie of it: the window list must finish the
                # call.  A window of fewer than M lines cannot hold the pops.
                # With M or M + 1 lines it holds every pop, and every line
                # outside it is strictly below every line inside: finishing
                # from the list is sound where its ties resolve, so either way
                # is right there and the stream alone decides.
                if window_rule and window < m and win_fin:
                    wrong.append(row)
                if window_rule and not row["past"] and (wide_fin or not win_fin):
                    wrong.append(row)
            print(row)
            report.append(row)
        comp.check_device()
    finally:
        oracle.tv16_free(ho)
    assert not wrong, f"window path against the host's prediction: {wrong}"
    return report


@pytest.mark.parametrize("n", rc.SIZES)
def test_tv16_one_bucket(gpu, oracle, n):
    """Every size, the whole schedule on one key.  A regime-B call that needs
    M lines from a window of fewer than M must not be finished from the window
    list; one whose window holds M + 2 or more must be (_one_key says why M and
    M + 1 are left to the stream).  Prints which of leader (52), crew (53) and
    literal heap (55 / 59) ran, and each call's time."""
    report = _one_key(gpu, oracle, n)
    b = [r for r in report if r["regime"] == "B"]
    print("n", n, "leader", sum(r["leader"] for r in b), "crew", sum(r["crew"] for r in b), "crew->literal",
          sum(r["crew_literal"] for r in b), "literal", sum(r["paths"][3] for r in b),
          "slowest ms", max(r["ms"] for r in report))
    if n > 4103:
        assert any(r["past"] for r in b) and any(not r["past"] for r in b)


# ---------------------------------------------------------------------------
# thresholdv16, batched: three entry points, keys at different points of RATIOS
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["plain", "residual", "wire"])
@pytest.mark.parametrize("n", rc.BATCH_SIZES)
def test_tv16_batched_staggered(gpu, oracle, n, entry):
    """6 keys per launch, key j 3 j entries ahead in RATIOS: one launch mixes a
    key whose k just grew, one whose k just shrank and steady ones.  plain:
    compress_batch; residual: the MERGE compress with error feedback, the
    residual carried into the next call's bucket; wire: flags 0-3."""
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    comp = ThresholdvCompressor16()
    ho = oracle.tv16_new()
    J = rc.BATCH_KEYS
    src = [torch.empty(n, dtype=torch.float32, device=gpu) for _ in range(J)]
    res_d = [torch.zeros(n, dtype=torch.float32, device=gpu) for _ in range(J)] if entry == "residual" else None
    res_np = [np.zeros(n, np.float32) for _ in range(J)]
    try:
        for step, row in enumerate(rc.batch_schedule(n)):
            items, exp, flags = [], [], []
            for j, (key, bucket, it, r, k) in enumerate(row):
                x = rc.ratio_input(n, it, bucket=bucket)
                if entry == "residual":
                    x = (x + res_np[j]).astype(np.float32)
                co, io, vo = oracle.tv16_compress(ho, key, x, k)
                flag = j % 4 if entry == "wire" else 0
                after = x
                if entry == "residual":
                    after = x.copy()
                    after[io[:k]] = 0  # all k slots (compress.cpp:178-179)
                    res_np[j] = after
                exp.append((co, oracle.wire_encode(io[:co], vo[:co], flag), oracle.tv16_state(ho, key), after))
                src[j].copy_(torch.from_numpy(x))
                di = torch.full((k,), -1, dtype=torch.int16 if flag & 1 else torch.int32, device=gpu)
                dv = torch.full((k,), -1, dtype=torch.int16 if flag & 2 else torch.float32, device=gpu)
                items.append((key, src[j], k, di, dv))
                flags.append(flag)
            counts = comp.compress_batch_async(items, residuals=res_d, wire_flags=flags if entry == "wire" else None)
            torch.cuda.synchronize()
            got = counts.cpu().numpy().tolist()
            for j, ((key, s, k, di, dv), (co, (wi, wv), so, after)) in enumerate(zip(items, exp)):
                what = f"{entry}, n {n}, launch {step}, key {j}: ratio {row[j][3]}, k {k}"
                assert got[j] == co, what
                ig, vg = u(di.cpu().numpy()), u(dv.cpu().numpy())
                bad = np.flatnonzero((ig[:co] != u(wi)) | (vg[:co] != u(wv)))
                assert not bad.size, f"{what}: {bad.size} of {co} pairs differ, first at {int(bad[0])}"
                assert state_bits(comp.state(key)) == state_bits(so), what
                assert np.array_equal(u(s.cpu().numpy()), u(after)), "bucket: " + what
                if entry == "residual":
                    assert np.array_equal(u(res_d[j].cpu().numpy()), u(after)), "residual: " + what
        comp.check_device()
        w = debug_words(comp, gpu)
        print(entry, n, "scan_ranked", w[44:46], "wide", w[52:56], "paths", w[56:60])
    finally:
        oracle.tv16_free(ho)


# ---------------------------------------------------------------------------
# D3: exact-zero lines tying at the cut of a large fill
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", rc.D3_SIZES)
def test_tv16_d3_one_bucket(gpu, oracle, n):
    report = _one_key(gpu, oracle, n, D3, rc.D3_ZP, rc.D3_SEED_BUCKET, rc.D3_RATIOS, window_rule=False)
    print("n", n, "slowest ms", max(r["ms"] for r in report))


def test_tv16_d3_batched(gpu, oracle):
    """Both D3 sizes as two keys of one batched launch per schedule entry."""
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    comp = ThresholdvCompressor16()
    ho = oracle.tv16_new()
    src = [torch.empty(n, dtype=torch.float32, device=gpu) for n in rc.D3_SIZES]
    try:
        for it, r in enumerate(rc.D3_RATIOS):
            items, exp = [], []
            for j, n in enumerate(rc.D3_SIZES):
                k = rc.merge_k(n, r)
                x = rc.ratio_input(n, it, D3, rc.D3_ZP, rc.D3_SEED_BUCKET)
                exp.append(oracle.tv16_compress(ho, f"z{j}@weight", x, k) + (oracle.tv16_state(ho, f"z{j}@weight"),))
                src[j].copy_(torch.from_numpy(x))
                items.append((f"z{j}@weight", src[j], k, torch.zeros(k, dtype=torch.int32, device=gpu),
                              torch.zeros(k, dtype=torch.float32, device=gpu)))
            counts = comp.compress_batch_async(items).cpu().numpy().tolist()
            torch.cuda.synchronize()
            for j, ((key, _, k, di, dv), (co, io, vo, so)) in enumerate(zip(items, exp)):
                what = f"D3 batched, call {it}, key {j}: ratio {r}, k {k}"
                assert counts[j] == co, what
                assert_same_stream(di.cpu().numpy().view(np.uint32), dv.cpu().numpy(), io, vo, co, what)
                assert state_bits(comp.state(key)) == state_bits(so), what
        comp.check_device()
        w = debug_words(comp, gpu)
        print("D3 batched: wide", w[52:56], "paths", w[56:60])
    finally:
        oracle.tv16_free(ho)


# ---------------------------------------------------------------------------
# the other finishes, each in a fresh child process
# ---------------------------------------------------------------------------
_child_failed = []


@pytest.mark.parametrize("env", [{"STG_TV16_LFIN": "0"}, {"STG_DEBUG_TV16_FILL": "1"}, {"STG_DEBUG_TV16_FILL": "2"},
                                 {"STG_DEBUG_TV16_FILL": "3"}, {"STG_DEBUG_TV16_FILL": "4"}],
                         ids=["batched_lone_fill", "shadow_heap", "literal_heap", "leader", "crew"])
def test_tv16_other_finishes(gpu, env):
    """The (1 << 18) + 5 schedule with the batched scan's lone fill
    (STG_TV16_LFIN=0) and with each forced fill mode of test_gpu_fill_modes.py.
    A child that failed stops the ones after it."""
    assert not _child_failed, f"not started: an earlier child failed ({_child_failed[0]})"
    full = dict(os.environ, **{"STG_DEBUG_TV16_FILL": "0", **env})
    r = subprocess.run([sys.executable, os.path.join(HERE, "ratio_fill_child.py")], capture_output=True, text=True,
                       timeout=110, env=full)
    if r.returncode != 0:
        _child_failed.append(env)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(out)
    assert out["ok"] and out["calls"] == len(rc.RATIOS) and out["largest_fill"] > 12288, out
    none, by_start, shadow, literal = out["paths"]
    leader, crew, leader_lit, crew_lit = out["wide"]
    mode = env.get("STG_DEBUG_TV16_FILL")
    if mode == "1":
        assert by_start == 0, out
    elif mode == "2":
        assert literal > 0 and by_start == 0 and shadow == 0 and out["wide"] == [0, 0, 0, 0], out
    elif mode == "3":
        assert by_start == 0 and shadow == 0 and leader > 0, out
    elif mode == "4":
        assert leader == 0 and crew > 0, out
    else:
        assert out["lfin"] == [0, 0, 0, 0] and crew + literal > 0, out


# ---------------------------------------------------------------------------
# threshold-v
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sched", list(rc.TV_SCHEDULES))
@pytest.mark.parametrize("n", rc.TV_SIZES)
def test_thresholdv_ratio(gpu, oracle, n, sched):
    """One device buffer (the state is keyed by its address), new data copied
    into it; k slots exactly, carved so that a store past them is seen.  The
    spike schedule finds hundreds of times k (far over the capacity)."""
    import torch
    from stellatrain_amd import ThresholdvCompressor
    comp = ThresholdvCompressor()
    ho = oracle.tv_new()
    d = torch.empty(n, dtype=torch.float32, device=gpu)
    worst = 0.0
    try:
        for it, r, k in rc.schedule(n, ratios=rc.TV_SCHEDULES[sched]):
            x = rc.ratio_input(n, it, bucket=rc.TV_SEED_BUCKET[sched])
            tb = oracle.tv_state(ho, 1)
            co, io, vo = oracle.tv_compress(ho, 1, x, k)
            if tb is not None:
                worst = max(worst, np.count_nonzero(np.abs(x) >= np.float32(tb)) / k)
            d.copy_(torch.from_numpy(x))
            idx = carve(torch, gpu, k, torch.int32, 0)
            val = carve(torch, gpu, k, torch.float32, 0)
            idx.zero_()
            val.zero_()
            what = f"threshold-v {sched}, n {n}, call {it}: ratio {r}, k {k}"
            assert comp.compress("ignored", d, k, idx, val) == co, what
            assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, co, what)
            assert fbits(comp.state("", key_ptr=d.data_ptr())[0]) == fbits(oracle.tv_state(ho, 1)), what
            assert_guards(idx, "idx: " + what)
            assert_guards(val, "val: " + what)
        comp.check_device()
    finally:
        oracle.tv_free(ho)
    print(sched, n, "largest cnt_found / k", round(worst, 1))
    if sched == "spike":
        assert worst > 50


# ---------------------------------------------------------------------------
# top-k: the hint meets a k ten times larger or smaller
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bug_compat", [False, True], ids=["exact", "shipped"])
def test_topk_k_schedule(gpu, oracle, bug_compat):
    import torch
    from stellatrain_amd import TopkCompressor
    comp = TopkCompressor(exact=not bug_compat)
    n = rc.TOPK_N
    d = torch.empty(n, dtype=torch.float32, device=gpu)
    w0 = debug_words(comp, gpu)
    for c, k in enumerate(rc.topk_ks(n)):
        x = rc.ratio_input(n, c, bucket=rc.TOPK_SEED_BUCKET)
        d.copy_(torch.from_numpy(x))
        what = f"top-k call {c}: k {k}"
        if k == 0:  # test_k_zero: the count is the capacity, nothing written
            idx = torch.zeros(4, dtype=torch.int32, device=gpu)
            val = torch.zeros(4, dtype=torch.float32, device=gpu)
            assert comp.compress("w", d, 0, idx, val, 0) == 4, what
            assert not idx.any() and not val.any(), what
        else:
            co, io, vo = oracle.topk_compress(x, k, bug_compat=bug_compat)
            idx = torch.zeros(k, dtype=torch.int32, device=gpu)
            val = torch.zeros(k, dtype=torch.float32, device=gpu)
            assert comp.compress("w", d, k, idx, val, 0) == co, what
            if bug_compat:
                np.testing.assert_array_equal(idx.cpu().numpy(), np.arange(k), what)
                assert_topk_values(val.cpu().numpy(), vo)
            else:
                assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, k, what)
        w = debug_words(comp, gpu)
        print(what, "band hits (38)", w[38] - w0[38], "select (39)", w[39] - w0[39])
        if c == 0:
            assert (w[38] - w0[38], w[39] - w0[39]) == (0, 1), w[36:40]  # the first call: the select's way
    comp.check_device()  # no failure bit


# ---------------------------------------------------------------------------
# sending side: CodecEngine.send_buckets across configure_compression_ratio
# ---------------------------------------------------------------------------
SEND_NS = (60000, 70003)  # u16 indices on the wire, u32 indices
SIDE_RATIOS = rc.RATIOS[:12]


def _send_grads(n, j, it, N=2, rank=0):
    return [synth(n, seed_for(940 + 10 * j + 100 * rank + s, it), D1) for s in range(N)]


@pytest.mark.parametrize("fp16_values", [False, True])
def test_send_buckets_ratio(gpu, oracle, fp16_values):
    """Two tensors, two sources each and a residual, the ratio reconfigured
    before every iteration: grad[0], residual, wire bytes up to the count,
    count and state against the oracle chain."""
    import torch
    from stellatrain_amd import CodecEngine, wire_flag
    eng = CodecEngine()
    ho = oracle.tv16_new()
    g = [[torch.zeros(n, dtype=torch.float32, device=gpu) for _ in range(2)] for n in SEND_NS]
    res = [torch.zeros(n, dtype=torch.float32, device=gpu) for n in SEND_NS]
    res_np = [np.zeros(n, np.float32) for n in SEND_NS]
    keys = [f"s{j}@weight" for j in range(len(SEND_NS))]
    try:
        for it, r in enumerate(SIDE_RATIOS):
            eng.configure_compression_ratio(r)
            srcs = [_send_grads(n, j, it) for j, n in enumerate(SEND_NS)]
            for j in range(len(SEND_NS)):
                for t, x in zip(g[j], srcs[j]):
                    t.copy_(torch.from_numpy(x))
            streams, counts = eng.send_buckets([(keys[j], g[j], res[j]) for j in range(len(SEND_NS))],
                                               fp16_values=fp16_values)
            torch.cuda.synchronize()
            cg = counts.cpu().numpy().tolist()
            for j, n in enumerate(SEND_NS):
                k, flag = rc.merge_k(n, r), wire_flag(n, fp16_values)
                what = f"send, iteration {it}: ratio {r}, n {n}, k {k}, flag {flag}"
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
# receiving side: per_rank shrinks and grows under persistent optimizer state
# ---------------------------------------------------------------------------
def _rank_streams_np(oracle, hos, name, n, j, it, per_rank, flag):
    """One wire stream per rank: the oracle's thresholdv16 stream of that
    rank's synthetic gradient (whole lines of 16 consecutive indices, ranks
    overlapping), packed by the oracle's wire_encode."""
    out = []
    for rank, ho in enumerate(hos):
        x = synth(n, seed_for(960 + 10 * j + rank, it), D1)
        co, io, vo = oracle.tv16_compress(ho, name, x, per_rank)
        assert co == per_rank
        out.append(oracle.wire_encode(io[:co], vo[:co], flag) + (flag,))
    return out


def _check_replicas(param, rep32, rep16, what):
    p = param.cpu().numpy()
    assert np.array_equal(u(rep32.cpu().numpy()), u(p)), "float32 replica: " + what
    import torch
    assert np.array_equal(rep16.view(torch.int16).cpu().numpy().view(np.uint16), P.f32_to_bf16_bits(p)), \
        "bfloat16 replica: " + what


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_merge_optimize_publish_ratio(gpu, oracle, kind, world):
    """merge_optimize_batch from MergeTasks rebuilt every iteration (per_rank
    follows the ratio), then PublishTasks.from_merge to a float32 and a
    bfloat16 replica; two names whose momentum / last-touched / m, v state
    persists while per_rank goes 600 -> 6,000 -> 60 -> 30,000 -> 600 (world 1)."""
    import torch
    from stellatrain_amd import MergeTasks, PublishTasks, publish_params, wire_flag
    from stellatrain_amd.engine import scatter_merge_check
    opt = Optim(oracle, kind)
    hos = [oracle.tv16_new() for _ in range(world)]
    names = [f"m{j}@weight" for j in range(len(SEND_NS))]
    p0 = [synth(n, seed_for(950 + j, 0), D1) * np.float32(100) for j, n in enumerate(SEND_NS)]
    po = [p.copy() for p in p0]
    pd = [torch.from_numpy(p).to(gpu) for p in p0]
    rep32 = [p.clone() for p in pd]
    rep16 = [p.to(torch.bfloat16) for p in pd]
    for j in range(len(SEND_NS)):
        _check_replicas(pd[j], rep32[j], rep16[j], "before the first step")
    try:
        for it, r in enumerate(SIDE_RATIOS):
            items, exp = [], []
            for j, n in enumerate(SEND_NS):
                per_rank, flag = rc.merge_k(n, r, world), wire_flag(n, bool(j))
                streams = _rank_streams_np(oracle, hos, names[j], n, j, it, per_rank, flag)
                ei, ev = W.expected(oracle, streams, per_rank, n)[2:4]
                exp.append((ei, ev))
                dev = [(torch.from_numpy(wi.view(np.int16 if wi.itemsize == 2 else np.int32)).to(gpu),
                        torch.from_numpy(wv.view(np.int16) if wv.itemsize == 2 else wv).to(gpu), f)
                       for wi, wv, f in streams]
                items.append((pd[j], names[j], dev, per_rank))
            tasks = MergeTasks(items)
            got = opt.dev.merge_optimize_batch(tasks)
            publish_params(PublishTasks.from_merge(tasks, [[rep32[j], rep16[j]] for j in range(len(SEND_NS))]))
            torch.cuda.synchronize()
            for j, n in enumerate(SEND_NS):
                what = f"{kind}, world {world}, iteration {it}: ratio {r}, n {n}, per_rank {rc.merge_k(n, r, world)}"
                ei, ev = exp[j]
                gi, gv = merged(got[j])
                assert gi.size == ei.size, "merged count: " + what
                assert np.array_equal(gi, ei) and np.array_equal(gv, u(ev)), "merged stream: " + what
                opt.apply_oracle(names[j], po[j], ev, ei)
            for j, n in enumerate(SEND_NS):  # (the optimizer's iteration count is shared by the names)
                what = f"{kind}, world {world}, iteration {it}: ratio {r}, n {n}, per_rank {rc.merge_k(n, r, world)}"
                opt.compare(names[j], pd[j], po[j], what)
                _check_replicas(pd[j], rep32[j], rep16[j], what)
        scatter_merge_check()
        opt.check()
    finally:
        for h in hos:
            oracle.tv16_free(h)
        opt.close()


# ---------------------------------------------------------------------------
# one closed loop: two ranks send, both merge what the two sent, and publish
# ---------------------------------------------------------------------------
def test_closed_loop_two_ranks(gpu, oracle):
    """Two simulated ranks, each with its own CodecEngine on its own stream.
    Their wire outputs are fed, in place, as the two rank streams of a world-2
    merge_optimize_batch + publish on each rank; the residual carries into the
    next iteration's send.  Parameters, residuals and thresholds of both ranks
    against the oracle chain, every iteration."""
    import torch
    from stellatrain_amd import CodecEngine, MergeTasks, PublishTasks, SparseSGD, publish_params, wire_flag
    from stellatrain_amd.engine import scatter_merge_check
    R, T = 2, len(SEND_NS)
    opts = dict(lr=0.05, momentum=0.9)
    eng = [CodecEngine() for _ in range(R)]
    sgd = [SparseSGD(**opts) for _ in range(R)]
    st = [torch.cuda.Stream(device=gpu) for _ in range(R)]
    ho = [oracle.tv16_new() for _ in range(R)]
    hs = oracle.sgd_new(**opts)
    keys = [f"c{j}@weight" for j in range(T)]
    p0 = [synth(n, seed_for(970 + j, 0), D1) * np.float32(100) for j, n in enumerate(SEND_NS)]
    po = [p.copy() for p in p0]
    pd = [[torch.from_numpy(p).to(gpu) for p in p0] for _ in range(R)]
    rep = [[p.to(torch.bfloat16) for p in pd[q]] for q in range(R)]
    g = [[[torch.zeros(n, dtype=torch.float32, device=gpu) for _ in range(2)] for n in SEND_NS] for _ in range(R)]
    res = [[torch.zeros(n, dtype=torch.float32, device=gpu) for n in SEND_NS] for _ in range(R)]
    res_np = [[np.zeros(n, np.float32) for n in SEND_NS] for _ in range(R)]
    torch.cuda.synchronize()
    try:
        for it, r in enumerate(SIDE_RATIOS):
            sent, srcs = [], []
            for q in range(R):
                eng[q].configure_compression_ratio(r)
                srcs.append([_send_grads(n, j, it, rank=q + 1) for j, n in enumerate(SEND_NS)])
                with torch.cuda.stream(st[q]):
                    for j in range(T):
                        for t, x in zip(g[q][j], srcs[q][j]):
                            t.copy_(torch.from_numpy(x))
                    sent.append(eng[q].send_buckets([(keys[j], g[q][j], res[q][j]) for j in range(T)], world=R))
            for q in range(R):
                st[q].synchronize()
            ks = [rc.merge_k(n, r, R) for n in SEND_NS]
            flags = [wire_flag(n) for n in SEND_NS]
            # in place: each rank's first per_rank slots of the buffers send_buckets handed out
            rank_streams = [[(sent[q][0][j][0][:ks[j]], sent[q][0][j][1][:ks[j]], flags[j]) for q in range(R)]
                            for j in range(T)]
            outs = []
            for q in range(R):
                with torch.cuda.stream(st[q]):
                    tasks = MergeTasks([(pd[q][j], keys[j], rank_streams[j], ks[j]) for j in range(T)])
                    outs.append(sgd[q].merge_optimize_batch(tasks))
                    publish_params(PublishTasks.from_merge(tasks, [[rep[q][j]] for j in range(T)]))
            torch.cuda.synchronize()
            # the oracle chain
            for j, n in enumerate(SEND_NS):
                what = f"closed loop, iteration {it}: ratio {r}, n {n}, per_rank {ks[j]}"
                wire = []
                for q in range(R):
                    x, co, wi, wv = oracle_send(oracle, ho[q], keys[j], srcs[q][j], res_np[q][j], ks[j], flags[j])
                    res_np[q][j] = x.copy()
                    assert int(sent[q][1].cpu().numpy()[j]) == co == ks[j], what
                    assert np.array_equal(u(res[q][j].cpu().numpy()), u(x)), f"residual of rank {q}: " + what
                    assert np.array_equal(u(sent[q][0][j][0].cpu().numpy())[:co], u(wi)), f"wire of rank {q}: " + what
                    assert np.array_equal(u(sent[q][0][j][1].cpu().numpy())[:co], u(wv)), f"wire of rank {q}: " + what
                    assert state_bits(eng[q].compressor().state(keys[j])) == \
                        state_bits(oracle.tv16_state(ho[q], keys[j])), f"threshold of rank {q}: " + what
                    wire.append((wi, wv, flags[j]))
                ei, ev = W.expected(oracle, wire, ks[j], n)[2:4]
                oracle.sgd_apply(hs, keys[j], po[j], ev, ei)
                for q in range(R):
                    gi, gv = merged(outs[q][j])
                    assert np.array_equal(gi, ei) and np.array_equal(gv, u(ev)), f"merged stream on rank {q}: " + what
                    assert np.array_equal(u(pd[q][j].cpu().numpy()), u(po[j])), f"parameter on rank {q}: " + what
                    assert np.array_equal(rep[q][j].view(torch.int16).cpu().numpy().view(np.uint16),
                                          P.f32_to_bf16_bits(po[j])), f"replica on rank {q}: " + what
        for q in range(R):
            with torch.cuda.stream(st[q]):
                scatter_merge_check()
            eng[q].compressor().check_device()
            sgd[q].check()
    finally:
        for h in ho:
            oracle.tv16_free(h)
        oracle.sgd_free(hs)
