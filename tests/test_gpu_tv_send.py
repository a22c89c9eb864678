"""GPU parity of the one-call send path on a threshold-v handle
(``stg_merge_send_batch_device`` / ``..._typed_device`` with ``"thresholdv"``,
``Compressor.merge_send_batch_async``, ``CodecEngine.send_buckets``): the
batched scan of csrc/tv_batch.hip and the finish that reads the device count.

Every comparison is whole-buffer and bit for bit, against both
(a) the oracle -- ``gather_add``, ``tv_compress`` into zeroed slots, the wire
    form of all ``W = min(idx_cap, n)`` slots, numpy error feedback over them
    (tests/tv_send_cases.py ``Ref``) -- and
(b) a twin ``ThresholdvCompressor`` running the per-tensor sequence on copies
    (``merge_gather_compress_async`` into zeroed u32 / f32 temporaries of
    ``idx_cap`` slots, then ``wire_encode`` of the first ``W``):
grad[0], the residual, the first ``W`` wire elements, the sentinel past ``W``,
the count, the threshold bits of ``state(key_ptr=...)``; ``check_device()``
clean on both sides.  The key is the pointer of grad[0], so either side keeps
its buffers for the whole test and fresh gradients are copied in per call.
tests/test_tv_send_host.py shows, by the reference alone, which situations the
sequences reach."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import tv_send_cases as T

pytestmark = pytest.mark.gpu


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.itemsize == 2 else a.view(np.uint32)


def _fbits(x):
    return int(np.asarray(x, np.float32).view(np.uint32))


class Side:
    """One codec side's device buffers of a case: persistent gradient and
    residual tensors and sentinel-filled wire outputs."""

    def __init__(self, torch, gpu, c):
        def buf(n, dt=torch.float32):  # shift: a view offset by one float, another 16-byte phase than grad[0]
            return torch.zeros(n + 1, dtype=dt, device=gpu)[1:] if c.shift else torch.zeros(n, dtype=dt, device=gpu)
        self.g = [torch.zeros(c.n, dtype=torch.float32, device=gpu)]
        for r in range(1, c.N):
            self.g.append(buf(c.n, torch.bfloat16 if c.bf16 and r == 1 else torch.float32))
        self.r = None
        if c.resid:
            self.r = buf(c.n)
            self.r.copy_(torch.from_numpy(c.resid0()))
        self.di = torch.empty(c.cap, dtype=torch.int16 if c.flag & 1 else torch.int32, device=gpu)
        self.dv = torch.empty(c.cap, dtype=torch.int16 if c.flag & 2 else torch.float32, device=gpu)

    def load(self, torch, srcs):
        for t, x in zip(self.g, srcs):
            t.copy_(torch.from_numpy(x).to(t.dtype))  # (a bf16 source holds bf16 values: exact)
        self.di.fill_(-1)
        self.dv.fill_(-1)

    def key(self):
        return self.g[0].data_ptr()

    def tensors(self):
        return self.g + ([self.r] if self.r is not None else []) + [self.di, self.dv]


def _twin_step(torch, twin, c, sd):
    """Comparison (b): the per-tensor sequence on the twin's buffers."""
    from stellatrain_amd import wire_encode
    ti = torch.zeros(c.cap, dtype=torch.int32, device=sd.di.device)
    tv = torch.zeros(c.cap, dtype=torch.float32, device=sd.di.device)
    cnt = twin.merge_gather_compress_async("", sd.g, c.k, ti, tv, residual=sd.r)
    if c.W:
        wire_encode(ti[:c.W], tv[:c.W], c.flag, idx_out=sd.di, val_out=sd.dv)
    return cnt


def _same(a, b, what):
    assert np.array_equal(_u(a.cpu().numpy()), _u(b.cpu().numpy())), what


def _sentinel(t, count):
    return bool((t[count:] == -1).all().item())


class Runner:
    """Both GPU sides and the oracle side of a list of cases, call after call."""

    def __init__(self, gpu, oracle, cases, mode="items", n_oracle=None):
        import torch
        from stellatrain_amd import CodecEngine, ThresholdvCompressor
        self.torch, self.gpu, self.o, self.cases, self.mode = torch, gpu, oracle, cases, mode
        self.eng = None
        if mode == "engine":
            self.eng = CodecEngine()
            self.eng.configure_compression("thresholdv")
        self.comp = self.eng.compressor() if self.eng else ThresholdvCompressor()
        assert self.comp.name() == "Thresholdv"
        self.twin = ThresholdvCompressor()
        self.ho = oracle.tv_new()
        self.new = [Side(torch, gpu, c) for c in cases]
        self.old = [Side(torch, gpu, c) for c in cases]
        n_oracle = len(cases) if n_oracle is None else n_oracle
        self.ref = [T.Ref(oracle, self.ho, j + 1, c) if j < n_oracle and c.n else None for j, c in enumerate(cases)]
        self.counts = torch.full((len(cases),), -1, dtype=torch.int32, device=gpu)
        self.pre = {}

    def close(self):
        self.o.tv_free(self.ho)

    def item(self, j):
        c, s = self.cases[j], self.new[j]
        return ("", s.g, c.k, s.di, s.dv, s.r, c.flag)

    def call(self, it, live=None, hook=None):
        """One batched call over the tasks `live` (default: all), its twin
        calls, and every comparison."""
        torch, cases = self.torch, self.cases
        from stellatrain_amd import SendTasks
        live = list(range(len(cases))) if live is None else live
        srcs = {j: cases[j].grads(it) for j in live}
        for j in live:
            self.new[j].load(torch, srcs[j])
            self.old[j].load(torch, srcs[j])
        self.counts.fill_(-1)
        if self.eng:
            streams, cnt = self.eng.send_buckets([("", self.new[j].g, self.new[j].r) if cases[j].resid else
                                                  ("", self.new[j].g) for j in live])
            for j, (wi, wv, fl) in zip(live, streams):
                assert fl == cases[j].flag and wi.numel() == cases[j].cap == cases[j].k
                self.new[j].di, self.new[j].dv = wi, wv
            got = cnt.cpu().numpy().tolist()
        elif self.mode == "prebuilt":
            key = tuple(live)
            if key not in self.pre:  # (counts: one word per item of the array)
                self.pre[key] = SendTasks([self.item(j) for j in live], counts=self.counts[:len(live)])
            assert self.comp.merge_send_batch_async(self.pre[key]) is self.pre[key].counts
            got = self.counts[:len(live)].cpu().numpy().tolist()
        else:
            self.comp.merge_send_batch_async([self.item(j) for j in live], counts=self.counts[:len(live)])
            got = self.counts[:len(live)].cpu().numpy().tolist()
        tcnt = {j: _twin_step(torch, self.twin, cases[j], self.old[j]) for j in live if cases[j].n}
        torch.cuda.synchronize()
        for pos, j in enumerate(live):
            c, a, b = cases[j], self.new[j], self.old[j]
            what = f"call {it}, task {j} ({c})"
            if not c.n:
                assert got[pos] == 0, what
                assert _sentinel(a.di, 0) and _sentinel(a.dv, 0), what
                continue
            assert got[pos] == int(tcnt[j].item()), "count vs twin: " + what
            assert 0 <= got[pos] <= c.W, what
            _same(a.g[0], b.g[0], "grad[0] vs twin: " + what)
            if c.resid:
                _same(a.r, b.r, "residual vs twin: " + what)
            _same(a.di[:c.W], b.di[:c.W], "wire indices vs twin: " + what)
            _same(a.dv[:c.W], b.dv[:c.W], "wire values vs twin: " + what)
            ta, tb = self.comp.state(key_ptr=a.key()), self.twin.state(key_ptr=b.key())
            assert ta is not None and _fbits(ta[0]) == _fbits(tb[0]), "threshold vs twin: " + what
            if not self.eng:  # (the engine hands out zeroed buffers of exactly numel slots)
                assert _sentinel(a.di, c.W) and _sentinel(a.dv, c.W), "written past W: " + what
            if self.ref[j] is None:
                continue
            st = self.ref[j].step(srcs[j])
            assert got[pos] == st.count, "count vs oracle: " + what
            g0 = a.g[0].cpu().numpy()
            assert np.array_equal(_u(g0), _u(st.grad)), "grad[0] vs oracle: " + what
            if c.resid:
                assert np.array_equal(_u(a.r.cpu().numpy()), _u(st.grad)), "residual vs oracle: " + what
            assert np.array_equal(_u(a.di.cpu().numpy())[:c.W], _u(st.wi)), "wire indices vs oracle: " + what
            assert np.array_equal(_u(a.dv.cpu().numpy())[:c.W], _u(st.wv)), "wire values vs oracle: " + what
            assert _fbits(ta[0]) == _fbits(st.t_next), "threshold vs oracle: " + what
            if hook:
                hook(it, j, c, st, g0)

    def check(self):
        self.comp.check_device()
        self.twin.check_device()


def _run(gpu, oracle, cases, calls, mode="items", hook=None):
    r = Runner(gpu, oracle, cases, mode)
    try:
        for it in range(calls):
            r.call(it, hook=hook)
        r.check()
    finally:
        r.close()


# ---- single tasks ----

@pytest.mark.parametrize("n", T.SINGLE_N)
def test_tv_send_single_task(gpu, oracle, n):
    """One task per call: the first call (its threshold from the gathered
    bucket) and two more; flags 0-3, N in {1, 2, 9}, with and without a
    residual, residual and sources at another 16-byte phase."""
    for c in T.single_cases(n):
        _run(gpu, oracle, [c], calls=3)


def test_tv_send_ragged_tail_element_selected(gpu, oracle):
    """An element of the n % 4 tail, folded by one lane of the last range, is
    on the wire and zeroed by its index."""
    hit = []

    def hook(it, j, c, st, g0):
        t = st.idx[:st.count][st.idx[:st.count] >= c.n // 4 * 4]
        hit.append(t.size)
        assert (g0[t] == 0).all()

    _run(gpu, oracle, [T.tail_case(T.TAIL_SEED)], calls=T.TAIL_CALLS, hook=hook)
    assert max(hit) > 0, hit


def test_tv_send_capacity_past_n(gpu, oracle):
    """idx_cap = 48 > n = 40: W = 40 slots are written, the other 8 keep the
    sentinel; a short count zeroes element 0."""
    short = []

    def hook(it, j, c, st, g0):
        short.append(st.count < c.W)
        if st.count < c.W:
            assert g0[0] == 0

    _run(gpu, oracle, [T.CAP_PAST_N], calls=3, hook=hook)
    assert any(short)


# ---- call sequences ----

@pytest.mark.parametrize("name", sorted(T.SEQ_CASES))
def test_tv_send_sequence(gpu, oracle, name):
    """SCALES twice through with the residual carried: calls that find more
    than the capacity, calls that find fewer (the unused slots on the wire,
    element 0 zeroed) and a range whose LDS list overflows and is re-scanned
    in order; for n = 60,000 under flag 1, u16 indices past 32,767 zeroed by
    their true index."""
    seen = {"over": 0, "short": 0, "lds": 0, "high": 0}

    def hook(it, j, c, st, g0):
        seen["over"] += st.found > c.cap
        seen["short"] += st.found < c.cap
        seen["lds"] += max(st.per_range) > T.LCAP
        ix = st.idx[:st.count]
        seen["high"] += int((ix > 32767).sum())
        assert (g0[ix] == 0).all()
        if st.count < c.W:
            assert g0[0] == 0

    c = T.SEQ_CASES[name]
    _run(gpu, oracle, [c], calls=T.SEQ_CALLS, hook=hook)
    assert seen["over"] and seen["short"] and seen["lds"], seen
    assert seen["high"] or c.n <= 32768


def test_tv_send_nan_from_the_third_call(gpu, oracle):
    """NaNs in the bucket from call 2 on (and in the residual after it): a
    NaN never qualifies, and with k < cnt the next threshold takes gmax by the
    reference's NaN-restart rule, from the re-read of the last range."""
    hits = []

    def hook(it, j, c, st, g0):
        hits.append(bool(np.isnan(g0).any()) and st.found > c.k)

    _run(gpu, oracle, [T.NAN_CASE], calls=T.NAN_CALLS, hook=hook)
    assert sum(hits) >= 2 and not any(hits[:2])


# ---- 40 tasks ----

@pytest.mark.parametrize("mode", ["items", "prebuilt", "engine"])
def test_tv_send_batched_40_tasks(gpu, oracle, mode):
    """Sizes 1 to 300,007 (one to 19 ranges), an empty task in the middle, one
    bf16 source (the typed entry point), keys that first appear at call 2 --
    first-call and steady keys in one scan launch -- and, between the batched
    calls, a per-tensor compress of another key on the same handle and stream:
    the batched and per-tensor launches share the workspace's ticket and tag
    sequence."""
    import torch
    cases = T.batch_cases(mode == "engine")
    r = Runner(gpu, oracle, cases, mode, n_oracle=12)
    other = T.Case(70001, 700, 0, 1, seed=90)
    src = torch.zeros(other.n, dtype=torch.float32, device=gpu)
    oi = torch.zeros(other.k, dtype=torch.int32, device=gpu)
    ov = torch.zeros(other.k, dtype=torch.float32, device=gpu)
    ho = oracle.tv_new()
    try:
        for it in range(T.BATCH_CALLS):
            r.call(it, live=T.batch_live(it))
            x = other.grads(it)[0]
            src.copy_(torch.from_numpy(x))
            co, io, vo = oracle.tv_compress(ho, 1, x, other.k)
            cnt = r.comp.compress_async("", src, other.k, oi, ov)
            assert int(cnt.item()) == co, it
            assert np.array_equal(oi.cpu().numpy().view(np.uint32)[:co], io[:co]), it
            assert np.array_equal(_u(ov.cpu().numpy())[:co], _u(vo[:co])), it
            assert _fbits(r.comp.state(key_ptr=src.data_ptr())[0]) == _fbits(oracle.tv_state(ho, 1)), it
        r.check()
    finally:
        oracle.tv_free(ho)
        r.close()


def test_tv_send_one_large_task_runs_alone(gpu, oracle):
    """2^22 + 5 floats are 257 ranges, more than one launch takes on this
    device: the task runs through the per-tensor scan between two shared
    launches, and the finish still reads its device count."""
    import torch
    from stellatrain_amd._capi import lib
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    sizes = (C.c_uint64 * 3)(1000, T.LARGE_N, 4099)
    first, launch = (C.c_uint32 * 3)(), (C.c_uint32 * 3)()
    assert lib().stg_debug_tv_batch_plan(sizes, 3, cus, first, launch) == 3 and list(launch) == [0, 1, 2], cus
    cases = [T.Case(1000, 10, 1, 2, seed=91), T.Case(T.LARGE_N, 41943, 3, 2, seed=92), T.Case(4099, 41, 0, 1, seed=93)]
    _run(gpu, oracle, cases, calls=2)


# ---- refusals: all or nothing ----

def test_tv_send_refusals_change_nothing(gpu):
    import torch
    from stellatrain_amd import SendTasks, ThresholdvCompressor, TopkCompressor
    from stellatrain_amd._capi import StgSendTask, lib
    L = lib()
    f = L.stg_merge_send_batch_device
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cases = [T.Case(4099, 41, (1, 3, 0)[j], 2, seed=60 + j) for j in range(3)]
    sides = [Side(torch, gpu, c) for c in cases]
    for c, s in zip(cases, sides):
        s.load(torch, c.grads(0))
    comp = ThresholdvCompressor()
    comp.merge_send_batch_async([("", sides[0].g, cases[0].k, sides[0].di, sides[0].dv, sides[0].r, cases[0].flag)])
    for c, s in zip(cases, sides):  # key 0 has state; keys 1 and 2 never compressed
        s.load(torch, c.grads(1))
    good = SendTasks([("", s.g, c.k, s.di, s.dv, s.r, c.flag) for c, s in zip(cases, sides)])
    torch.cuda.synchronize()
    st0, snap = comp.state(key_ptr=sides[0].key()), [[t.clone() for t in s.tensors()] for s in sides]
    assert st0 is not None

    def unchanged(what):
        torch.cuda.synchronize()
        assert _fbits(comp.state(key_ptr=sides[0].key())[0]) == _fbits(st0[0]), what
        assert comp.state(key_ptr=sides[1].key()) is None and comp.state(key_ptr=sides[2].key()) is None, what
        for s, before in zip(sides, snap):
            for t, b in zip(s.tensors(), before):
                _same(t, b, what)

    null_src = (C.c_void_p * 2)(sides[1].g[0].data_ptr(), None)
    bad = {
        "repeated pointer key": (2, lambda t: setattr(t.bucket, "d_src", sides[0].key()), b"key"),
        "flag 4": (1, lambda t: setattr(t, "wire_flag", 4), b"flag"),
        "null source": (1, lambda t: setattr(t, "d_grads", null_src), b"null source"),
    }
    for what, (pos, spoil, word) in bad.items():
        arr = (StgSendTask * 3)()
        C.memmove(arr, good.array, C.sizeof(arr))
        spoil(arr[pos])
        assert f(comp._h, arr, 3, sp) == -1, what
        msg = L.stg_last_error()
        assert msg.startswith(b"task %d:" % pos) and word in msg, (what, msg)
        unchanged(what)

    topk = TopkCompressor()
    assert f(topk._h, good.array, 3, sp) == -4, L.stg_last_error()
    unchanged("topk handle")

    # the untouched array still runs
    comp.merge_send_batch_async(good)
    torch.cuda.synchronize()
    assert all(0 <= c <= 41 for c in good.counts.cpu().numpy().tolist())
    assert comp.state(key_ptr=sides[1].key()) is not None
    comp.check_device()
