"""GPU parity of the gather-add from bf16 / fp16 gradient sources
(``stg_gather_add_typed_device``, ``stg_merge_gather_compress_typed_device``,
``stg_merge_send_batch_typed_device`` through ``gather_add``,
``merge_gather_compress_async`` and ``merge_send_batch_async``).

Widening bf16 / fp16 to fp32 is exact, so every result is defined bit for bit
by what the project already pins: the oracle's gather-add run on CPU-widened
copies, and, for the send path, a twin codec handle fed fp32 copies through the
existing fp32 entry points.  Every comparison is of the 32-bit words."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from stellatrain_amd.synth import D1, D2, seed_for, synth

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2
GUARD = 0x5ca1ab1e  # the word around every bucket


def _tdt(torch, dt):
    return (torch.float32, torch.bfloat16, torch.float16)[dt]


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.itemsize == 2 else a.view(np.uint32)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _words(torch, t):
    """The raw words of a tensor, on the host."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy().copy()


def _at(torch, gpu, host, off, pad=8):
    """`host` (a CPU tensor) on the device at element offset `off` of a fresh
    allocation: the 16-byte phase of the view is off * element size."""
    base = torch.zeros(host.numel() + off + pad, dtype=host.dtype, device=gpu)
    v = base[off:off + host.numel()]
    v.copy_(host)
    return v


def _plan(tensors, start, n):
    """The launcher's plan for these streams over n elements from `start`."""
    from stellatrain_amd._capi import lib
    from stellatrain_amd.compressor import grad_dtype
    a = (C.c_uint64 * len(tensors))(*[t.data_ptr() + t.element_size() * start for t in tensors])
    d = (C.c_int * len(tensors))(*[grad_dtype(t) for t in tensors])
    w, h = C.c_uint32(), C.c_uint32()
    assert lib().stg_debug_gather_plan(a, d, len(tensors), n, C.byref(w), C.byref(h)) == 0
    return w.value, h.value


# ---- 1. exhaustive widening ----

@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
def test_every_16bit_word_widens_exactly(gpu, dt):
    """All 65,536 words as one source into a bucket of -0.0 (-0.0 + x is x, sign
    included, for every non-NaN x): the bucket equals torch's CPU widening bit
    for bit and is NaN exactly where the word is; the same with the words as
    the typed first term (no addition at all), and through the scalar path."""
    import torch
    from stellatrain_amd import gather_add
    n = 1 << 16
    words = torch.from_numpy(np.arange(n, dtype=np.uint16).view(np.int16)).view(_tdt(torch, dt))
    want = words.float().numpy()
    nan = np.isnan(want)
    assert 0 < nan.sum() < 2200 and np.signbit(want[0x8000]) and want[0x8000] == 0 and want[1] > 0

    def check(bucket, what):
        got = bucket.cpu().numpy()
        assert np.array_equal(np.isnan(got), nan), what
        assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), what

    neg0 = torch.full((n,), -0.0, dtype=torch.float32)
    for off, width in ((0, 8), (1, 0)):  # (an odd 16-bit element against the bucket's phase 0: no common head)
        src = _at(torch, gpu, words, off)
        bucket = _at(torch, gpu, neg0, 0)
        assert _plan([bucket, src], 0, n // 2)[0] == width
        for r in range(2):
            gather_add([bucket, src], None, r)
        check(bucket, f"source, offset {off}")
        assert _words(torch, src).tolist() == _words(torch, words).tolist()
        bucket = _at(torch, gpu, torch.full((n,), 7.0), 0)
        gather_add([src], None, 0, out=bucket)
        check(bucket, f"typed first term, offset {off}")


# ---- 2. parity with the oracle ----

def _planted(torch, dt):
    """+-0, +-inf, the largest finite value and the smallest subnormal of a type."""
    if dt == F32:
        w = np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 1, 0x80000001], np.uint32)
        return torch.from_numpy(w.view(np.float32).copy())
    big = 0x7f7f if dt == BF16 else 0x7bff
    inf = 0x7f80 if dt == BF16 else 0x7c00
    w = np.array([0, 0x8000, inf, 0x8000 | inf, big, 0x8000 | big, 1, 0x8001], np.uint16)
    return torch.from_numpy(w.view(np.int16).copy()).view(_tdt(torch, dt))


MIXES = {"bf16": lambda s: BF16, "fp16": lambda s: F16, "mixed": lambda s: (F32, BF16, F16)[s % 3]}
SIZES = list(range(1, 34)) + [4099, 65541, 100003]


def _host_sources(torch, n, N, mix, seed):
    """Source s of a case: synth D1 / D2 rounded to its type, the planted words
    in source 1 (or 0 when alone) from element 3 on; and the fp32 widening."""
    out = []
    for s in range(N):
        dt = MIXES[mix](s)
        t = torch.from_numpy(synth(n, seed_for(seed + s, 1), D1 if s % 2 else D2)).to(_tdt(torch, dt))
        if s == min(1, N - 1):
            p = _planted(torch, dt)[:max(0, n - 3)]
            t[3:3 + p.numel()] = p
        out.append(t)
    return out, [t.float().numpy().copy() for t in out]


@pytest.mark.parametrize("N", [2, 3, 5, 9, 16])
def test_gather16_matches_oracle(gpu, oracle, N):
    """Every local rank's slice against oracle.gather_add on widened copies,
    the whole guarded allocation compared after every rank's call: all-bf16,
    all-fp16 and mixed sources, with and without the residual (the oracle adds
    -0.0 for none: the identity), in place and with a typed first term."""
    import torch
    from stellatrain_amd import gather_add
    widths = set()
    for n in SIZES:
        resid_np = (synth(n, seed_for(31, n & 7)) * np.float32(0.25)).astype(np.float32)
        d_res = _at(torch, gpu, torch.from_numpy(resid_np), 0)
        for mix in MIXES:
            host, wide = _host_sources(torch, n, N, mix, 90)
            dev = [_at(torch, gpu, t, 0) for t in host]
            for use_res in (True, False):
                for term0 in (False, True):
                    # the bucket between guard words; in place it starts as fp32 data of its own
                    own = synth(n, seed_for(60, 2), D1)
                    buf = torch.full((n + 16,), 0, dtype=torch.int32, device=gpu)
                    buf.fill_(GUARD)
                    bucket = buf[8:8 + n].view(torch.float32)
                    bucket.copy_(torch.from_numpy(own))
                    exp = np.full(n + 16, GUARD, np.uint32)
                    ref = [(wide[0] if term0 else own).copy()] + wide[1:]
                    r_ref = resid_np if use_res else np.full(n, -0.0, np.float32)
                    grads = dev if term0 else [bucket] + dev[1:]
                    what = f"n={n} N={N} {mix} resid={use_res} term0={term0}"
                    if not term0:
                        exp[8:8 + n] = own.view(np.uint32)
                    done = np.zeros(n, bool)
                    for r in range(N):
                        a, b = n * r // N, n * (r + 1) // N
                        if b > a:
                            streams = [bucket] + ([d_res] if use_res else []) + (dev if term0 else dev[1:])
                            widths.add(_plan(streams, a, b - a)[0])
                        gather_add(grads, d_res if use_res else None, r, out=bucket if term0 else None)
                        oracle.gather_add(ref, r_ref, r)
                        done[a:b] = True
                        got = buf.cpu().numpy().view(np.uint32)
                        if term0:  # (write-only bucket: a slice not yet summed still holds its own data)
                            exp[8:8 + n] = np.where(done, ref[0].view(np.uint32), own.view(np.uint32))
                        else:
                            exp[8:8 + n] = ref[0].view(np.uint32)
                        assert not np.isnan(ref[0]).any(), what
                        assert np.array_equal(got, exp), f"{what} rank {r}"
            for t, h in zip(dev, host):
                assert np.array_equal(_words(torch, t), _words(torch, h)), f"a source changed: n={n} {mix}"
            assert np.array_equal(_u(d_res.cpu().numpy()), _u(resid_np)), "the residual changed"
    assert 8 in widths


# (n, bucket offset, residual offset, the two 16-bit sources' offsets, rank 0's plan): offsets in elements
PHASES = [
    (4099, 0, 0, (0, 0), (8, 0)),
    (4099, 1, 1, (5, 5), (8, 3)),   # 3 floats and 5 + 3 halves reach 16 bytes
    (37, 3, 3, (7, 7), (8, 1)),
    (4099, 0, 0, (0, 4), (4, 0)),   # the 16-bit streams 8 bytes apart in phase: no 8-wide group
    (4099, 2, 2, (2, 6), (4, 2)),
    (4099, 0, 0, (1, 0), (0, 0)),   # an odd 16-bit element against fp32 phase 0: scalar
    (4099, 0, 1, (0, 0), (0, 0)),   # bucket and residual at different phases: scalar
    (4099, 3, 3, (3, 2), (0, 0)),
]


def _model_plan(tensors, start, n):
    """The rule of include/stg/codec.h, written out again."""
    for w in (8, 4):
        for h in range(w):
            if all((t.data_ptr() + t.element_size() * (start + h)) % (16 if t.element_size() == 4 else 2 * w) == 0
                   for t in tensors):
                return w, min(h, n)
    return 0, 0


@pytest.mark.parametrize("case", PHASES, ids=lambda c: f"n{c[0]}-b{c[1]}-r{c[2]}-s{c[3][0]}_{c[3][1]}")
def test_gather16_phases(gpu, oracle, case):
    """fp32 buffers at element offsets 0..3 and 16-bit buffers at 0..7 against
    16 bytes, cases for each plan (8-wide, 4-wide, scalar; heads and tails
    included): which plan runs is asserted through the diagnostic with the
    case's pointers, for every rank's slice."""
    import torch
    from stellatrain_amd import gather_add
    n, ob, orr, o16, plan0 = case
    host, wide = _host_sources(torch, n, 3, "mixed", 40)  # (f32), bf16, f16
    own = synth(n, seed_for(61, 2), D2)
    resid_np = synth(n, seed_for(32, 1), D1)
    bucket = _at(torch, gpu, torch.from_numpy(own), ob)
    d_res = _at(torch, gpu, torch.from_numpy(resid_np), orr)
    grads = [bucket, _at(torch, gpu, host[1], o16[0]), _at(torch, gpu, host[2], o16[1])]
    streams = [bucket, d_res] + grads[1:]
    assert _plan(streams, 0, n // 3) == plan0
    ref = [own.copy()] + wide[1:]
    for r in range(3):
        a, b = n * r // 3, n * (r + 1) // 3
        assert _plan(streams, a, b - a) == _model_plan(streams, a, b - a), r
        gather_add(grads, d_res, r)
        oracle.gather_add(ref, resid_np, r)
    assert np.array_equal(_u(bucket.cpu().numpy()), _u(ref[0])), case


# ---- 3. the send path against a twin handle fed fp32 copies ----

class Task:
    def __init__(self, key, n, N, flag, dts, resid=True, term0=False, k=None):
        self.key, self.n, self.N, self.flag, self.dts, self.resid, self.term0 = key, n, N, flag, dts, resid, term0
        self.k = (max(n // 100, 1) if n else 0) if k is None else k
        self.cap = self.k if n else 4
        self.count = min(self.cap, n)

    def sources(self, torch, it, seed):
        s = np.float32((1.0, 0.01, 30.0)[it % 3])
        return [torch.from_numpy((synth(self.n, seed_for(500 + seed + r, it), D2 if r % 2 else D1) * s)
                                 .astype(np.float32)).to(_tdt(torch, dt)) for r, dt in enumerate(self.dts)]


class Bufs:
    """One side's device buffers of a task.  typed: the sources in their own
    types (and a separate bucket under a typed first term); else fp32 copies."""

    def __init__(self, torch, gpu, t, typed):
        self.typed = typed
        dts = t.dts if typed else [F32] * t.N
        self.g = [torch.zeros(t.n, dtype=_tdt(torch, dt), device=gpu) for dt in dts]
        self.bucket = torch.zeros(t.n, dtype=torch.float32, device=gpu) if typed and t.term0 else self.g[0]
        self.r = torch.zeros(t.n, dtype=torch.float32, device=gpu) if t.resid else None
        self.di = torch.empty(t.cap, dtype=torch.int16 if t.flag & 1 else torch.int32, device=gpu)
        self.dv = torch.empty(t.cap, dtype=torch.int16 if t.flag & 2 else torch.float32, device=gpu)

    def load(self, srcs):
        for d, s in zip(self.g, srcs):
            d.copy_(s.float() if d.dtype != s.dtype else s)
        if self.bucket is not self.g[0]:
            self.bucket.fill_(123.0)
        self.di.fill_(-1)
        self.dv.fill_(-1)

    def item(self, t):
        base = (t.key, self.g, t.k, self.di, self.dv, self.r, t.flag)
        return base + (0, self.bucket) if self.bucket is not self.g[0] else base


def _send_tasks():
    ns = [1, 17, 33, 1000, 4099, 60000, 70000, 65541, 0, 4097, 259, 8191, 16, 12345, 40001, 999, 2048, 31, 5000, 69999]
    out = []
    for j, n in enumerate(ns):
        N = (1, 2, 4)[j % 3]
        flag = j % 4 if n < 65536 else (j % 4) & 2
        dts = [(F32, BF16, F16)[(j + s) % 3] for s in range(N)]
        term0 = j in (3, 10)
        dts[0] = (BF16 if j == 3 else F16) if term0 else F32
        if j == 7:
            dts = [F32] * N  # all fp32 in place: srcs[i] stays null
        out.append(Task(f"t{j}@g16", n, N, flag, dts, resid=j % 5 != 4, term0=term0))
    assert sum(t.term0 for t in out) == 2 and any(t.n == 0 for t in out) and len(out) == 20
    assert any(BF16 in t.dts[1:] for t in out) and any(F16 in t.dts[1:] for t in out)
    return out


def _run_send(gpu, tasks, calls, single=False):
    """`calls` consecutive calls: the typed call on one handle, the fp32 call on
    fp32 copies on its twin; everything the call leaves must be equal."""
    import torch
    from stellatrain_amd import SendTasks, ThresholdvCompressor16
    comp, twin = ThresholdvCompressor16(), ThresholdvCompressor16()
    new = [Bufs(torch, gpu, t, True) for t in tasks]
    old = [Bufs(torch, gpu, t, False) for t in tasks]
    for t, a, b in zip(tasks, new, old):
        if t.resid:
            r0 = torch.from_numpy((synth(t.n, seed_for(499, 0)) * np.float32(0.25)).astype(np.float32))
            a.r.copy_(r0)
            b.r.copy_(r0)
    pre = None
    if not single:
        pre = SendTasks([a.item(t) for t, a in zip(tasks, new)])
        assert pre.srcs is not None and not pre.srcs[7] and pre.srcs[3] and pre.srcs[10]
    for it in range(calls):
        for j, (t, a, b) in enumerate(zip(tasks, new, old)):
            srcs = t.sources(torch, it, 10 * j)
            a.load(srcs)
            b.load(srcs)
        if single:
            t, a, b = tasks[0], new[0], old[0]
            c1 = comp.merge_gather_compress_async(t.key, a.g, t.k, a.di, a.dv, residual=a.r,
                                                  bucket=a.bucket if t.term0 else None)
            c2 = twin.merge_gather_compress_async(t.key, b.g, t.k, b.di, b.dv, residual=b.r)
            cn, co = c1.cpu().numpy().tolist(), c2.cpu().numpy().tolist()
        else:
            cn = comp.merge_send_batch_async(pre).cpu().numpy().tolist()
            co = twin.merge_send_batch_async([b.item(t) for t, b in zip(tasks, old)]).cpu().numpy().tolist()
        torch.cuda.synchronize()
        assert cn == co == [t.count for t in tasks], it
        for j, (t, a, b) in enumerate(zip(tasks, new, old)):
            what = f"call {it}, task {j}: n={t.n} N={t.N} flag={t.flag} dts={t.dts} resid={t.resid} term0={t.term0}"
            if not t.n:
                assert bool((a.di == -1).all().item()) and bool((a.dv == -1).all().item()), what
                continue
            assert np.array_equal(_u(a.bucket.cpu().numpy()), _u(b.bucket.cpu().numpy())), "bucket: " + what
            if t.resid:
                assert np.array_equal(_u(a.r.cpu().numpy()), _u(b.r.cpu().numpy())), "residual: " + what
            assert np.array_equal(_words(torch, a.di), _words(torch, b.di)), "wire indices: " + what
            assert np.array_equal(_words(torch, a.dv), _words(torch, b.dv)), "wire values: " + what
            assert _bits(comp.state(t.key)) == _bits(twin.state(t.key)), "AIMD state: " + what
            srcs = t.sources(torch, it, 10 * j)
            for d, s in zip(a.g[0 if t.term0 else 1:], srcs[0 if t.term0 else 1:]):
                assert np.array_equal(_words(torch, d), _words(torch, s)), "a source changed: " + what
    comp.check_device()
    twin.check_device()


def test_send16_batch_of_20_matches_fp32_twin(gpu):
    """20 tasks (past the 16-per-launch group): n from 1 to 70,000 with ragged
    sizes and one n = 0, N in {1, 2, 4}, flags 0..3, mixed source types, two
    typed first terms, one task with a null srcs[i]; three consecutive calls."""
    _run_send(gpu, _send_tasks(), 3)


def test_send16_lone_task_takes_the_typed_gather_then_the_plain_scan(gpu):
    """2^22 + 5 floats alone with a bf16 peer: the twin sums its fp32 source
    inside the one-bucket scan, the typed call gathers first; the same bits."""
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    t = Task("lone@g16", (1 << 22) + 5, 2, 3 & 2, [F32, BF16], k=41943)
    comp, twin = ThresholdvCompressor16(), ThresholdvCompressor16()
    a, b = Bufs(torch, gpu, t, True), Bufs(torch, gpu, t, False)
    r0 = torch.from_numpy((synth(t.n, seed_for(499, 0)) * np.float32(0.25)).astype(np.float32))
    a.r.copy_(r0)
    b.r.copy_(r0)
    for it in range(3):
        srcs = t.sources(torch, it, 7)
        a.load(srcs)
        b.load(srcs)
        cn = comp.merge_send_batch_async([a.item(t)])
        co = twin.merge_send_batch_async([b.item(t)])
        torch.cuda.synchronize()
        assert cn.item() == co.item() == t.count
        for x, y, what in ((a.bucket, b.bucket, "bucket"), (a.r, b.r, "residual")):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (it, what)
        assert torch.equal(a.di, b.di) and torch.equal(a.dv, b.dv), it
        assert _bits(comp.state(t.key)) == _bits(twin.state(t.key)), it
    comp.check_device()
    twin.check_device()


@pytest.mark.parametrize("term0", [False, True], ids=["in-place", "typed-term0"])
def test_gather_compress16_matches_fp32_twin(gpu, term0):
    dts = [BF16 if term0 else F32, F16, BF16]
    _run_send(gpu, [Task("gc@g16", 70001, 3, 0, dts, term0=term0)], 3, single=True)


# ---- 4. refusals ----

def test_gather16_refusals(gpu):
    import torch
    from stellatrain_amd import SendTasks, ThresholdvCompressor16, gather_add
    from stellatrain_amd._capi import StgGradSrc, StgSendTask, lib
    L = lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = 4099
    f = torch.ones(n, dtype=torch.float32, device=gpu)
    h = torch.ones(n + 1, dtype=torch.float16, device=gpu)
    with pytest.raises(ValueError, match="needs a float32 bucket"):
        gather_add([h[:n], f], None, 0)
    ga = L.stg_gather_add_typed_device

    def srcs(*pairs):
        return (StgGradSrc * len(pairs))(*[StgGradSrc(p, d) for p, d in pairs])

    bad = {
        b"dtype": srcs((None, 0), (h.data_ptr(), 3)),
        b"aligned": srcs((None, 0), (h.data_ptr() + 1, F16)),
        b"null source": srcs((None, 0), (None, BF16)),
    }
    for word, arr in bad.items():
        assert ga(C.c_void_p(f.data_ptr()), None, arr, 2, n, 0, sp) == -1 and word in L.stg_last_error(), word
    assert ga(C.c_void_p(f.data_ptr()), None, srcs((f.data_ptr() + 2, F32), (h.data_ptr(), F16)), 2, n, 0, sp) == -1
    torch.cuda.synchronize()
    assert bool((f == 1).all().item())

    # the send call: all or nothing, the task named, no key state, every output as preset
    tasks = [Task(f"r{j}@g16", n, 2, j, [F32, (BF16, F16)[j]]) for j in range(2)]
    bufs = [Bufs(torch, gpu, t, True) for t in tasks]
    for t, b in zip(tasks, bufs):
        b.load(t.sources(torch, 0, 3))
        b.r.fill_(0.5)
    good = SendTasks([b.item(t) for t, b in zip(tasks, bufs)])
    good.counts.fill_(-7)
    snap = [[x.clone() for x in b.g + [b.r, b.di, b.dv]] for b in bufs]
    comp = ThresholdvCompressor16()
    fs = L.stg_merge_send_batch_typed_device
    g1 = bufs[1].g
    spoil = {
        "unknown dtype": (srcs((None, 0), (g1[1].data_ptr(), 7)), b"dtype"),
        "odd pointer": (srcs((None, 0), (g1[1].data_ptr() + 1, F16)), b"aligned"),
        "null source": (srcs((None, 0), (None, F16)), b"null source"),
        "odd typed term0": (srcs((g1[1].data_ptr() + 1, BF16), (g1[1].data_ptr(), F16)), b"aligned"),
    }
    for what, (arr, word) in spoil.items():
        ptrs = (C.POINTER(StgGradSrc) * 2)()
        ptrs[0] = good.srcs[0]
        ptrs[1] = arr
        assert fs(comp._h, good.array, ptrs, 2, sp) == -1, what
        msg = L.stg_last_error()
        assert msg.startswith(b"task 1:") and word in msg, (what, msg)
        torch.cuda.synchronize()
        assert comp.state(tasks[0].key) is None and comp.state(tasks[1].key) is None, what
        assert good.counts.cpu().numpy().tolist() == [-7, -7], what
        for b, before in zip(bufs, snap):
            for x, y in zip(b.g + [b.r, b.di, b.dv], before):
                assert np.array_equal(_words(torch, x), _words(torch, y)), what
    assert isinstance(good.array[0], StgSendTask)
    # the untouched arrays still run
    comp.merge_send_batch_async(good)
    torch.cuda.synchronize()
    assert good.counts.cpu().numpy().tolist() == [t.count for t in tasks]
    comp.check_device()
