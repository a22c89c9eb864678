"""GPU parity of the one-call send path on an exact top-k handle
(``stg_merge_send_batch_device`` / ``..._typed_device`` with ``"topk_exact"``,
``Compressor.merge_send_batch_async``, ``CodecEngine.send_buckets``): the
batched select and ordered emission of csrc/topk_batch.hip and the shared
finish.

Every comparison is whole-buffer and bit for bit, against both
(a) the oracle -- ``gather_add``, ``topk_compress(bug_compat=False)`` into
    zeroed slots, the wire form of all ``W = min(idx_cap, n)`` slots, numpy
    error feedback over all ``idx_cap`` slots (tests/topk_send_cases.py
    ``Ref``) -- for finite inputs, and
(b) a twin ``TopkCompressor(exact=True)`` running the per-tensor sequence on
    copies (``merge_gather_compress_async`` into zeroed u32 / f32 temporaries
    of ``idx_cap`` slots, then ``wire_encode`` of the first ``W``):
grad[0], the residual, the first ``W`` wire elements, the ``-1`` sentinel past
``W``, the count, the bits of ``state(key)[0]`` on both sides -- which must also
be the oracle's k-th magnitude; ``check_device()`` clean on both sides.
tests/test_topk_send_host.py shows, by the oracle alone, which situations the
sequences reach."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import topk_send_cases as T

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
        def buf(n, dt=torch.float32, shift=c.shift):  # shift: a view offset by one float, another 16-byte phase
            return torch.zeros(n + 1, dtype=dt, device=gpu)[1:] if shift else torch.zeros(n, dtype=dt, device=gpu)
        self.g = [buf(c.n, shift=c.shift0)]
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

    def tensors(self):
        return self.g + ([self.r] if self.r is not None else []) + [self.di, self.dv]


def _twin_step(torch, twin, key, c, sd):
    """Comparison (b): the per-tensor sequence on the twin's buffers."""
    from stellatrain_amd import wire_encode
    ti = torch.zeros(c.cap, dtype=torch.int32, device=sd.di.device)
    tv = torch.zeros(c.cap, dtype=torch.float32, device=sd.di.device)
    cnt = twin.merge_gather_compress_async(key, sd.g, c.k, ti, tv, residual=sd.r, idx_offset=c.off)
    if c.W:
        wire_encode(ti[:c.W], tv[:c.W], c.flag, idx_out=sd.di, val_out=sd.dv)
    return cnt


def _same(a, b, what):
    assert np.array_equal(_u(a.cpu().numpy()), _u(b.cpu().numpy())), what


def _sentinel(t, count):
    return bool((t[count:] == -1).all().item())


class Runner:
    """Both GPU sides and the oracle side of a list of cases, call after call."""

    def __init__(self, gpu, oracle, cases, mode="items", n_oracle=None, finite=True):
        import torch
        from stellatrain_amd import CodecEngine, TopkCompressor
        self.torch, self.gpu, self.o, self.cases, self.mode = torch, gpu, oracle, cases, mode
        self.eng = None
        if mode == "engine":
            self.eng = CodecEngine()
            self.eng.configure("topk_exact")
        self.comp = self.eng.compressor() if self.eng else TopkCompressor(exact=True)
        assert self.comp.name() == "Topk"
        self.twin = TopkCompressor(exact=True)
        self.new = [Side(torch, gpu, c) for c in cases]
        self.old = [Side(torch, gpu, c) for c in cases]
        n_oracle = len(cases) if n_oracle is None else n_oracle
        self.ref = [T.Ref(oracle, c) if finite and j < n_oracle and c.n else None for j, c in enumerate(cases)]
        self.counts = torch.full((len(cases),), -1, dtype=torch.int32, device=gpu)
        self.pre = {}

    @staticmethod
    def key(j):
        return f"layer{j}.weight"

    def item(self, j):
        c, s = self.cases[j], self.new[j]
        return (self.key(j), s.g, c.k, s.di, s.dv, s.r, c.flag, c.off)

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
            streams, cnt = self.eng.send_buckets([(self.key(j), self.new[j].g, self.new[j].r) if cases[j].resid else
                                                  (self.key(j), self.new[j].g) for j in live])
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
        tcnt = {j: _twin_step(torch, self.twin, self.key(j), cases[j], self.old[j]) for j in live if cases[j].n}
        torch.cuda.synchronize()
        for pos, j in enumerate(live):
            c, a, b = cases[j], self.new[j], self.old[j]
            what = f"call {it}, task {j} ({c})"
            if not c.n:
                assert got[pos] == 0, what
                assert _sentinel(a.di, 0) and _sentinel(a.dv, 0), what
                continue
            assert got[pos] == int(tcnt[j].item()) == c.cap, "count vs twin: " + what
            _same(a.g[0], b.g[0], "grad[0] vs twin: " + what)
            if c.resid:
                _same(a.r, b.r, "residual vs twin: " + what)
                _same(a.r, a.g[0], "residual vs grad[0]: " + what)
            _same(a.di[:c.W], b.di[:c.W], "wire indices vs twin: " + what)
            _same(a.dv[:c.W], b.dv[:c.W], "wire values vs twin: " + what)
            ta, tb = self.comp.state(self.key(j)), self.twin.state(self.key(j))
            assert ta is not None and tb is not None and _fbits(ta[0]) == _fbits(tb[0]), "state vs twin: " + what
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
            assert _fbits(ta[0]) == st.T, "state vs the oracle's k-th magnitude: " + what
            if hook:
                hook(it, j, c, st, g0)

    def check(self):
        self.comp.check_device()
        self.twin.check_device()


def _run(gpu, oracle, cases, calls, mode="items", hook=None, finite=True):
    r = Runner(gpu, oracle, cases, mode, finite=finite)
    for it in range(calls):
        r.call(it, hook=hook)
    r.check()
    return r


# ---- single tasks ----

@pytest.mark.parametrize("n", T.SINGLE_N)
def test_topk_send_single_task(gpu, oracle, n):
    """One task per call, three calls: flags 0-3, N in {1, 2, 9}, with and
    without a residual, residual, sources and once the bucket at another
    16-byte phase, k in {1, max(1, n // 100), n}, idx_cap above k."""
    for c in T.single_cases(n):
        _run(gpu, oracle, [c], calls=3)


# ---- the situations of tests/test_topk_send_host.py ----

def test_topk_send_ties_partly_taken_across_tiles(gpu, oracle):
    """The k-th magnitude is shared by more elements than are taken, in more
    than one tile and with both signs: the first ones in index order win."""
    seen = []

    def hook(it, j, c, st, g0):
        seen.append((st.eq_taken, st.n_eq, len(st.eq_tiles), st.eq_signs == {False, True}))

    _run(gpu, oracle, [T.TIES], calls=T.TIES_CALLS, hook=hook)
    assert all(0 < t < e and tiles > 1 and signs for t, e, tiles, signs in seen), seen


def test_topk_send_zero_threshold(gpu, oracle):
    """T = 0: every non-zero wins and zeros are taken in index order; the
    state holds +0.0."""
    ts = []

    def hook(it, j, c, st, g0):
        ts.append(st.T)

    _run(gpu, oracle, [T.ZEROS], calls=T.ZEROS_CALLS, hook=hook)
    assert ts == [0] * T.ZEROS_CALLS


@pytest.mark.parametrize("name", sorted(T.SEQ_CASES))
def test_topk_send_sequence(gpu, oracle, name):
    """SCALES twice through with the residual carried: winners that come from
    residual mass alone; for n = 60,000 under flag 1, u16 indices past 32,767
    zeroed by their true index."""
    seen = {"resid": 0, "high": 0}

    def hook(it, j, c, st, g0):
        seen["resid"] += st.from_resid
        ix = st.idx[:c.kk]
        seen["high"] += int((ix > 32767).sum())
        assert (g0[ix] == 0).all()

    c = T.SEQ_CASES[name]
    _run(gpu, oracle, [c], calls=T.SEQ_CALLS, hook=hook)
    assert seen["resid"] and (seen["high"] or c.n <= 32768), seen


def test_topk_send_ragged_tail_element_selected(gpu, oracle):
    """A winner among the last n % 4 elements of the last, partial tile is on
    the wire and zeroed by its index."""
    hit = []

    def hook(it, j, c, st, g0):
        t = st.idx[:c.kk][st.idx[:c.kk] >= c.n // 4 * 4]
        hit.append(t.size)
        assert (g0[t] == 0).all()

    _run(gpu, oracle, [T.tail_case()], calls=T.TAIL_CALLS, hook=hook)
    assert max(hit) > 0, hit


@pytest.mark.parametrize("case", [T.CAP_PAST_K, T.CAP_PAST_N], ids=["past_k", "past_n"])
def test_topk_send_capacity_past_k_and_n(gpu, oracle, case):
    """idx_cap > k: slots [k, W) are the wire form of (0, 0.0) and element 0
    is zeroed; idx_cap = 48 > n = 40: W = 40 slots are written, the other 8
    keep the sentinel."""
    zeroed = []

    def hook(it, j, c, st, g0):
        zeroed.append(g0[0] == 0 and st.bucket[0] != 0)

    _run(gpu, oracle, [case], calls=3, hook=hook)
    assert all(zeroed)


def test_topk_send_nan_and_infinity(gpu, oracle):
    """NaNs (from the third call on, carried by the residual after it) and
    infinities: a NaN ranks above infinity, as per tensor.  Against the twin."""
    assert np.isnan(T.NAN_CASES[0].grads(2)[0]).sum() == 5 and np.isinf(T.NAN_CASES[1].grads(0)[0]).sum() == 5
    r = _run(gpu, oracle, T.NAN_CASES, calls=T.NAN_CALLS, finite=False)
    # k = 3 of five NaNs: the k-th magnitude itself is a NaN, and the state holds it
    j = [c.k for c in T.NAN_CASES].index(3)
    assert np.isnan(r.comp.state(r.key(j))[0]) and np.isnan(r.twin.state(r.key(j))[0])


# ---- 40 tasks ----

@pytest.mark.parametrize("mode", ["items", "prebuilt", "engine"])
def test_topk_send_batched_40_tasks(gpu, oracle, mode):
    """Sizes 1 to 300,007 (one to 37 tiles), an empty task in the middle, one
    bf16 source (the typed entry point), keys that first appear at call 2 --
    fresh and steady keys in one group."""
    cases = T.batch_cases(mode == "engine")
    r = Runner(gpu, oracle, cases, mode, n_oracle=12)
    for it in range(T.BATCH_CALLS):
        r.call(it, live=T.batch_live(it))
    r.check()


def test_topk_send_one_task_over_the_tile_cap_runs_alone(gpu, oracle):
    """One tile more than a group takes on this device: the task runs through
    the per-tensor top-k between two shared groups, and the shared finish
    packs it."""
    import torch
    from stellatrain_amd._capi import lib
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    sizes, first, launch, cap = (C.c_uint64 * 3)(1000, 1, 4099), (C.c_uint32 * 3)(), (C.c_uint32 * 3)(), C.c_uint32()
    assert lib().stg_debug_topk_batch_plan(sizes, 3, cus, first, launch, C.byref(cap)) == 1
    big = (cap.value + 1) * T.TILE - 5
    sizes[1] = big
    assert lib().stg_debug_topk_batch_plan(sizes, 3, cus, first, launch, C.byref(cap)) == 3
    assert list(launch) == [0, 1, 2] and T.tiles_of(big) == cap.value + 1
    cases = [T.Case(1000, 10, 1, 2, seed=91), T.Case(big, big // 100, 3, 2, seed=92), T.Case(4099, 41, 0, 1, seed=93)]
    _run(gpu, oracle, cases, calls=2)


# ---- interleaving with the per-tensor call ----

def test_topk_send_interleaves_with_per_tensor_compress(gpu, oracle):
    """One handle, one key: batched, per-tensor ``compress``, batched,
    per-tensor.  The per-tensor call is steered by the state the batched call
    left and the other way round; every call is exact."""
    import torch
    from stellatrain_amd import TopkCompressor
    c = T.Case(60000, 600, 0, 1, seed=94, resid=False, scales=[1.0, 1.03, 0.5, 1.0])
    comp, key = TopkCompressor(exact=True), "interleaved.weight"
    sd = Side(torch, gpu, c)
    for it in range(4):
        x = c.grads(it)[0]
        sd.load(torch, [x])
        _, io, vo = oracle.topk_compress(x, c.k, bug_compat=False)
        if it % 2 == 0:
            cnt = comp.merge_send_batch_async([(key, sd.g, c.k, sd.di, sd.dv, None, c.flag)])
        else:
            cnt = comp.compress_async(key, sd.g[0], c.k, sd.di, sd.dv)
        torch.cuda.synchronize()
        assert int(cnt.cpu().numpy().ravel()[0]) == c.k, it
        assert np.array_equal(_u(sd.di.cpu().numpy()), _u(io)), it
        assert np.array_equal(_u(sd.dv.cpu().numpy()), _u(vo)), it
        assert _fbits(comp.state(key)[0]) == T.kth_bits(x, c.k), it
        comp.check_device()


# ---- refusals: all or nothing ----

def test_topk_send_refusals_change_nothing(gpu):
    import torch
    from stellatrain_amd import SendTasks, TopkCompressor
    from stellatrain_amd._capi import StgSendTask, lib
    L = lib()
    f = L.stg_merge_send_batch_device
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cases = [T.Case(4099, 41, (1, 3, 0)[j], 2, seed=60 + j) for j in range(3)]
    keys = [f"r{j}.weight" for j in range(3)]
    sides = [Side(torch, gpu, c) for c in cases]
    for c, s in zip(cases, sides):
        s.load(torch, c.grads(0))
    comp = TopkCompressor(exact=True)
    comp.merge_send_batch_async([(keys[0], sides[0].g, cases[0].k, sides[0].di, sides[0].dv, sides[0].r,
                                  cases[0].flag)])  # key 0 has state; keys 1 and 2 never compressed
    for c, s in zip(cases, sides):
        s.load(torch, c.grads(1))
    good = SendTasks([(kk, s.g, c.k, s.di, s.dv, s.r, c.flag) for kk, c, s in zip(keys, cases, sides)])
    torch.cuda.synchronize()
    st0, snap = comp.state(keys[0]), [[t.clone() for t in s.tensors()] for s in sides]
    assert st0 is not None

    def unchanged(what):
        torch.cuda.synchronize()
        assert _fbits(comp.state(keys[0])[0]) == _fbits(st0[0]), what
        assert comp.state(keys[1]) is None and comp.state(keys[2]) is None, what
        for s, before in zip(sides, snap):
            for t, b in zip(s.tensors(), before):
                _same(t, b, what)

    null_src = (C.c_void_p * 2)(sides[1].g[0].data_ptr(), None)
    bad = {
        "repeated key": (2, lambda t: setattr(t.bucket, "key", keys[0].encode()), b"key"),
        "flag 4": (1, lambda t: setattr(t, "wire_flag", 4), b"flag"),
        "null source": (1, lambda t: setattr(t, "d_grads", null_src), b"null source"),
        "idx_cap < k": (1, lambda t: setattr(t.bucket, "k", t.bucket.idx_cap + 1), b"Invalid parameter k"),
    }
    for what, (pos, spoil, word) in bad.items():
        arr = (StgSendTask * 3)()
        C.memmove(arr, good.array, C.sizeof(arr))
        spoil(arr[pos])
        assert f(comp._h, arr, 3, sp) == -1, what
        msg = L.stg_last_error()
        assert msg.startswith(b"task %d:" % pos) and word in msg, (what, msg)
        unchanged(what)

    # the untouched array still runs
    comp.merge_send_batch_async(good)
    torch.cuda.synchronize()
    assert good.counts.cpu().numpy().tolist() == [41, 41, 41]
    assert comp.state(keys[1]) is not None
    comp.check_device()


def test_topk_send_still_refuses_the_shipped_topk(gpu):
    """The bug-compatible handle writes idx[i] = i: there are no true indices
    to zero, so the entry keeps returning STG_ERR_UNSUPPORTED and changes
    nothing."""
    import torch
    from stellatrain_amd import SendTasks, TopkCompressor
    from stellatrain_amd._capi import lib
    c = T.Case(4099, 41, 1, 2, seed=63)
    sd = Side(torch, gpu, c)
    sd.load(torch, c.grads(0))
    good = SendTasks([("w", sd.g, c.k, sd.di, sd.dv, sd.r, c.flag)])
    torch.cuda.synchronize()
    snap = [t.clone() for t in sd.tensors()]
    topk = TopkCompressor()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib().stg_merge_send_batch_device(topk._h, good.array, 1, sp) == -4, lib().stg_last_error()
    torch.cuda.synchronize()
    assert topk.state("w") is None
    for t, b in zip(sd.tensors(), snap):
        _same(t, b, "topk handle")
