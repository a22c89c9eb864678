"""GPU checks of the parameter publish (``publish_params`` / ``PublishTasks``,
``stg_param_publish_batch_device``).

Every replica starts as a sentinel that differs from the converted master in
every element, inside a larger tensor with guard words on both sides.  The
expected replica is computed in numpy (tests/publish_cases.py: the sentinel,
with ``cvt(master[j])`` at the published indices; the 16-bit conversions are
the integer models tests/test_publish_host.py pins against torch's CPU
``.to()``) and compared bit for bit over the whole tensor, guards included.
The one exception: where the expected word is a NaN, any NaN passes; NaNs are
kept to at most 1 % of the published elements.

T is the kernel's tile (stream slots per workgroup), read from ws.h; a lane
takes four consecutive slots.
"""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import publish_cases as P
import wire_merge_cases as W

pytestmark = pytest.mark.gpu

_WS_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stellatrain_amd", "csrc", "ws.h")
T = int(re.search(r"constexpr uint32_t PUBLISH_TILE = (\d+);", open(_WS_H).read()).group(1))
COUNTS = [0, 1, 3, 4, 5, T - 1, T, T + 1, 2 * T + 37]
LENS = [8199, 60000]
SHAPES = ["lines", "union", "random", "ends", "planted"]
RSETS = [1, 2, 7, 16]
STALE = 41           # slots past the count, holding valid indices that must not be published
GUARD = 8            # guard words around a replica
OFFS = [1, 0, 2, 3]  # replica r starts OFFS[r % 4] elements into its tensor: 1 = element-aligned only
SPECIAL = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x477fe000, 0x477ff000,
                    0xc7800000, 0x33000000, 0x33000001, 0x387fc000, 0x387fe000, 0x33800000, 0x7f7fffff, 0xff7f8000,
                    0x3f808000, 0x3f818000, 0x3f80ffff], np.uint32)
NANS = np.array([0x7fc00000, 0xffc12345, 0x7f800001, 0x7fffffff], np.uint32)
_BASE = {}


def _base(n):
    """The master before a case plants its specials: finite, over float16's
    overflow, normal, subnormal and underflow ranges."""
    if n not in _BASE:
        rng = np.random.default_rng(n)
        _BASE[n] = (rng.standard_normal(n) * 10.0 ** rng.integers(-9, 7, n)).astype(np.float32)
    return _BASE[n]


def _indices(shape, n, c, seed):
    """The first c stream slots of one shape (uint32)."""
    rng = np.random.default_rng([SHAPES.index(shape), n, c, seed])
    if shape == "lines":  # aligned lines of 16 consecutive indices, as thresholdv16 emits them; the last one cut
        lines = rng.choice(n // 16, (c + 15) // 16, replace=False)
        return (lines[:, None] * 16 + np.arange(16)[None, :]).reshape(-1)[:c].astype(np.uint32)
    if shape == "union":  # index-ascending; runs start at phases 1, 2, 3 and cross lane groups and the tile edge
        out, pos, k = [], 5, 0
        lens, gaps = [7, 1, 18, 3, 33, 2, 5], [3, 9, 2, 30]
        while len(out) < c:
            ln = lens[k % len(lens)]
            if T - 33 <= len(out) < T:
                ln = max(ln, T - len(out) + 5)  # this run crosses the tile edge
            pos += (1 + k % 3 - pos) % 4
            out.extend(range(pos, pos + ln))
            pos += ln + gaps[k % len(gaps)]
            k += 1
        out = np.array(out[:c], np.uint32)
        assert out[-1] < n and (c <= T or out[T] == out[T - 1] + 1)
        return out
    if shape == "random":
        return rng.choice(n, c, replace=False).astype(np.uint32)
    if shape == "ends":  # index 0, and index n - 1 ending a run
        run = min(5, c - 1)
        mid = 10 + rng.choice(n - 30, c - 1 - run, replace=False)
        return np.concatenate([[0], mid, np.arange(n - run, n)]).astype(np.uint32)
    out = rng.choice(n, c, replace=False).astype(np.uint32)  # planted: one index >= n, one repeat
    out[c // 2] = n + 5 if c % 2 else 0xfffffff0
    out[c - 1] = out[0]
    return out


def _fits(shape, c):
    return c >= 3 if shape in ("ends", "planted") else (c > 0 or shape == "lines")


def _case(shape, n, c, seed=0):
    """(master, idx buffer of c + STALE slots, stale indices): specials
    planted at published positions, NaNs at no more than 1 in 128 of them."""
    idx = _indices(shape, n, c, seed)
    valid = np.unique(idx[idx < n])
    rng = np.random.default_rng([7, SHAPES.index(shape), n, c, seed])
    master = _base(n).copy()
    mu = master.view(np.uint32)
    sp = valid[::3]
    mu[sp] = SPECIAL[np.arange(sp.size) % SPECIAL.size]
    nn = valid[5::128]
    mu[nn] = NANS[np.arange(nn.size) % NANS.size]
    rest = np.setdiff1d(np.arange(n, dtype=np.uint32), valid)
    stale = rng.choice(rest, STALE, replace=False).astype(np.uint32)
    return master, np.concatenate([idx, stale]).astype(np.uint32), stale


def _dtypes(R, rot):
    return [(r + rot) % 3 for r in range(R)]


class _Rep:
    """One replica on the device: `words` (the sentinel) OFFS elements into a
    tensor of guard words."""

    def __init__(self, torch, gpu, words, dtype, r):
        self.dtype, self.n, self.off = dtype, words.size, GUARD + OFFS[r % 4]
        self.g = words.dtype.type(0xa5a5a5a5 if words.dtype == np.uint32 else 0xa5a5)
        raw = np.full(self.n + 2 * GUARD + 4, self.g, words.dtype)
        raw[self.off:self.off + self.n] = words
        self.start = raw
        self.big = torch.from_numpy(raw.view(np.int32 if dtype == P.DT_F32 else np.int16)).to(gpu)
        tdt = {P.DT_F32: torch.float32, P.DT_BF16: torch.bfloat16, P.DT_F16: torch.float16}[dtype]
        self.t = self.big[self.off:self.off + self.n].view(tdt)
        assert self.t.data_ptr() == self.big.data_ptr() + self.off * self.big.element_size()

    def read(self):
        raw = self.big.cpu().numpy().view(self.start.dtype)
        body = raw[self.off:self.off + self.n]
        guards = np.concatenate([raw[:self.off], raw[self.off + self.n:]])
        assert (guards == self.g).all(), "a guard word was written"
        return body


def _sentinel(master, dtype):
    return ~P.cvt_bits(master, dtype)


def _same(got, exp, dtype):
    nan = P.is_nan_bits(exp, dtype)
    return (got == exp) | (nan & P.is_nan_bits(got, dtype))


class _Task:
    """A publish task on the device with its numpy expectation."""

    def __init__(self, torch, gpu, shape, n, c, R, rot, seed=0, count_word=None):
        self.master, idx, self.stale = _case(shape, n, c, seed)
        self.c, self.idx = c, idx
        self.param = torch.from_numpy(self.master).to(gpu)
        self.d_idx = torch.from_numpy(idx.view(np.int32)).to(gpu)
        word = c if count_word is None else count_word
        self.d_cnt = torch.from_numpy(np.array([word], np.uint32).view(np.int32)).to(gpu)
        self.word = word
        self.reps = [_Rep(torch, gpu, _sentinel(self.master, d), d, r) for r, d in enumerate(_dtypes(R, rot))]

    def item(self):
        return (self.param, self.d_idx, self.d_cnt, [r.t for r in self.reps])

    def check(self, what):
        assert np.array_equal(self.param.cpu().numpy().view(np.uint32), self.master.view(np.uint32)), what
        for r, rep in enumerate(self.reps):
            sent = _sentinel(self.master, rep.dtype)
            exp, pub = P.expected_replica(sent, self.master, self.idx, self.word, rep.dtype)
            nan = P.is_nan_bits(exp, rep.dtype) & pub
            assert nan.sum() * 100 <= pub.sum(), what                   # NaNs: at most 1 % of what is published
            assert not (exp[pub] == sent[pub]).any()                    # every published element must change
            got = rep.read()
            ok = _same(got, exp, rep.dtype)
            assert ok.all(), (what, r, rep.dtype, rep.off, np.flatnonzero(~ok)[:8])
            assert (got[self.stale] == sent[self.stale]).all(), what    # slots past the count are ignored
        return self


@pytest.mark.parametrize("n", LENS)
@pytest.mark.parametrize("shape", SHAPES)
def test_single_task(gpu, shape, n):
    """Every count the shape fits x 1, 2, 7 and 16 replicas of mixed types."""
    import torch
    from stellatrain_amd import publish_params
    k = 0
    for c in COUNTS:
        if not _fits(shape, c):
            continue
        for R in RSETS:
            t = _Task(torch, gpu, shape, n, c, R, rot=k)
            k += 1
            publish_params([t.item()])
            t.check((shape, n, c, R))


def test_every_dtype_is_published_from_an_element_aligned_start():
    """The replica sets above put each dtype one element into its tensor."""
    for R in RSETS:
        seen = set()
        for rot in range(3):
            seen |= {d for r, d in enumerate(_dtypes(R, rot)) if OFFS[r % 4] == 1}
        assert seen == {P.DT_F32, P.DT_BF16, P.DT_F16}, R


@pytest.mark.parametrize("word", ["poison", "cap + 1"])
def test_count_above_the_buffer_publishes_nothing(gpu, word):
    import torch
    from stellatrain_amd import publish_params
    for shape, c in (("lines", T + 1), ("random", 5)):
        w = 0xffffffff if word == "poison" else c + STALE + 1
        t = _Task(torch, gpu, shape, 8199, c, 7, rot=1, count_word=w)
        publish_params([t.item()])
        t.check((word, shape))
        for rep in t.reps:
            assert np.array_equal(rep.read(), _sentinel(t.master, rep.dtype))


def test_count_equal_to_the_buffer_publishes_all_of_it(gpu):
    """The last legal count: the stale slots are published too."""
    import torch
    from stellatrain_amd import publish_params
    c = T + 1
    t = _Task(torch, gpu, "union", 8199, c, 2, rot=0, count_word=c + STALE)
    t.stale = np.zeros(0, np.int64)
    publish_params([t.item()])
    t.check("full buffer")


def _batch(torch, gpu, ntasks, seed):
    """ntasks tasks: the counts cycled, a zero-count task after every third,
    shapes, lengths and replica sets cycled."""
    out, k = [], 0
    counts = [c for c in COUNTS if c >= 3]
    for i in range(ntasks):
        if i % 4 == 3:
            out.append(("lines", LENS[i % 2], 0, RSETS[i % 4]))
        else:
            out.append((SHAPES[k % len(SHAPES)], LENS[k % 2], counts[k % len(counts)], RSETS[(k // 2) % 4]))
            k += 1
    return [_Task(torch, gpu, s, n, c, R, rot=i, seed=seed) for i, (s, n, c, R) in enumerate(out)]


@pytest.mark.parametrize("ntasks", [1, 16, 17, 40])
@pytest.mark.parametrize("prebuilt", [False, True])
def test_batch_equals_the_tasks_one_by_one(gpu, ntasks, prebuilt):
    import torch
    from stellatrain_amd import PublishTasks, publish_params
    a, b = _batch(torch, gpu, ntasks, 3), _batch(torch, gpu, ntasks, 3)
    items = [t.item() for t in a]
    publish_params(PublishTasks(items) if prebuilt else items)
    for t in b:
        publish_params([t.item()])
    for i, (ta, tb) in enumerate(zip(a, b)):
        ta.check(("batch", ntasks, i))
        tb.check(("single", ntasks, i))
        for ra, rb in zip(ta.reps, tb.reps):
            ga, gb = ra.read(), rb.read()
            nan = P.is_nan_bits(ga, ra.dtype) & P.is_nan_bits(gb, rb.dtype)
            assert ((ga == gb) | nan).all(), (ntasks, i)


def _up(torch, gpu, a):
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


PR = [1, 7, 9, 1023, 1024, 1025, 4099, 17]


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_closure_over_three_iterations(gpu, oracle, kind, world):
    """The merged indices are all a step changes: a float32 replica that was a
    clone of the parameter, and a bfloat16 one that was its rounding, are
    bitwise the parameter (its rounding) over the whole tensor after every
    publish, on 8 tensors through three iterations."""
    import torch
    from stellatrain_amd import MergeTasks, PublishTasks, SparseAdam, SparseSGD, publish_params
    from stellatrain_amd.engine import scatter_merge_check
    opt = SparseSGD(momentum=0.9) if kind == "sgd" else SparseAdam()
    base = np.random.default_rng(23).standard_normal(1 << 20).astype(np.float32)
    specs = [dict(name=f"c{i}", family=W.FAMILIES[(i // 2) % 2], per_rank=PR[i], flag=i % 4) for i in range(8)]

    def streams(it):
        return [W.make_streams(oracle, s["family"], s["per_rank"], s["flag"], world, seed=100 * it + i,
                               specials=False) for i, s in enumerate(specs)]

    first = streams(0)
    params = [torch.from_numpy(base[:W.n_of(s["flag"])] + np.float32(i)).to(gpu) for i, s in enumerate(specs)]
    dev = [[(_up(torch, gpu, wi), _up(torch, gpu, wv), f) for wi, wv, f in st] for st in first]
    merge = MergeTasks([(p, s["name"], d, s["per_rank"]) for p, s, d in zip(params, specs, dev)])
    f32 = [p.clone() for p in params]
    b16 = [p.to(torch.bfloat16) for p in params]
    pub = PublishTasks.from_merge(merge, [[a, b] for a, b in zip(f32, b16)])
    changed = 0
    for it in range(3):
        if it:
            for d, st in zip(dev, streams(it)):
                for (ti, tv, _), (wi, wv, _) in zip(d, st):
                    ti.copy_(_up(torch, gpu, wi))
                    tv.copy_(_up(torch, gpu, wv))
        before = [p.clone() for p in params]
        opt.merge_optimize_batch(merge)
        publish_params(pub)
        for i, (p, a, b, p0) in enumerate(zip(params, f32, b16, before)):
            hp = p.cpu()
            changed += int((hp != p0.cpu()).sum())
            assert np.array_equal(a.cpu().numpy().view(np.uint32), hp.numpy().view(np.uint32)), (kind, world, it, i)
            assert np.array_equal(b.cpu().view(torch.int16).numpy(),
                                  hp.to(torch.bfloat16).view(torch.int16).numpy()), (kind, world, it, i)
    # The steps did move the parameters.  No more is asked than that: the raw u16 streams drop
    # their block pairs, and an SGD step of lr * value below half an ulp of the parameter (about
    # half the values, which span 1e-9 .. 1e3) leaves its element as it was.
    assert changed > 1000
    scatter_merge_check()
