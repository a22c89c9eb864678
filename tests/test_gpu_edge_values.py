"""GPU parity on the values a mixed-precision overflow step hands the sending
side: infinities, finite lines whose |x| sum overflows, denormals, -0.0 and
magnitudes over the whole exponent range (tests/edge_values.py).

Everything is compared with the oracle bit for bit -- counts, whole streams,
threshold state -- and the oracle is pinned to the reference on the same
inputs by tests/test_oracle_golden_edge.py.  NaN (steady state only) has a
file of its own, test_gpu_edge_nan.py.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from edge_values import FINITE_KINDS, distinct, draws, edge_input
from parity import assert_same_stream, assert_topk_values, bits, fbits
from stellatrain_amd.synth import D1, D3, seed_for, synth
from test_gpu_send_batch import Case as SendCase, _run as _run_send

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
INF_BITS = 0x7F800000
SIZES = [(4103, 40), (65541, 655), ((1 << 20) + 13, 10485)]
# The one-bucket sequences' seed bucket: the first (of 100, 101, ...) at which,
# on the CPU oracle, every size whose threshold stays finite meets both
# regimes in its 8 calls, for every kind; asserted in the test.
SEED_BUCKET = 100


def _tv16_call(gpu, oracle, comp, ho, key, src, k, off=0):
    """One thresholdv16 call on both sides: count, whole stream, state bits.
    Returns the oracle's (state before, state after)."""
    import torch
    t_before = oracle.tv16_state(ho, key)
    co, io, vo = oracle.tv16_compress(ho, key, src, k, idx_offset=off)
    idx = torch.zeros(k, dtype=torch.int32, device=gpu)
    val = torch.zeros(k, dtype=torch.float32, device=gpu)
    cg = comp.compress(key, torch.from_numpy(src).to(gpu), k, idx, val, off)
    assert cg == co
    assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, co, key)
    so, sg = oracle.tv16_state(ho, key), comp.state(key)
    assert bits(np.array(so, np.float32)).tolist() == bits(np.array(sg, np.float32)).tolist(), key
    return t_before, so


@pytest.mark.parametrize("kind", FINITE_KINDS)
def test_thresholdv16_edge(gpu, oracle, kind):
    """One-bucket calls, 8 per size; both regimes among the later calls of
    every size.  `inf` and `huge` pin t = inf at the small sizes (5 and 4 inf
    line sums against k / 16 = 2) and wide_exp's sums overflow often enough to
    do the same at 65541, so a size whose threshold ends at inf is exempt and
    the kind must then meet both regimes at another size."""
    from stellatrain_amd import ThresholdvCompressor16
    comp = ThresholdvCompressor16()
    ho = oracle.tv16_new()
    union = set()
    for n, k in SIZES:
        key = f"{kind}{n}@w"
        regimes = set()
        for it in range(8):
            t_before, so = _tv16_call(gpu, oracle, comp, ho, key, edge_input(kind, n, SEED_BUCKET, it), k)
            if kind == "inf_first":
                assert [fbits(so[0]), fbits(so[1])] == [INF_BITS, INF_BITS], (n, it)
            elif t_before is not None and so[0] != t_before[0]:
                regimes.add("B" if so[0] < t_before[0] else "A")
        if fbits(so[0]) != INF_BITS:
            assert regimes == {"A", "B"}, (n, regimes)
        union |= regimes
    comp.check_device()
    oracle.tv16_free(ho)
    if kind != "inf_first":
        assert union == {"A", "B"}, union


def test_thresholdv16_edge_batch(gpu, oracle):
    """One batched launch of 9 buckets: every kind, mixed sizes, idx offsets,
    and a repeated key that splits the batch (its second call sees the
    threshold its first call wrote)."""
    import torch
    from stellatrain_amd import ThresholdvCompressor16
    spec = [(f"e{j}@w", kind, *SIZES[(j + 1) % 3], 7 * j) for j, kind in enumerate(FINITE_KINDS)]
    spec.insert(5, spec[1])  # (inf_first at 2^20 + 13, again)
    spec.append(("e8@w", "wide_exp", *SIZES[0], 0))
    assert len(spec) == 9
    comp = ThresholdvCompressor16()
    ho = oracle.tv16_new()
    for it in range(8):
        items, ref = [], []
        for j, (key, kind, n, k, off) in enumerate(spec):
            src = edge_input(kind, n, 70 + j, it)
            co, io, vo = oracle.tv16_compress(ho, key, src, k, idx_offset=off)
            ref.append((co, io, vo, oracle.tv16_state(ho, key)))
            items.append((key, torch.from_numpy(src).to(gpu), k, torch.zeros(k, dtype=torch.int32, device=gpu),
                          torch.zeros(k, dtype=torch.float32, device=gpu), off))
        counts = comp.compress_batch_async(items).cpu().numpy()
        torch.cuda.synchronize()
        last = {}
        for j, ((key, _, k, idx, val, off), (co, io, vo, so)) in enumerate(zip(items, ref)):
            assert counts[j] == co, (it, j)
            assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, co, f"call {it} {key}")
            last[key] = so
        for key, so in last.items():
            assert bits(np.array(so, np.float32)).tolist() == bits(np.array(comp.state(key), np.float32)).tolist(), key
    comp.check_device()
    oracle.tv16_free(ho)


# ---- each way of ordering the fill ----

def _fill_child(mode: int):
    env = dict(os.environ, STG_DEBUG_TV16_FILL=str(mode))
    r = subprocess.run([sys.executable, os.path.join(HERE, "edge_fill_child.py")],
                       capture_output=True, text=True, timeout=110, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4], ids=["production", "shadow", "literal", "leader", "crew"])
def test_edge_fill_modes(gpu, mode):
    """denorm_all, wide_exp, huge and negzero through every way the regime-B
    fill orders its pops (edge_fill_child.py checks every stream against the
    oracle); the forced way's counter shows it ran."""
    out = _fill_child(mode)
    assert out["ok"], out
    none, by_start, shadow, literal = out["paths"]
    leader, crew, leader_lit, crew_lit = out["wide"]
    forced = {1: shadow, 2: literal, 3: leader, 4: crew}
    if mode:
        assert forced[mode] > 0, out


# ---- threshold-v ----

@pytest.mark.parametrize("kind,n,k", [(kind, n, k) for kind in FINITE_KINDS for (n, k) in SIZES[1:]] +
                         [("wide_exp", (1 << 22) + 3, 1 << 21)])
def test_thresholdv_edge(gpu, oracle, kind, n, k):
    """((1 << 22) + 3, k = n / 2: most workgroups' LDS lists overflow and the
    units are read again, csrc/tv.hip tv_steal.)"""
    import torch
    from stellatrain_amd import ThresholdvCompressor
    comp = ThresholdvCompressor()
    ho = oracle.tv_new()
    d = torch.empty(n, dtype=torch.float32, device=gpu)  # one stable buffer: pointer-keyed state
    for it in range(8):
        src = edge_input(kind, n, 63, it)
        co, io, vo = oracle.tv_compress(ho, 1, src, k)
        d.copy_(torch.from_numpy(src))
        idx = torch.zeros(k, dtype=torch.int32, device=gpu)
        val = torch.zeros(k, dtype=torch.float32, device=gpu)
        assert comp.compress("ignored", d, k, idx, val) == co, it
        assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, co, f"call {it}")
        st = comp.state("", key_ptr=d.data_ptr())
        assert fbits(st[0]) == fbits(oracle.tv_state(ho, 1)), it
    comp.check_device()
    oracle.tv_free(ho)


# ---- top-k ----

def _topk_call(gpu, oracle, comp, key, src, k, bug_compat):
    """One call against the oracle; returns the oracle's T (the k-th magnitude)."""
    import torch
    co, io, vo = oracle.topk_compress(src, k, bug_compat=bug_compat)
    idx = torch.zeros(k, dtype=torch.int32, device=gpu)
    val = torch.zeros(k, dtype=torch.float32, device=gpu)
    assert comp.compress(key, torch.from_numpy(src).to(gpu), k, idx, val) == co
    if bug_compat:
        np.testing.assert_array_equal(idx.cpu().numpy(), np.arange(k))
        assert_topk_values(val.cpu().numpy(), vo)
    else:
        assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, k, key)
    return np.abs(vo[:k]).min()


@pytest.mark.parametrize("kind", FINITE_KINDS)
@pytest.mark.parametrize("bug_compat", [False, True])
def test_topk_edge(gpu, oracle, kind, bug_compat):
    from stellatrain_amd import TopkCompressor
    comp = TopkCompressor(exact=not bug_compat)
    for n, k in [(4099, 41), (65536, 8192), (1 << 20, 10485)]:
        _topk_call(gpu, oracle, comp, f"{kind}{n}", edge_input(kind, n, 65, 0), k, bug_compat)
    comp.check_device()


def _scaled(x, s):
    return (x.astype(np.float64) * s).astype(np.float32)


@pytest.mark.parametrize("bug_compat", [False, True])
def test_topk_edge_hints(gpu, oracle, bug_compat):
    """One key steered through every hint topk1.hip's band_of tells apart: a
    denormal T, T = inf, T = 0, and a normal T within 2^10 ulps of
    0x00800000 (whose band's lower end drops into the denormals).  Each
    call's T is the oracle's, and the property a call is there for is asserted
    on it; the call after it is the one the hint steers.  (The shipped mode
    sees the first n / 4 floats only, so the plants go there.)"""
    from stellatrain_amd import TopkCompressor
    comp = TopkCompressor(exact=not bug_compat)
    n, k = (1 << 20) + 17, 10485
    d1 = lambda c: synth(n, seed_for(67, c), D1)
    many_inf = d1(5)
    pos = distinct(draws("topk_inf", 67, 5, 4 * k), n // 4, 2 * k)
    many_inf[pos] = np.where(pos & 1, np.float32(-np.inf), np.float32(np.inf))
    # the k-th magnitude of a D1 bucket, then the scale that puts it 2^9 ulps above FLT_MIN
    probe = [d1(9), d1(10)]
    near = []
    for x in probe:
        t0 = np.abs(oracle.topk_compress(x, k, bug_compat=bug_compat)[2][:k]).min()
        near.append(_scaled(x, float(np.uint32(0x00800200).view(np.float32)) / float(t0)))
    seq = [("d1", d1(0)), ("d1", d1(1)), ("denorm", edge_input("denorm_all", n, 67, 2)),
           ("denorm", edge_input("denorm_all", n, 67, 3)), ("d1", d1(4)), ("inf", many_inf), ("d1", d1(6)),
           ("zero", synth(n, seed_for(67, 7), D3, 9995)), ("d1", d1(8)), ("near_min", near[0]), ("near_min", near[1])]
    for c, (what, src) in enumerate(seq):
        T = _topk_call(gpu, oracle, comp, "steer", src, k, bug_compat)
        tb = fbits(T)
        if what == "denorm":
            assert 0 < tb < 0x00800000, (c, T)
        elif what == "inf":
            assert tb == INF_BITS, (c, T)
        elif what == "zero":
            assert tb == 0, (c, T)
        elif what == "near_min":
            assert 0x00800000 <= tb < 0x00800000 + (1 << 10), (c, hex(tb))
        else:
            assert 0x30000000 < tb < 0x40000000, (c, T)  # an ordinary normal magnitude
    comp.check_device()


# ---- send path ----

class EdgeSendCase(SendCase):
    """test_gpu_send_batch.Case with values planted in every source and in the
    initial residual, at positions fixed per case: 3e38 + 3e38 at one (inf
    after the gather), 64 denormals (the sum stays denormal) and 2000 times
    -0.0 + -0.0.  With `nan_from` set, +inf and -inf meet at another position
    from that call on: a NaN born inside the gather, in steady state
    (test_gpu_edge_nan.py runs that variant in a child process)."""

    nan_from = None

    def _pos(self):
        return distinct(draws("send", 700 + self.seed, 0, 4096), self.n, 2 + 64 + 2000)

    def _plant(self, x):
        p = self._pos()
        x[p[2:66]] = _scaled(x[p[2:66]], 1e-36)
        x[p[66:]] = np.float32(-0.0)
        return x

    def grads(self, it):
        g = [self._plant(x.copy()) for x in SendCase.grads(self, it)]
        p = self._pos()
        for r, x in enumerate(g):
            x[p[0]] = np.float32(3e38)
            if self.nan_from is not None and it >= self.nan_from:
                x[p[1]] = np.float32(-np.inf if r else np.inf)
        return g

    def resid0(self):
        return self._plant(SendCase.resid0(self).copy())


def send_edge_cases(nan_from=None):
    from stellatrain_amd import merge_numel, wire_flag
    n = 60000
    cases = [EdgeSendCase(f"edge{j}@s", n, merge_numel(n, 0.99), wire_flag(n), 2, seed=80 + j) for j in range(4)]
    for c in cases:
        c.nan_from = nan_from
    return cases


def test_send_edge(gpu, oracle):
    """CodecEngine.send_buckets, 2 sources, 4 tensors of 60,000 floats, 4
    iterations, against the per-tensor oracle chain of test_gpu_send_batch.py:
    residual bits, wire words and state.  (thresholdv16 sends lines in index
    order, so the inf goes out in some calls and stays in the residual, still
    inf, in the others.)"""
    seen = {"inf": 0, "negzero": 0, "denorm": 0}

    def hook(it, j, c, idx, g0):
        p = c._pos()
        seen["inf"] += int(g0[p[0]] == 0 if p[0] in idx else fbits(g0[p[0]]) == INF_BITS)
        seen["negzero"] += int((bits(g0[p[66:]]) == 0x80000000).any())
        seen["denorm"] += int((((bits(g0[p[2:66]]) & 0x7FFFFFFF) - 1) < 0x007FFFFF).any())

    _run_send(gpu, oracle, send_edge_cases(), calls=4, mode="engine", hook=hook)
    assert all(v == 16 for v in seen.values()), seen


# ---- host path ----

def test_host_path_edge(gpu, oracle):
    """stg_codec_compress_host (numpy in and out) on wide_exp, idx_offset 5."""
    from stellatrain_amd import ThresholdvCompressor16
    comp = ThresholdvCompressor16()
    ho = oracle.tv16_new()
    n, k = 200003, 2000
    for it in range(4):
        src = edge_input("wide_exp", n, 69, it)
        co, io, vo = oracle.tv16_compress(ho, "h", src, k, idx_offset=5)
        idx = np.zeros(k, np.uint32)
        val = np.zeros(k, np.float32)
        assert comp.compress("h", src, k, idx, val, 5) == co
        assert_same_stream(idx, val, io, vo, co, f"call {it}")
        assert bits(np.array(oracle.tv16_state(ho, "h"), np.float32)).tolist() == \
            bits(np.array(comp.state("h"), np.float32)).tolist()
    comp.check_device()
    oracle.tv16_free(ho)
