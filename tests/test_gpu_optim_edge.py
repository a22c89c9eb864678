"""GPU parity of the receiving side on edge values: the MERGE decompress and the
SGD / Adam steps on infinities, overflowing sums, denormals, -0.0, the whole
exponent range and NaNs (inputs: tests/optim_edge.py; the oracle chain
``wire_decode`` -> ``merge_decompress`` -> ``sgd_apply`` / ``adam_apply`` is
pinned to the reference on exactly these inputs by
test_oracle_golden_optim_edge.py).

Every comparison goes through ``parity.assert_same_f32`` (bit-equal; where the
oracle has a NaN the device must have one, of any payload) after every call:
parameter, momentum or m and v, last, vmax, tick and iter.  The device checks
(``check()``, ``check_device()``, ``scatter_merge_check()``) must be clean.

Paths:
  A  optimize_raw (sgd_apply<false/true>, adam_apply, adam_apply_ams)
  B  merge_optimize at world 1: copy and election paths, decoded and wire forms
  C  scatter_merge / scatter_merge_wire at worlds 2-8, scratch handed back zero
  D  merge_optimize at world 3 with the planted sums on shared indices
  E  merge_optimize_batch, world-1 and world-3 tensors, against the oracle and
     the per-tensor twin
"""
from __future__ import annotations

import numpy as np
import pytest

import optim_edge as E
import wire_merge_cases as W
from parity import assert_same_f32

pytestmark = pytest.mark.gpu

# every kind and every configuration once per optimizer (optim_edge._cross's first entries)
HALF = E.SGD_CASES[::2] + E.ADAM_CASES[::2]
_ids = lambda c: c["name"]  # noqa: E731


def _up(gpu, a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(gpu)


def _make(case):
    from stellatrain_amd import SparseAdam, SparseSGD
    return (SparseSGD if case["opt"] == "sgd" else SparseAdam)(**E.cfg_of(case))


def _same_state(case, opt, name, pg, po, st, what):
    """Device parameter and optimizer state of `name` against the oracle's."""
    n = po.size
    assert_same_f32(pg.cpu().numpy(), po, f"{what}: param")
    if case["opt"] == "sgd":
        if "mom" in st:
            assert_same_f32(opt.momentum_buffer(name, n), st["mom"], f"{what}: momentum")
        else:
            assert opt.momentum_buffer(name, n) is None
        if "last" in st:
            assert np.array_equal(opt.last_buffer(name, n), st["last"]), f"{what}: last"
        assert opt.iteration == st["iter"], what
    else:
        m, v, vmax, tick = opt.state(name, n)
        assert_same_f32(m, st["m"], f"{what}: m")
        assert_same_f32(v, st["v"], f"{what}: v")
        assert_same_f32(np.array([vmax], np.float32), np.array([st["vmax"]], np.float32), f"{what}: vmax")
        assert tick == st["tick"], what


def _nan_cap(po, st, touched, what):
    """The NaN rule's condition on the oracle's output of the very chain the
    device is compared with: every compared array, against the elements touched
    so far."""
    share = E.nan_share(E.state_arrays(po, st), int(touched.sum()))
    assert share <= E.NAN_CAP, f"{what}: NaN share {share:.4f}"


def _clean(case, opt):
    from stellatrain_amd.engine import scatter_merge_check
    opt.check() if case["opt"] == "sgd" else opt.check_device()
    scatter_merge_check()


# -- A: optimize_raw --------------------------------------------------------
@pytest.mark.parametrize("case", E.OPT_CASES, ids=_ids)
def test_optimize_raw_edge(gpu, oracle, case):
    param0, calls, results = E.run_oracle(oracle, case)
    E.check_stats(case, E.stats(case, param0, calls, results))
    opt = _make(case)
    pg = _up(gpu, param0)
    for it, ((idx, g), (po, st)) in enumerate(zip(calls, results)):
        opt.optimize_raw(pg, "w", _up(gpu, g), _up(gpu, idx))
        _same_state(case, opt, "w", pg, po, st, f"{case['name']} call {it}")
    _clean(case, opt)


# -- B: merge_optimize at world 1 -------------------------------------------
def _w1_stream(mode, idx, g, it=0):
    """(stream idx, stream val, wire flag) of a call's pairs."""
    if mode in ("wire2", "wire3"):
        g = E.thin_for_fp16(g, it)
    if mode == "elect":  # a third of the indices once more in front: the later pair wins
        d = idx.size // 3
        return np.concatenate([idx[:d], idx]), np.concatenate([g[::-1][:d], g]), 0
    return idx, g, {"copy": 0, "wire1": 1, "wire2": 2, "wire3": 3}[mode]


def _merged_in_order(gi, gv, ei, ev, what):
    """The device's merged stream holds the oracle's pairs; returns the oracle's
    values in the emitted order (amsgrad's running maximum follows it)."""
    o = np.argsort(gi, kind="stable")
    assert np.array_equal(gi[o], ei), f"{what}: merged indices"
    assert_same_f32(gv[o], ev, f"{what}: merged values")
    out = np.empty_like(ev)
    out[o] = ev
    return out


@pytest.mark.parametrize("mode", ["copy", "elect", "wire1", "wire2", "wire3"])
@pytest.mark.parametrize("case", HALF + E.AMS_CASES[:2], ids=_ids)
def test_merge_optimize_world1_edge(gpu, oracle, case, mode):
    n = E.N16 if mode in ("wire1", "wire3") else E.N
    param0, calls = E.optim_run(case, n)
    opt, h = _make(case), E.oracle_new(oracle, case)
    po, pg = param0.copy(), _up(gpu, param0)
    touched = np.zeros(n, bool)
    for it, (idx, g) in enumerate(calls):
        what = f"{case['name']} {mode} call {it}"
        si, sv, flag = _w1_stream(mode, idx, g, it)
        per_rank = si.size
        wi, wv = oracle.wire_encode(si, sv, flag)
        ei, ev = W.expected(oracle, [(wi, wv, flag)], per_rank, n)[2:4]
        if flag:
            oi, ov, cnt = opt.merge_optimize_wire(pg, "w", [(_up(gpu, wi), _up(gpu, wv), flag)], per_rank)
        else:
            oi, ov, cnt = opt.merge_optimize(pg, "w", _up(gpu, si), _up(gpu, sv), per_rank, 1)
        m = int(cnt.cpu().numpy().view(np.uint32)[0])
        assert m == ei.size, what
        gi = oi[:m].cpu().numpy().view(np.uint32)
        vals = _merged_in_order(gi, ov[:m].cpu().numpy(), ei, ev, what)
        E.oracle_step(oracle, case, h, "w", po, vals, gi)
        st = E.oracle_state(oracle, case, h, "w", n)
        _same_state(case, opt, "w", pg, po, st, what)
        touched[ei] = True
        _nan_cap(po, st, touched, what)
    _clean(case, opt)
    E.oracle_free(oracle, case, h)


# -- C: scatter_merge / scatter_merge_wire ------------------------------------
class _Scratch:
    def __init__(self, gpu, n):
        import torch
        self.dense = torch.zeros(n, dtype=torch.float32, device=gpu)
        self.mark = torch.zeros(n, dtype=torch.uint8, device=gpu)

    def is_zero(self):
        import torch
        return not bool(self.dense.view(torch.int32).any()) and not bool(self.mark.any())


@pytest.fixture(scope="module")
def scratch(gpu):
    return _Scratch(gpu, E.MERGE_N)


def _merge_streams(oracle, case, flag, thin=()):
    """(idx, val, plants, wire streams, merged idx, merged val) of a merge case;
    `thin`: thinnings applied to every rank's values first."""
    idx, val, plants = E.merge_case(case)
    pr = E.MERGE_PER_RANK
    if flag & 2:  # binary16 turns half of a wide-exponent stream into inf: a few per rank stay
        thin = tuple(thin) + (E.thin_for_fp16,)
    for f in thin:
        val = np.concatenate([f(val[r * pr:(r + 1) * pr], r) for r in range(case["world"])])
    streams = [oracle.wire_encode(idx[r * pr:(r + 1) * pr], val[r * pr:(r + 1) * pr], flag) + (flag,)
               for r in range(case["world"])]
    ei, ev = W.expected(oracle, streams, pr, E.MERGE_N)[2:4]
    return idx, val, plants, streams, ei, ev


def _scatter(gpu, idx, val, streams, flag, world, scratch):
    from stellatrain_amd.engine import scatter_merge, scatter_merge_wire
    pr = E.MERGE_PER_RANK
    if flag:
        dev = [(_up(gpu, wi), _up(gpu, wv), f) for wi, wv, f in streams]
        oi, ov, cnt = scatter_merge_wire(dev, pr, E.MERGE_N, dense=scratch.dense, mark=scratch.mark)
    else:
        oi, ov, cnt = scatter_merge(_up(gpu, idx), _up(gpu, val), pr, world, E.MERGE_N, dense=scratch.dense,
                                    mark=scratch.mark)
    m = int(cnt.cpu().numpy().view(np.uint32)[0])
    return oi[:m].cpu().numpy().view(np.uint32), ov[:m].cpu().numpy()


TAME = dict(name="merge_tame", world=3, kind="tame")


@pytest.mark.parametrize("flag", [0, 2])
@pytest.mark.parametrize("case", E.MERGE_CASES, ids=_ids)
def test_scatter_merge_edge(gpu, oracle, scratch, case, flag):
    from stellatrain_amd.engine import scatter_merge_check
    idx, val, plants, streams, ei, ev = _merge_streams(oracle, case, flag)
    assert np.isnan(ev).sum() <= max(1, int(E.NAN_CAP * ev.size))
    if flag == 0:
        E.merge_check_stats(case, plants, ei, ev)
    gi, gv = _scatter(gpu, idx, val, streams, flag, case["world"], scratch)
    assert np.array_equal(gi, ei), "the merged stream is index-ascending, each index once"
    assert_same_f32(gv, ev, f"{case['name']} flag {flag}")
    assert scratch.is_zero(), "a NaN or inf left in dense would poison the next bucket"
    # a tame bucket on the same scratch right after
    tidx, tval, _ = E.merge_case(dict(TAME, world=case["world"], kind=None), plant=False)
    ti, tv = oracle.merge_decompress(tidx, tval, E.MERGE_PER_RANK, case["world"], E.MERGE_N)
    assert np.isfinite(tv).all()
    gi, gv = _scatter(gpu, tidx, tval, None, 0, case["world"], scratch)
    assert np.array_equal(gi, ti)
    assert_same_f32(gv, tv, f"tame bucket after {case['name']}")
    assert scratch.is_zero()
    scatter_merge_check()


# -- D: merge_optimize at world 3 ---------------------------------------------
def _w3_case(kind):
    return dict(name=f"merge_{kind or 'planted'}_w3", world=3, kind=kind)


def _thin_for(case):
    """The thinning a handle's configuration needs on every rank's values
    (eps = 0: two values a rank whose square underflows, of 800 merged ones)."""
    if case["opt"] == "adam" and case["cfg"] == "d":
        return lambda g, it: E.thin_for_eps0(g, it, 2)
    return None


def _w3_param(seed, first, later, plant=True):
    """A parameter of MERGE_N elements with +-inf, -0.0, subnormals and +-FLT_MAX
    at indices of the merged streams: `first` is touched by the first calls,
    `later` by the later ones (one plant sits on an index only they touch)."""
    p = E.synth(E.MERGE_N, E.seed_for(E.BUCKET + 4, seed)) * np.float32(1000.0)
    if not plant:
        return p
    only_later = np.setdiff1d(later, first)
    both = np.intersect1d(first, later)
    k = first.size
    p[first[3]] = np.inf
    p[both[5]] = -np.inf
    p[first[10]] = np.float32(-0.0)
    p[first[k - 3]] = np.float32(1e-40)
    p[only_later[2]] = np.float32(-3e-41)
    p[first[k // 3]] = E.FLT_MAX
    p[both[50]] = -E.FLT_MAX
    return np.ascontiguousarray(p, np.float32)


# SGD (b), (e); Adam (a), (c): calls 0-1 the planted sums, calls 2-3 a gradient kind
W3_OPT = [("sgd_b_huge", "huge"), ("sgd_e_negzero", "denorm_half"), ("adam_a_inf", "negzero"),
          ("adam_c_inf", "denorm_all")]


@pytest.mark.parametrize("flag", [0, 2])
@pytest.mark.parametrize("name,kind", W3_OPT, ids=[f"{n[:5].rstrip('_')}_{k}" for n, k in W3_OPT])
def test_merge_optimize_world3_edge(gpu, oracle, scratch, name, kind, flag):
    case = E.case_by_name(name)
    n, pr = E.MERGE_N, E.MERGE_PER_RANK
    w3 = [_w3_case(None)] * 2 + [_w3_case(kind)] * 2
    chains = [_merge_streams(oracle, mc, flag, (_two_big,) if mc["kind"] else ()) for mc in w3]
    param0 = _w3_param(W3_OPT.index((name, kind)), chains[0][4], chains[2][4])
    opt, h = _make(case), E.oracle_new(oracle, case)
    po, pg = param0.copy(), _up(gpu, param0)
    touched = np.zeros(n, bool)
    for it, (idx, val, plants, streams, ei, ev) in enumerate(chains):
        what = f"{case['opt']}_{case['cfg']} world 3 flag {flag} call {it}"
        if flag:
            dev = [(_up(gpu, wi), _up(gpu, wv), f) for wi, wv, f in streams]
            oi, ov, cnt = opt.merge_optimize_wire(pg, "w", dev, pr, dense=scratch.dense, mark=scratch.mark)
        else:
            oi, ov, cnt = opt.merge_optimize(pg, "w", _up(gpu, idx), _up(gpu, val), pr, 3, dense=scratch.dense,
                                             mark=scratch.mark)
        m = int(cnt.cpu().numpy().view(np.uint32)[0])
        assert m == ei.size, what
        gi = oi[:m].cpu().numpy().view(np.uint32)
        assert np.array_equal(gi, ei), what  # index-ascending: amsgrad's order is the oracle's
        assert_same_f32(ov[:m].cpu().numpy(), ev, f"{what}: merged values")
        E.oracle_step(oracle, case, h, "w", po, ev, ei)
        st = E.oracle_state(oracle, case, h, "w", n)
        _same_state(case, opt, "w", pg, po, st, what)
        assert scratch.is_zero(), what
        touched[ei] = True
        _nan_cap(po, st, touched, what)
    _clean(case, opt)
    E.oracle_free(oracle, case, h)


# -- E: merge_optimize_batch ----------------------------------------------------
def _empty_streams(gpu, world):
    return [(_up(gpu, np.zeros(1, np.uint32)), _up(gpu, np.zeros(1, np.float32)), 0)] * world


W3_BATCH_KINDS = [None, "inf", "denorm_half", "huge", "denorm_all", "wide_exp", "nan_steady"]  # calls 2-3: negzero


def _two_big(g, it):
    """Five infinities, or 64 values of +-3e38, a rank on three ranks pass 1 % of
    the 800 to 1,400 touched elements: two a rank stay."""
    return E.thin_where(g, np.abs(g) >= np.float32(3e38), it, 2)


def _batch_tasks(oracle, world, case):
    """[(name, n, param0, [per call: (streams, per_rank, merged idx, merged val)])]
    for a handle of `case`'s configuration."""
    tasks = []
    if world == 1:
        for kind in E.GRAD_KINDS:
            param0, calls = E.optim_run(dict(case, name=f"batch_{kind}", kind=kind, plant=None))
            per_call = []
            for idx, g in calls:
                ei, ev = oracle.merge_decompress(idx, g, idx.size, 1, E.N)
                per_call.append(([(idx, g, 0)], idx.size, ei, ev))
            tasks.append((f"t_{kind}", E.N, param0, per_call))
    else:
        for j, kind in enumerate(W3_BATCH_KINDS):
            thin = [f for f in (_thin_for(case), _two_big if kind in ("inf", "huge") else None) if f]
            chains = [_merge_streams(oracle, dict(name="b", world=world, kind=k), 0, thin) for k in (kind, "negzero")]
            per_call = [(c[3], E.MERGE_PER_RANK, c[4], c[5]) for c in chains for _ in range(2)]
            # eps = 0 already turns the planted sums into x / 0 and 0 / 0: its parameter stays tame
            param0 = _w3_param(10 + j, chains[0][4], chains[1][4], plant=_thin_for(case) is None)
            tasks.append((f"t_{kind or 'planted'}", E.MERGE_N, param0, per_call))
    return tasks


# every configuration of both optimizers
BATCH_OPT = [E.case_by_name(n) for n in ("sgd_a_inf", "sgd_b_huge", "sgd_c_inf", "sgd_d_huge", "sgd_e_negzero",
                                         "adam_a_inf", "adam_b_huge", "adam_c_inf", "adam_d_denorm_all",
                                         "adam_e_negzero")]


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("case", BATCH_OPT, ids=lambda c: f"{c['opt']}_{c['cfg']}")
def test_merge_optimize_batch_edge(gpu, oracle, scratch, case, world):
    """One batched call per iteration on handle `a` (an empty task in the middle
    takes the per-tensor route; so does every task under amsgrad), the
    per-tensor twin on `b`, the oracle chain per task."""
    tasks = _batch_tasks(oracle, world, case)
    a, b, h = _make(case), _make(case), E.oracle_new(oracle, case)
    pa = {nm: _up(gpu, p0) for nm, n, p0, _ in tasks}
    pb = {nm: _up(gpu, p0) for nm, n, p0, _ in tasks}
    po = {nm: p0.copy() for nm, n, p0, _ in tasks}
    pa["empty"], pb["empty"], po["empty"] = _up(gpu, tasks[0][2]), _up(gpu, tasks[0][2]), tasks[0][2].copy()
    touched = {nm: np.zeros(p.size, bool) for nm, p in po.items()}
    extra = (scratch.dense, scratch.mark) if world > 1 else ()
    kw = dict(dense=scratch.dense, mark=scratch.mark) if world > 1 else {}
    for it in range(E.CALLS):
        items, seq = [], []
        for j, (nm, n, p0, per_call) in enumerate(tasks):
            if j == 2:
                dev = _empty_streams(gpu, world)
                items.append((pa["empty"], "empty", dev, 0) + extra)
                seq.append(("empty", dev, 0, np.zeros(0, np.uint32), np.zeros(0, np.float32)))
            streams, pr, ei, ev = per_call[it]
            dev = [(_up(gpu, wi), _up(gpu, wv), f) for wi, wv, f in streams]
            items.append((pa[nm], nm, dev, pr) + extra)
            seq.append((nm, dev, pr, ei, ev))
        got = a.merge_optimize_batch(items)
        assert len(got) == len(seq)
        for (nm, dev, pr, ei, ev), (oi, ov, cnt) in zip(seq, got):
            what = f"{case['opt']}_{case['cfg']} world {world} call {it} task {nm}"
            m = int(cnt.cpu().numpy().view(np.uint32)[0])
            assert m == ei.size, what
            gi = oi[:m].cpu().numpy().view(np.uint32)
            vals = _merged_in_order(gi, ov[:m].cpu().numpy(), ei, ev, what)
            ti, tv, tc = b.merge_optimize_wire(pb[nm], nm, dev, pr, **kw)
            assert int(tc.cpu().numpy().view(np.uint32)[0]) == m, what
            assert np.array_equal(ti[:m].cpu().numpy().view(np.uint32), gi), f"{what}: twin's emitted order"
            assert_same_f32(tv[:m].cpu().numpy(), ov[:m].cpu().numpy(), f"{what}: twin's merged values")
            E.oracle_step(oracle, case, h, nm, po[nm], vals, gi)
            touched[nm][ei] = True
        for nm in po:
            n = po[nm].size
            st = E.oracle_state(oracle, case, h, nm, n)
            _nan_cap(po[nm], st, touched[nm], f"call {it} {nm}")
            _same_state(case, a, nm, pa[nm], po[nm], st, f"batch call {it} {nm}")
            _same_state(case, b, nm, pb[nm], po[nm], st, f"twin call {it} {nm}")
        if world > 1:
            assert scratch.is_zero()
    _clean(case, a)
    _clean(case, b)
    E.oracle_free(oracle, case, h)
