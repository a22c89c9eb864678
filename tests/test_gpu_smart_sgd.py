"""GPU parity of smart-momentum sparse SGD (optim/sgd.cpp:54, 225-232, 258-259;
``configure("smart_momentum", true)``, sgd.cpp:291-292).

The goldens (tests/golden/golden_smart_sgd.npz) come from the reference's own
sgd.cpp compiled in place with the option on; every comparison is bit-exact
(fp32 bit patterns, uint32 last-touched iterations, the iteration count).
"""
from __future__ import annotations

import numpy as np
import pytest

import smart_sgd_golden as G
from stellatrain_amd.synth import seed_for, synth

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(a, gpu):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(gpu)


def _make(case):
    from stellatrain_amd import SparseSGD
    return SparseSGD(**G.opts(case))


def _check_final(case, sgd, params_gpu):
    for j, (nm, n) in enumerate(zip(case["names"], case["lens"])):
        param, mom, last = G.final_state(case, j)
        assert np.array_equal(_bits(params_gpu[j].cpu().numpy()), _bits(param)), nm
        assert np.array_equal(_bits(sgd.momentum_buffer(nm, n)), _bits(mom)), nm
        assert np.array_equal(sgd.last_buffer(nm, n), last), nm
    assert sgd.iteration == case["iter"]
    sgd.check()


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c["name"])
def test_smart_sgd_matches_reference_goldens(gpu, case):
    """optimize_raw against every golden case: the parameter after each call,
    then the buffer, the last-touched array and the iteration count.  Case f
    runs its first two calls with the option off and enables it mid-run."""
    sgd = _make(case)
    exp = G.initial_params(case)
    pg = [_dev(p, gpu) for p in exp]
    on = False
    for s, (nm, smart, idx, grad, after) in enumerate(G.calls(case)):
        if smart != on:
            sgd.configure("smart_momentum", smart)
            on = smart
        sgd.optimize_raw(pg[nm], case["names"][nm], _dev(grad, gpu), _dev(idx, gpu))
        exp[nm][idx] = after
        assert np.array_equal(_bits(pg[nm].cpu().numpy()), _bits(exp[nm])), f"param differs after call {s}"
    _check_final(case, sgd, pg)


def _stream(mode, idx, grad, rng):
    """The golden's pairs as MERGE rank streams: (idx, val, per_rank, world)."""
    k = idx.size
    if mode == "copy" or k == 0:  # duplicate-free: the emission copies the stream
        return idx, grad, k, 2 if mode == "world2" else 1
    if mode == "elect":  # earlier occurrences of a third of the indices lose to the golden's pairs
        d = k // 3
        return (np.concatenate([idx[:d], idx]), np.concatenate([rng.standard_normal(d).astype(np.float32), grad]),
                k + d, 1)
    # world 2: disjoint halves; merged = (2 g + 0) / 2 == g exactly
    assert k % 2 == 0
    return idx, grad * np.float32(2.0), k // 2, 2


@pytest.mark.parametrize("mode", ["copy", "elect", "world2"])
@pytest.mark.parametrize("name", ["a_overlap", "c_two_names"])
def test_smart_sgd_fused_merge_optimize(gpu, name, mode):
    """Cases a and c through merge_optimize: world 1 on the duplicate-free copy
    path and on the election path (the step runs inside the emission), and
    world 2 (the merge, then the step over its output).  Same goldens."""
    case = G.case_by_name(name)
    sgd = _make(case)
    sgd.configure("smart_momentum", True)
    exp = G.initial_params(case)
    pg = [_dev(p, gpu) for p in exp]
    rng = np.random.default_rng(5)
    for s, (nm, smart, idx, grad, after) in enumerate(G.calls(case)):
        si, sv, per_rank, world = _stream(mode, idx, grad, rng)
        oi, ov, cnt = sgd.merge_optimize(pg[nm], case["names"][nm], _dev(si, gpu), _dev(sv, gpu), per_rank, world)
        m = int(cnt.item())
        assert m == idx.size, s
        o = np.argsort(idx, kind="stable")
        gi, gv = oi[:m].cpu().numpy().view(np.uint32), ov[:m].cpu().numpy()
        go = np.argsort(gi, kind="stable")
        assert np.array_equal(gi[go], idx[o]) and np.array_equal(_bits(gv[go]), _bits(grad[o])), s
        exp[nm][idx] = after
        assert np.array_equal(_bits(pg[nm].cpu().numpy()), _bits(exp[nm])), f"param differs after call {s}"
    _check_final(case, sgd, pg)
    from stellatrain_amd.engine import scatter_merge_check
    scatter_merge_check()


def test_smart_sgd_same_indices_equals_plain(gpu, oracle):
    """The same index set every step: every gap is 1 and pow(m, 1) == m, so the
    option changes nothing -- bit-equal to the CPU oracle's plain SGD."""
    from stellatrain_amd import SparseSGD
    opt = dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=1e-4, nesterov=True)
    n, k = 4103, 300  # two workgroups, a ragged second one
    sgd = SparseSGD(smart_momentum=True, **opt)
    ho = oracle.sgd_new(**opt)
    po = synth(n, seed_for(38, 1)) * np.float32(1000)
    pg = _dev(po, gpu)
    gidx = np.random.default_rng(8).choice(n, k, replace=False).astype(np.uint32)
    for step in range(4):
        g = synth(k, seed_for(38, 10 + step)) * np.float32(100)
        oracle.sgd_apply(ho, "w", po, g, gidx)
        sgd.optimize_raw(pg, "w", _dev(g, gpu), _dev(gidx, gpu))
        assert np.array_equal(_bits(pg.cpu().numpy()), _bits(po)), step
    assert np.array_equal(_bits(sgd.momentum_buffer("w", n)), _bits(oracle.sgd_momentum(ho, "w", n)))
    last = np.zeros(n, np.uint32)
    last[gidx] = 3
    assert np.array_equal(sgd.last_buffer("w", n), last)
    sgd.check()
    oracle.sgd_free(ho)


def test_smart_sgd_option_off_is_plain(gpu):
    """A handle told smart_momentum=False equals one that never heard of the
    option (SGD_CASES[1]'s options of test_gpu_apply.py), and keeps no
    last-touched array."""
    from stellatrain_amd import SparseSGD
    opt = dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=1e-4, nesterov=True)
    n, k = 4103, 300
    a, b = SparseSGD(smart_momentum=False, **opt), SparseSGD(**opt)
    a.configure("smart_momentum", False)
    p0 = synth(n, seed_for(38, 2)) * np.float32(1000)
    pa, pb = _dev(p0, gpu), _dev(p0, gpu)
    perm = np.random.default_rng(9).permutation(n).astype(np.uint32)
    for step, lo in enumerate([0, 150, 0, 600]):  # overlapping sets, gaps of 1, 2 and none
        gidx, g = _dev(perm[lo:lo + k], gpu), _dev(synth(k, seed_for(38, 20 + step)) * np.float32(100), gpu)
        a.optimize_raw(pa, "w", g, gidx)
        b.optimize_raw(pb, "w", g, gidx)
        assert np.array_equal(_bits(pa.cpu().numpy()), _bits(pb.cpu().numpy())), step
    assert np.array_equal(_bits(a.momentum_buffer("w", n)), _bits(b.momentum_buffer("w", n)))
    assert a.last_buffer("w", n) is None and a.iteration == b.iteration == 4
    a.check()


def test_smart_sgd_repeated_index_is_skipped_and_reported(gpu):
    """An index twice in one call at iteration 1: the reference asserts on the
    second occurrence's factor pow(m, 0) == 1.  Here one occurrence is applied,
    the other skipped, check() reports STG_ERR_DEVICE, and every other element
    equals a run of the same call without the repeat."""
    from stellatrain_amd import CodecError, SparseSGD
    opt = dict(lr=0.1, momentum=0.9, nesterov=True)
    n, k = 4103, 300
    perm = np.random.default_rng(10).permutation(n).astype(np.uint32)
    g0, g1 = (synth(k, seed_for(38, 30 + s)) * np.float32(100) for s in range(2))
    idx0, idx1 = perm[:k], perm[100:100 + k].copy()
    idx1[250] = idx1[7]  # the pair at 250 repeats the index of the pair at 7
    dup = int(idx1[7])
    p0 = synth(n, seed_for(38, 3)) * np.float32(1000)

    def run(keep):
        sgd = SparseSGD(smart_momentum=True, **opt)
        pg = _dev(p0, gpu)
        sgd.optimize_raw(pg, "w", _dev(g0, gpu), _dev(idx0, gpu))
        sgd.optimize_raw(pg, "w", _dev(g1[keep], gpu), _dev(idx1[keep], gpu))
        return sgd, pg.cpu().numpy(), sgd.momentum_buffer("w", n), sgd.last_buffer("w", n)

    every = np.ones(k, bool)
    sgd, p, mom, last = run(every)
    with pytest.raises(CodecError) as e:
        sgd.check()
    assert e.value.code == -5
    refs = []
    for drop in (250, 7):  # the same call with one of the two occurrences only
        keep = every.copy()
        keep[drop] = False
        rs, rp, rmom, rlast = run(keep)
        rs.check()
        refs.append((rp, rmom))
        others = np.arange(n) != dup
        assert np.array_equal(_bits(p)[others], _bits(rp)[others])
        assert np.array_equal(_bits(mom)[others], _bits(rmom)[others])
        assert np.array_equal(last, rlast) and last[dup] == 1
    assert any(_bits(p)[dup] == _bits(rp)[dup] and _bits(mom)[dup] == _bits(rmom)[dup] for rp, rmom in refs)
