"""Pin the CPU oracle's receiving side to the reference where values are not
tame (tests/golden/make_golden_optim_edge.py, inputs from tests/optim_edge.py):
sparse SGD, smart-momentum SGD, Adam, amsgrad and the MERGE decompress on
infinities, overflowing sums, denormals, -0.0, the whole exponent range and
NaNs; and the oracle's smart momentum to every case of golden_smart_sgd.npz.

Every case first checks the sha256 of its regenerated inputs (a generator drift
is a fixture problem), then the NaN rule of parity.assert_same_f32: hashes are
taken after mapping every NaN to 0x7fc00000, and NaN positions stay within 1 %
of the touched elements.

``test_wrong_kernel_*`` prove the inputs discriminate: numpy restatements of
plausible wrong kernels, each built on the pinned state so that only the named
deviation differs; the correct restatement reproduces the golden first.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import optim_edge as E
import smart_sgd_golden as G
from parity import assert_same_f32, bits, canon_nan

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest_optim_edge.json")))
ARR = np.load(os.path.join(GOLD, "golden_optim_edge.npz"))
OPT = {c["name"]: c for c in MANIFEST["optim"]}
MERGE = {c["name"]: c for c in MANIFEST["merge"]}
FIXTURE = "fixture problem: optim_edge.py no longer generates the golden inputs"


def test_manifest_lists_the_cases_of_optim_edge():
    assert [c["name"] for c in MANIFEST["optim"]] == [c["name"] for c in E.OPT_CASES]
    assert [c["name"] for c in MANIFEST["merge"]] == [c["name"] for c in E.MERGE_CASES]
    for c in E.OPT_CASES:
        assert OPT[c["name"]]["options"] == E.cfg_of(c)
    assert {c["kind"] for c in E.SGD_CASES} == {c["kind"] for c in E.ADAM_CASES} == set(E.GRAD_KINDS)
    assert {c["cfg"] for c in E.SGD_CASES} == set(E.SGD_CFG) and {c["cfg"] for c in E.ADAM_CASES} == set(E.ADAM_CFG)


# -- the oracle's smart momentum on the old golden ---------------------------
@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c["name"])
def test_oracle_smart_sgd_matches_reference_goldens(oracle, case):
    h = oracle.sgd_new(**G.opts(case))
    params = G.initial_params(case)
    for s, (nm, smart, idx, grad, after) in enumerate(G.calls(case)):
        oracle.sgd_smart(h, smart)
        before = params[nm].copy()
        oracle.sgd_apply(h, case["names"][nm], params[nm], grad, idx)
        before[idx] = after
        assert np.array_equal(bits(params[nm]), bits(before)), f"param differs after call {s}"
    for j, (nm, n) in enumerate(zip(case["names"], case["lens"])):
        param, mom, last = G.final_state(case, j)
        assert np.array_equal(bits(params[j]), bits(param)), nm
        assert np.array_equal(bits(oracle.sgd_momentum(h, nm, n)), bits(mom)), nm
        assert np.array_equal(oracle.sgd_last(h, nm, n), last), nm
    assert oracle.sgd_iter(h) == case["iter"]
    oracle.sgd_free(h)


# -- SGD, smart SGD, Adam, amsgrad on edge values ----------------------------
def _check_call(name, it, rec, idx, p, st):
    if f"{name}/it{it}/param" in ARR.files:  # whole arrays first: a mismatch names its element
        assert_same_f32(p[idx], ARR[f"{name}/it{it}/param"].view(np.float32), f"{name} call {it} param")
        for f in ("mom", "m", "v"):
            if f in st:
                assert_same_f32(st[f][idx], ARR[f"{name}/it{it}/{f}"].view(np.float32), f"{name} call {it} {f}")
        if "last" in st:
            np.testing.assert_array_equal(st["last"][idx], ARR[f"{name}/it{it}/last"])
    assert E.sha(canon_nan(p)) == rec["param"], f"{name} call {it}: param"
    for f in ("mom", "m", "v"):
        assert (f in st) == (f in rec)
        if f in st:
            assert E.sha(canon_nan(st[f])) == rec[f], f"{name} call {it}: {f}"
    assert ("last" in st) == ("last" in rec)
    if "last" in st:
        assert E.sha(st["last"]) == rec["last"], f"{name} call {it}: last"
    if "vmax" in st:
        assert int(canon_nan(np.array([st["vmax"]], np.float32))[0]) == rec["vmax_bits"], f"{name} call {it}: vmax"
        assert st["tick"] == rec["tick"]
    if "iter" in st:
        assert st["iter"] == rec["iter"]


@pytest.mark.parametrize("case", E.OPT_CASES, ids=lambda c: c["name"])
def test_optimizer_oracle_matches_reference_edge(oracle, case):
    gold = OPT[case["name"]]
    param0, calls = E.optim_run(case)
    assert E.input_hashes(param0, calls) == gold["inputs"], FIXTURE
    param0, calls, results = E.run_oracle(oracle, case)
    for it, ((idx, g), (p, st)) in enumerate(zip(calls, results)):
        _check_call(case["name"], it, gold["calls"][it], idx, p, st)
    s = E.stats(case, param0, calls, results)
    E.check_stats(case, s)  # the 1 % NaN cap among them
    assert s == gold["stats"]


@pytest.mark.parametrize("case", E.MERGE_CASES, ids=lambda c: c["name"])
def test_merge_oracle_matches_torch_edge(oracle, case):
    gold = MERGE[case["name"]]
    idx, val, plants = E.merge_case(case)
    assert E.sha(idx) + ":" + E.sha(val) == gold["inputs"], FIXTURE
    oi, ov = oracle.merge_decompress(idx, val, E.MERGE_PER_RANK, case["world"], E.MERGE_N)
    if case["name"] in E.MERGE_WHOLE:
        np.testing.assert_array_equal(oi, ARR[f"{case['name']}/idx"])
        assert_same_f32(ov, ARR[f"{case['name']}/val"].view(np.float32), case["name"])
    assert oi.size == gold["union"] and int(np.isnan(ov).sum()) == gold["nans"]
    assert E.sha(oi) + ":" + E.sha(canon_nan(ov)) == gold["sha256"]
    E.merge_check_stats(case, plants, oi, ov)


def test_whole_exponent_range_reaches_every_edge_of_the_step():
    """The fixtures hold what the issue names: a subnormal vt, an infinite vt
    beside a finite parameter, vmax == inf with unmoved elements behind the
    plant, a subnormal merged value (merge_check_stats), +-inf parameters."""
    assert any(c["stats"].get("subnormal_v", 0) > 0 for c in MANIFEST["optim"])
    assert any(c["stats"].get("inf_v_finite_param", 0) > 0 for c in MANIFEST["optim"])
    s = OPT["ams_inf_mid"]["stats"]
    assert s["vmax_bits"] == 0x7F800000 and s["moved_from_plant"] == 0 and s["moved_before_plant"] > 1500
    assert max(c["stats"]["nan_share"] for c in MANIFEST["optim"]) <= E.NAN_CAP
    assert any(c["stats"]["nan_share"] > 0 for c in MANIFEST["optim"])


# -- wrong kernels ------------------------------------------------------------
def _np_merge(idx, val, per_rank, world, n, divide=True, flush=False):
    """cpu_optimize.cpp:40-72 in numpy float32; `divide=False`: * (1 / world);
    `flush`: subnormal operands and results become zero."""
    ftz = _ftz if flush else (lambda a: a)
    merged = np.zeros(n, np.float32)
    for r in range(world):
        tmp = np.zeros(n, np.float32)
        tmp[idx[r * per_rank:(r + 1) * per_rank]] = ftz(val[r * per_rank:(r + 1) * per_rank])
        with np.errstate(all="ignore"):
            merged = ftz((merged + tmp).astype(np.float32))
    w = np.float32(world)
    with np.errstate(all="ignore"):
        merged = ftz(merged / w if divide else merged * (np.float32(1) / w))
    ui = np.unique(idx)
    return ui, merged[ui]


def _merge_differs(case, **kw):
    idx, val, _ = E.merge_case(case)
    gold = MERGE[case["name"]]
    ui, uv = _np_merge(idx, val, E.MERGE_PER_RANK, case["world"], E.MERGE_N, **kw)
    return E.sha(ui) + ":" + E.sha(canon_nan(uv)) != gold["sha256"]


def test_wrong_kernel_merge_restatement_is_right_first():
    for case in E.MERGE_CASES:
        assert not _merge_differs(case), case["name"]


def test_wrong_kernel_world_reciprocal():
    """/ world as * (1 / world): exact for the powers of two, caught at every
    other world by the planted and the wide-exponent cases."""
    caught = [c["name"] for c in E.MERGE_CASES if _merge_differs(c, divide=False)]
    assert {"merge_planted_w3", "merge_planted_w5", "merge_planted_w6", "merge_planted_w7"} <= set(caught)
    assert "merge_planted_w2" not in caught and "merge_planted_w8" not in caught  # 1 / 2^k is exact


def test_wrong_kernel_merge_flushes_subnormals():
    caught = [c["name"] for c in E.MERGE_CASES if _merge_differs(c, flush=True)]
    assert {f"merge_planted_w{w}" for w in E.MERGE_WORLDS} <= set(caught)
    assert "merge_denorm_all_w6" in caught and "merge_denorm_half_w5" in caught


def _ftz(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.abs(a) < E.FLT_MIN, np.copysign(np.float32(0), a), a).astype(np.float32)


def test_wrong_kernel_optimizer_flushes_subnormals(oracle):
    """The step with its operands (parameter, gradient) and results flushed:
    differs from the golden on the denormal kinds of both optimizers."""
    caught = []
    for name in ("sgd_a_denorm_all", "sgd_e_denorm_half", "adam_a_denorm_all", "adam_e_denorm_half", "ams_subnormal",
                 "sgd_a_wide_exp", "adam_a_wide_exp"):
        case = E.case_by_name(name)
        param0, calls = E.optim_run(case)
        h = E.oracle_new(oracle, case)
        p = _ftz(param0)
        differs = False
        for it, (idx, g) in enumerate(calls):
            E.oracle_step(oracle, case, h, "w", p, _ftz(g), idx)
            p = _ftz(p)
            differs |= E.sha(canon_nan(p)) != OPT[name]["calls"][it]["param"]
            st = E.oracle_state(oracle, case, h, "w", param0.size)
            for f in ("mom", "m", "v"):
                if f in st:
                    differs |= E.sha(canon_nan(_ftz(st[f]))) != OPT[name]["calls"][it][f]
        E.oracle_free(oracle, case, h)
        if differs:
            caught.append(name)
    assert caught == ["sgd_a_denorm_all", "sgd_e_denorm_half", "adam_a_denorm_all", "adam_e_denorm_half",
                      "ams_subnormal", "sgd_a_wide_exp", "adam_a_wide_exp"]


def _ams_replay(oracle, case, mode):
    """amsgrad's parameter and vmax restated in numpy from the pinned m and v
    of each call (adam.cpp:64-72).  mode: 'right' (serial prefix maximum, NaN
    never wins, vmax carried), 'nan_wins' (np.maximum), 'whole_call' (one
    maximum over the call for every element), 'not_carried' (vmax restarts at
    0 every call).  Returns whether (param, vmax) differ from the golden."""
    cfg = {"lr": 1e-3, "b1": 0.9, "b2": 0.999, "eps": 1e-8, **E.cfg_of(case)}
    gold = OPT[case["name"]]
    param0, calls, results = E.run_oracle(oracle, case)
    x_prev, vmax = param0, np.float32(0)
    differs = False
    for it, ((idx, g), (p, st)) in enumerate(zip(calls, results)):
        tick = it + 1
        c1 = 1.0 - float(np.float32(cfg["b1"])) ** tick
        c2 = 1.0 - float(np.float32(cfg["b2"])) ** tick
        mt, vt = st["m"][idx].astype(np.float64), st["v"][idx].astype(np.float64)
        with np.errstate(all="ignore"):
            num = (mt / c1) * float(np.float32(cfg["lr"]))
            vt_hat = vt / c2
            hat32 = vt_hat.astype(np.float32)
            start = np.float32(0) if mode == "not_carried" else vmax
            if mode == "nan_wins":
                run = np.maximum.accumulate(np.concatenate([[start], hat32]))[1:]
            else:
                run = np.fmax.accumulate(np.concatenate([[start], hat32]))[1:]  # fmax: NaN never wins
            if mode == "whole_call":
                run = np.full_like(run, run[-1])
            den = (np.sqrt(run.astype(np.float32)) + np.float32(cfg["eps"])).astype(np.float32).astype(np.float64)
            x = x_prev.copy()
            x[idx] = (x_prev[idx].astype(np.float64) - num / den).astype(np.float32)
        vmax = np.float32(run[-1])
        differs |= E.sha(canon_nan(x)) != gold["calls"][it]["param"]
        differs |= int(canon_nan(np.array([vmax], np.float32))[0]) != gold["calls"][it]["vmax_bits"]
        x_prev = p  # the next call restarts from the pinned parameter: one deviation at a time
        if mode != "not_carried":
            vmax = np.float32(st["vmax"])
    return differs


AMS_NAMES = ["adam_c_inf", "adam_c_denorm_half", "adam_c_wide_exp", "ams_inf_mid", "ams_nan_ends", "ams_carry",
             "ams_subnormal"]


def test_wrong_kernel_amsgrad_maximum(oracle):
    caught = {m: [n for n in AMS_NAMES if _ams_replay(oracle, E.case_by_name(n), m)]
              for m in ("right", "nan_wins", "whole_call", "not_carried")}
    assert caught["right"] == []  # the restatement reproduces the reference on every amsgrad case
    assert "ams_nan_ends" in caught["nan_wins"]
    assert {"ams_inf_mid", "ams_nan_ends", "adam_c_denorm_half"} <= set(caught["whole_call"])
    assert {"ams_carry", "ams_inf_mid"} <= set(caught["not_carried"])


def _fmaf(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the product of two floats is exact in a
    double; the sum is rounded to odd in double (TwoSum gives the error's sign),
    which the one rounding to float then treats as the exact value."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.uint64) & np.uint64(1)) == 0)
        up = fix & ((err > 0) == (s > 0))  # away from zero: the next bit pattern
        sb = s.view(np.int64).copy()
        sb[up] += 1
        sb[fix & ~up] -= 1
        return sb.view(np.float64).astype(np.float32)


def _count_diff(a, b):
    return int((canon_nan(a) != canon_nan(b)).sum())


def test_wrong_kernel_separate_multiply_and_add(oracle):
    """Momentum and the second moment as a rounded product plus a rounded
    product instead of the FMA, from the pinned previous state.  The FMA form
    restated the same way reproduces the pinned state exactly first."""
    f = np.float32
    # SGD (a): b = b * m + g  vs  fmaf(b, m, g)
    case = E.case_by_name("sgd_a_wide_exp")
    param0, calls, results = E.run_oracle(oracle, case)
    hit = 0
    for it in range(1, E.CALLS):
        idx, g = calls[it]
        b0, b1 = results[it - 1][1]["mom"][idx], results[it][1]["mom"][idx]
        with np.errstate(all="ignore"):
            right = _fmaf(b0, f(0.9), (f(1.0) * g).astype(np.float32))
            wrong = ((b0 * f(0.9)).astype(np.float32) + (f(1.0) * g)).astype(np.float32)
        assert _count_diff(right, b1) == 0
        hit += _count_diff(wrong, b1)
    assert hit > 0
    # Adam (a): v = b2 * v + ((1 - b2) g) g  and  m = b1 * m + (1 - b1) g
    for name in ("adam_a_wide_exp", "adam_a_inf"):
        case = E.case_by_name(name)
        param0, calls, results = E.run_oracle(oracle, case)
        hit_m = hit_v = 0
        for it in range(1, E.CALLS):
            idx, g = calls[it]
            m0, v0 = results[it - 1][1]["m"][idx], results[it - 1][1]["v"][idx]
            m1, v1 = results[it][1]["m"][idx], results[it][1]["v"][idx]
            with np.errstate(all="ignore"):
                am = ((f(1) - f(0.9)) * g).astype(np.float32)
                av = (((f(1) - f(0.999)) * g).astype(np.float32) * g).astype(np.float32)
                wm = ((f(0.9) * m0).astype(np.float32) + am).astype(np.float32)
                wv = ((f(0.999) * v0).astype(np.float32) + av).astype(np.float32)
            assert _count_diff(_fmaf(f(0.9), m0, am), m1) == 0 and _count_diff(_fmaf(f(0.999), v0, av), v1) == 0, name
            hit_m += _count_diff(wm, m1)
            hit_v += _count_diff(wv, v1)
        assert hit_m > 0 and hit_v > 0, name


def test_oracle_refuses_smart_momentum_without_momentum(oracle):
    """The reference reads a null last-touched array there; the oracle reports
    an error and leaves the parameter alone."""
    h = oracle.sgd_new(lr=0.1, momentum=0.0, smart_momentum=True)
    p = np.ones(8, np.float32)
    with pytest.raises(RuntimeError, match="smart_momentum"):
        oracle.sgd_apply(h, "w", p, np.ones(2, np.float32), np.array([1, 2], np.uint32))
    assert (p == 1).all() and oracle.sgd_iter(h) == 0
    oracle.sgd_free(h)
