"""Pin the CPU oracle to the reference on non-finite, denormal, signed-zero
and wide-exponent gradients (tests/golden/make_golden_edge.py, inputs from
tests/edge_values.py).

Every case first checks the sha256 of its regenerated input against the
manifest: a drift of the generator fails as a fixture problem, not as a codec
failure.  The GPU parity tests (test_gpu_edge_values.py, test_gpu_edge_nan.py)
then compare the HIP path with this pinned oracle.
"""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np
import pytest

from edge_values import FINITE_KINDS, KINDS, edge_input, sha_input

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest_edge.json")))
ARR = np.load(os.path.join(GOLD, "golden_edge.npz"))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


def _input(case, it):
    src = edge_input(case["kind"], case["n"], case["seed_bucket"], it)
    assert sha_input(src) == case["inputs"][it], "fixture problem: edge_values.py no longer generates the golden input"
    return src


def _codec_case(oracle, case, codec):
    h = oracle.tv16_new() if codec == "tv16" else oracle.tv_new()
    name = case["name"]
    for it in range(case["iters"]):
        src = _input(case, it)
        if codec == "tv16":
            cnt, idx, val = oracle.tv16_compress(h, case["key"], src, case["k"])
            t, inc = oracle.tv16_state(h, case["key"])
            assert f32bits(inc) == ARR[f"{name}/inc_bits"][it], it
        else:
            cnt, idx, val = oracle.tv_compress(h, 1, src, case["k"])
            t = oracle.tv_state(h, 1)
        assert cnt == ARR[f"{name}/counts"][it], it
        assert f32bits(t) == ARR[f"{name}/t_bits"][it], it
        if case["full"]:
            np.testing.assert_array_equal(idx[:cnt], ARR[f"{name}/it{it}/idx"])
            np.testing.assert_array_equal(val[:cnt].view(np.uint32), ARR[f"{name}/it{it}/val"])
        assert sha(idx[:cnt]) + ":" + sha(val[:cnt].view(np.uint32)) == case["hashes"][it], it
    (oracle.tv16_free if codec == "tv16" else oracle.tv_free)(h)


@pytest.mark.parametrize("case", MANIFEST["tv16"], ids=lambda c: c["name"])
def test_tv16_oracle_matches_reference_edge(oracle, case):
    _codec_case(oracle, case, "tv16")


@pytest.mark.parametrize("case", MANIFEST["tv"], ids=lambda c: c["name"])
def test_tv_oracle_matches_reference_edge(oracle, case):
    _codec_case(oracle, case, "tv")


@pytest.mark.parametrize("case", MANIFEST["topk"], ids=lambda c: c["name"])
def test_topk_oracle_matches_reference_edge(oracle, case):
    """bug-compat top-k, including libstdc++ nth_element partition order."""
    src = _input(case, 0)
    cnt, idx, val = oracle.topk_compress(src, case["k"], bug_compat=True)
    assert cnt == case["count"]
    np.testing.assert_array_equal(idx, ARR[f"{case['name']}/idx"])
    np.testing.assert_array_equal(val.view(np.uint32), ARR[f"{case['name']}/val"])


def test_edge_goldens_hold_what_they_are_for():
    """The fixtures reach the values each kind exists for: inf thresholds that
    stay inf, denormal thresholds below 2^18 ulps, thresholds near FLT_MAX,
    -0.0 and NaN in the streams, and both AIMD regimes for every kind whose
    threshold is finite."""
    by = {}
    for c in MANIFEST["tv16"]:
        by.setdefault(c["kind"], []).append(c)
    assert set(by) == set(KINDS)
    inf = 0x7F800000
    for c in by["inf_first"]:
        assert (ARR[f"{c['name']}/t_bits"] == inf).all() and (ARR[f"{c['name']}/inc_bits"] == inf).all()
    for c in by["denorm_all"]:
        assert (ARR[f"{c['name']}/t_bits"] < (1 << 18) * 4).all() and (ARR[f"{c['name']}/t_bits"] > 0).all()
    assert max(int(ARR[f"{c['name']}/t_bits"].max()) for c in by["wide_exp"]) > f32bits(3.2e38)
    for kind in KINDS:
        if kind == "inf_first":
            continue
        ups = downs = 0
        for c in by[kind]:
            t = ARR[f"{c['name']}/t_bits"].view(np.float32).astype(np.float64)
            fin = np.isfinite(t)
            d = np.diff(t[fin])
            ups += int((d > 0).sum())
            downs += int((d < 0).sum())
        assert ups and downs, kind
    vals = lambda names: np.concatenate([ARR[f] for f in ARR.files if f.endswith("/val") and any(s in f for s in names)])
    assert (vals(["negzero"]) == 0x80000000).any()
    nan_bits = vals(["tv16_nan_steady", "tv16_nan_tail_only"])
    assert ((nan_bits & 0x7FFFFFFF) > inf).any()
    assert ((vals(["tv16_inf_"]) & 0x7FFFFFFF) == inf).any()
    assert set(FINITE_KINDS) | {"nan_steady", "nan_tail_only"} == set(KINDS)
