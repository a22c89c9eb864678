"""Pin the CPU oracle to the reference on buckets whose large values cluster
by position (tests/golden/make_golden_layered.py, inputs from
tests/layered.py): thresholdv16, threshold-v and top-k in both modes.

Every call first checks the sha256 of its regenerated input against the
manifest: a drift of the generator fails as a fixture problem, not as a codec
failure.  The GPU parity tests (test_gpu_layered.py) then compare the HIP path
with this pinned oracle on the same inputs; tests/test_layered_host.py asserts
that the inputs reach what they are for.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import layered as ly
from ratio_cases import sha

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest_layered.json")))
ARR = np.load(os.path.join(GOLD, "golden_layered.npz"))


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


def _input(case, it):
    assert case["k"] == ly.K[case["n"]] and case["seed_bucket"] == ly.seed_bucket_of(case["kind"]), \
        "fixture problem: layered.py no longer has the golden k or seed bucket"
    src = ly.layered_input(case["kind"], case["n"], case["seed_bucket"], it)
    assert sha(src.view(np.uint32)) == case["inputs"][it], \
        "fixture problem: layered.py no longer generates the golden input"
    return src


def _codec_case(oracle, case, codec):
    h = oracle.tv16_new() if codec == "tv16" else oracle.tv_new()
    name, k = case["name"], case["k"]
    assert len(case["hashes"]) == ly.CALLS
    for it in range(ly.CALLS):
        src = _input(case, it)
        if codec == "tv16":
            cnt, idx, val = oracle.tv16_compress(h, "5@weight", src, k)
            t, inc = oracle.tv16_state(h, "5@weight")
            assert f32bits(inc) == ARR[f"{name}/inc_bits"][it], it
        else:
            cnt, idx, val = oracle.tv_compress(h, 1, src, k)
            t = oracle.tv_state(h, 1)
        assert cnt == ARR[f"{name}/counts"][it], it
        assert f32bits(t) == ARR[f"{name}/t_bits"][it], it
        if case["full"]:
            np.testing.assert_array_equal(idx[:cnt], ARR[f"{name}/it{it}/idx"])
            np.testing.assert_array_equal(val[:cnt].view(np.uint32), ARR[f"{name}/it{it}/val"])
        assert sha(idx[:cnt]) + ":" + sha(val[:cnt].view(np.uint32)) == case["hashes"][it], it
    (oracle.tv16_free if codec == "tv16" else oracle.tv_free)(h)


@pytest.mark.parametrize("case", MANIFEST["tv16"], ids=lambda c: c["name"])
def test_tv16_oracle_matches_reference_layered(oracle, case):
    _codec_case(oracle, case, "tv16")


@pytest.mark.parametrize("case", MANIFEST["tv"], ids=lambda c: c["name"])
def test_tv_oracle_matches_reference_layered(oracle, case):
    _codec_case(oracle, case, "tv")


@pytest.mark.parametrize("case", MANIFEST["topk"], ids=lambda c: c["name"])
def test_topk_oracle_matches_reference_layered(oracle, case):
    """Shipped mode: the reference's stream, libstdc++ partition order
    included.  Exact mode: true indices in ascending order whose values are
    the reference's as a multiset (either sign among ties at the k-th
    magnitude), read from the input at those indices."""
    name, n, k = case["name"], case["n"], case["k"]
    for it in range(ly.TOPK_CALLS):
        src = _input(case, it)
        cnt, idx, val = oracle.topk_compress(src, k, bug_compat=True)
        assert cnt == k
        if case["full"]:
            np.testing.assert_array_equal(idx, np.arange(k))
            np.testing.assert_array_equal(val.view(np.uint32), ARR[f"{name}/it{it}/val"])
        assert sha(idx) + ":" + sha(val.view(np.uint32)) == case["hashes"][it], it
        cnt, idx, val = oracle.topk_compress(src, k, bug_compat=False)
        assert cnt == k
        assert np.all(np.diff(idx.astype(np.int64)) > 0) and idx[-1] < n, it
        np.testing.assert_array_equal(val.view(np.uint32), src[idx].view(np.uint32))
        cut = np.abs(val).min()
        assert f32bits(cut) == ARR[f"{name}/cut_bits"][it], it
        assert sha(np.sort(val[np.abs(val) > cut].view(np.uint32))) == case["above"][it], it
        assert np.count_nonzero(np.abs(val) == cut) == ARR[f"{name}/at_cut"][it], it


def test_manifest_is_the_table():
    """The fixtures cover the tables of layered.py, no more and no less, with
    whole streams where the generator promises them."""
    for codec, cases in (("tv16", ly.tv16_cases()), ("tv", ly.tv_cases()), ("topk", ly.topk_cases())):
        assert [(c["kind"], c["n"]) for c in MANIFEST[codec]] == cases
        for c in MANIFEST[codec]:
            assert c["full"] == (c["n"] <= ly.FULL_STREAM_MAX_N)
            assert (f"{c['name']}/it0/val" in ARR.files) == c["full"]
    assert os.path.getsize(os.path.join(GOLD, "golden_layered.npz")) <= \
        os.path.getsize(os.path.join(GOLD, "golden_ratio.npz"))
