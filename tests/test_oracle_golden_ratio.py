"""Pin the CPU oracle to the reference when a key's k changes between calls
(tests/golden/make_golden_ratio.py, cases from tests/ratio_cases.py), and
assert that the table reaches what it is for.

Every call first checks the sha256 of its regenerated input against the
manifest: a drift of the generator fails as a fixture problem, not as a codec
failure.  The GPU parity tests (test_gpu_ratio.py) then compare the HIP path
with this pinned oracle over the same table.

test_table_* use the oracle alone.  A failure there means the table no longer
drives the kernels where it should (the fixture is inadequate), not that a
kernel is wrong.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import ratio_cases as rc
from stellatrain_amd.synth import D3

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest_ratio.json")))
ARR = np.load(os.path.join(GOLD, "golden_ratio.npz"))


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


def _input(case, it):
    src = rc.ratio_input(case["n"], it, case["dist"], case["param"], case["seed_bucket"])
    assert rc.sha(src.view(np.uint32)) == case["inputs"][it], \
        "fixture problem: ratio_cases.py no longer generates the golden input"
    return src


def _codec_case(oracle, case, codec):
    h = oracle.tv16_new() if codec == "tv16" else oracle.tv_new()
    name, n = case["name"], case["n"]
    assert len(case["ratios"]) == len(case["ks"]) == len(case["hashes"])
    for it, (r, k) in enumerate(zip(case["ratios"], case["ks"])):
        assert k == rc.merge_k(n, r), "fixture problem: merge_numel no longer gives the golden k"
        src = _input(case, it)
        if codec == "tv16":
            cnt, idx, val = oracle.tv16_compress(h, case["key"], src, k)
            t, inc = oracle.tv16_state(h, case["key"])
            assert f32bits(inc) == ARR[f"{name}/inc_bits"][it], it
        else:
            cnt, idx, val = oracle.tv_compress(h, 1, src, k)
            t = oracle.tv_state(h, 1)
        assert cnt == ARR[f"{name}/counts"][it], it
        assert f32bits(t) == ARR[f"{name}/t_bits"][it], it
        if case["stored"][it]:
            np.testing.assert_array_equal(idx[:cnt], ARR[f"{name}/it{it}/idx"])
            np.testing.assert_array_equal(val[:cnt].view(np.uint32), ARR[f"{name}/it{it}/val"])
        assert rc.sha(idx[:cnt]) + ":" + rc.sha(val[:cnt].view(np.uint32)) == case["hashes"][it], it
    (oracle.tv16_free if codec == "tv16" else oracle.tv_free)(h)


@pytest.mark.parametrize("case", MANIFEST["tv16"], ids=lambda c: c["name"])
def test_tv16_oracle_matches_reference_ratio(oracle, case):
    _codec_case(oracle, case, "tv16")


@pytest.mark.parametrize("case", MANIFEST["tv"], ids=lambda c: c["name"])
def test_tv_oracle_matches_reference_ratio(oracle, case):
    _codec_case(oracle, case, "tv")


def test_manifest_is_the_table():
    """The fixtures cover the table of ratio_cases.py, no more and no less."""
    want = {f"tv16_one_{n}": rc.RATIOS for n in rc.SIZES}
    want.update({f"tv16_batch_{n}_key{j}": [rc.batch_ratio(j, s) for s in range(rc.BATCH_STEPS)]
                 for n in rc.BATCH_SIZES for j in range(rc.BATCH_KEYS)})
    want.update({f"tv16_d3_{n}": rc.D3_RATIOS for n in rc.D3_SIZES})
    assert {c["name"]: c["ratios"] for c in MANIFEST["tv16"]} == want
    want = {f"tv_{s}_{n}": r for s, r in rc.TV_SCHEDULES.items() for n in rc.TV_SIZES}
    assert {c["name"]: c["ratios"] for c in MANIFEST["tv"]} == want
    for c in MANIFEST["tv16"] + MANIFEST["tv"]:  # whole streams where the generator promises them
        for it, cnt in enumerate(ARR[f"{c['name']}/counts"]):
            one_key = "_batch_" not in c["name"]
            assert c["stored"][it] == (one_key and c["n"] <= rc.FULL_STREAM_MAX_N and cnt <= rc.FULL_STREAM_MAX_COUNT)


@pytest.fixture(scope="module")
def probes(oracle):
    """Per one-key thresholdv16 case: one dict per call after the first, with
    the regime and fill_probe's (q, head, M, window) against the threshold the
    call met."""
    out = {}
    for n, dist, param, bucket, ratios, tag in \
            [(n, 0, 0, rc.SEED_BUCKET, rc.RATIOS, "one") for n in rc.SIZES] + \
            [(n, D3, rc.D3_ZP, rc.D3_SEED_BUCKET, rc.D3_RATIOS, "d3") for n in rc.D3_SIZES]:
        h = oracle.tv16_new()
        calls = []
        for it, r, k in rc.schedule(n, ratios=ratios):
            src = rc.ratio_input(n, it, dist, param, bucket)
            before = oracle.tv16_state(h, "p")
            cnt, idx, _ = oracle.tv16_compress(h, "p", src, k)
            if before is None:
                continue
            q, head, m, window = rc.fill_probe(oracle, src, k, before[0], cnt)
            call = {"it": it, "k": k, "count": cnt, "q": q, "head": head, "M": m, "window": window,
                    "regime": "B" if oracle.tv16_state(h, "p")[0] < before[0] else "A"}
            if tag == "d3" and call["regime"] == "B":
                sums = oracle.tv16_block_sums(src)
                popped = np.unique(idx[head:cnt].astype(np.int64) // 16)
                popped = popped[popped < sums.size]
                last = int(idx[cnt - 1]) // 16
                call["last_sum"] = float(sums[last]) if last < sums.size else None
                call["zero_left"] = int(np.count_nonzero(sums == 0)) - int(np.count_nonzero(sums[popped] == 0))
            calls.append(call)
        oracle.tv16_free(h)
        out[(tag, n)] = calls
    return out


def _b(calls):
    return [c for c in calls if c["regime"] == "B"]


def test_table_window_hits_and_misses(probes):
    """(a) every size from 65541 up has regime-B calls the window holds
    (M + 2 <= window) and calls past it."""
    for n in rc.SIZES[1:]:
        b = _b(probes[("one", n)])
        assert any(c["M"] + 2 <= c["window"] for c in b), n
        assert any(c["M"] + 2 > c["window"] for c in b), n


def test_table_fill_sizes(probes):
    """(b) more than three tiles of 4,096 lines at the two large sizes;
    (c) a fill between the small tile and the one-bucket leader's 11,264."""
    for n in ((1 << 18) + 5, (1 << 20) + 13):
        assert any(c["M"] > 12288 for c in _b(probes[("one", n)])), n
    assert any(4096 < c["M"] <= 11264 for c in _b(probes[("one", (1 << 20) + 13)]))


def test_table_stale_threshold_overfills(probes):
    """(d) a call at every size meets a threshold that lets through at least
    eight times the whole lines the output holds, with a partial last line."""
    for n in rc.SIZES:
        assert any(c["q"] >= 8 * (c["k"] // 16) and c["k"] % 16 for c in probes[("one", n)]), n


def test_table_both_regimes(probes):
    """(e) both regimes at every size."""
    for n in rc.SIZES:
        assert {c["regime"] for c in probes[("one", n)]} == {"A", "B"}, n


def test_table_d3_zero_tie_at_the_cut(probes):
    """(f) a regime-B call of each D3 size pops a zero line last and leaves
    zero lines unpopped: the tie is at the cut, inside a fill of thousands."""
    for n in rc.D3_SIZES:
        hit = [c for c in _b(probes[("d3", n)]) if c["last_sum"] == 0.0 and c["zero_left"] > 0]
        assert hit and max(c["M"] for c in hit) > 3000, n


def test_table_tv_found_against_k(oracle):
    """(g) threshold-v: calls that find more than 50 k elements and calls that
    find fewer than k, at both sizes."""
    for n in rc.TV_SIZES:
        over = under = 0
        for sched, ratios in rc.TV_SCHEDULES.items():
            h = oracle.tv_new()
            for it, r, k in rc.schedule(n, ratios=ratios):
                src = rc.ratio_input(n, it, bucket=rc.TV_SEED_BUCKET[sched])
                t = oracle.tv_state(h, 1)
                oracle.tv_compress(h, 1, src, k)
                if t is None:
                    continue
                found = int(np.count_nonzero(np.abs(src) >= np.float32(t)))
                over += found > 50 * k
                under += 0 < found < k
            oracle.tv_free(h)
        assert over and under, (n, over, under)
