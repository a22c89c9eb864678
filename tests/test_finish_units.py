"""The scalar rules the three thresholdv16 finishes share
(stellatrain_amd/csrc/tv16_finish.h) on a CPU, driven by
tests/cpp/finish_units.cpp: a plain executable built with the address and
undefined-behaviour sanitizers, which includes only that header; nothing is
preloaded.

The stage-3 rule and the close are compared with the oracle
(oracle/stg_oracle.cpp, tv16_compress): the program decides a call from the
bucket, dst_len and the threshold, and the oracle's answers for the same call
(its next threshold, its count and its index stream) must show the same
regime, the same count and the tail's stage-3 pairs at the same place.

Inputs are built from the oracle's own threshold t after a first call, out of
values whose sums are exact in any order: a line of 16 equal floats v sums to
16 v, a ragged tail of two equal floats w has the signed sum 2 w and, as a
candidate, the key 16 w.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIN = 1 << 18  # TV16_WIN


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("finish_units") / "finish_units"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tests", "cpp", "finish_units.cpp"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def test_header_units_under_sanitizers(exe):
    """Decision round trip, window_lo, the pops against a walk over ranks,
    rf_key / is_desc against a right-first pre-order of 63 and 100 nodes."""
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "finish_units: ok" in r.stdout


def bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def from_bits(u: int) -> np.float32:
    return np.uint32(u).view(np.float32)


def cases(t0: np.float32):
    """name -> (floats, dst_len).  HI qualifies (sum 16 t), LO is a candidate
    far below the window (sum t / 4), WIN a candidate 1000 ulps below t."""
    f = np.float32
    hi, lo = [t0] * 16, [f(t0 / f(64))] * 16
    s1, s2 = from_bits(bits(t0) - 1000), from_bits(bits(t0) - 2000)
    win = [f(s1 / f(16))] * 16
    big = f(2.0) ** f(np.ceil(np.log2(float(t0))))  # a power of two >= t: any count of them sums exactly
    return {
        "tl0": (hi + lo + win + hi, 40),
        "tail_fits": (hi + lo + win + [t0] * 2, 40),
        "tail_cut": (hi + lo + [big] * 5, 19),
        "cand_in_window": (hi + win + lo + lo + [f(s2 / f(16))] * 2, 38),
        "cand_below_window": (hi + win + lo + [f(t0 / f(128))] * 2, 50),
        "tail_minus_zero": (hi + win + lo + [f(-0.0)] * 3, 50),
        "tail_nan": (hi + win + lo + lo + [f(np.nan), f(1.0)], 36),
        "partial_line": (hi + hi + hi + lo + [t0] * 2, 20),
        "dst_past_bucket": (hi + lo + win + [big] * 3, 100),
        "none_qualifies": (lo + win + lo + [f(t0 / f(128))] * 2, 20),
    }


def run_regime(exe, src, dst_len, t, inc):
    text = f"{src.size} {dst_len} {bits(t):x} {bits(inc):x}\n" + " ".join(f"{int(u):x}" for u in src.view(np.uint32))
    r = subprocess.run([exe, "regime"], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for kv in r.stdout.split():
        k, v = kv.split("=")
        out[k] = int(v, 16) if k in ("tail_key", "next_t") else int(v)
    return out


def test_stage3_and_close_against_the_oracle(exe, oracle):
    rng = np.random.default_rng(5)
    first = rng.standard_normal(16 * 8).astype(np.float32)
    hit = set()
    for name in cases(np.float32(1.0)):
        h = oracle.tv16_new()
        oracle.tv16_compress(h, "p", first, 32)
        t0, inc = (np.float32(x) for x in oracle.tv16_state(h, "p"))
        assert np.isfinite(t0) and t0 > 0 and bits(t0) > WIN + 4000
        floats, dst_len = cases(t0)[name]
        src = np.array(floats, np.float32)
        n, nb, tl = src.size, src.size // 16, src.size % 16
        cnt_o, idx, _ = oracle.tv16_compress(h, "p", src, dst_len)
        t1 = np.float32(oracle.tv16_state(h, "p")[0])
        oracle.tv16_free(h)
        idx = idx[:cnt_o]

        # ---- what the oracle shows ----
        b_bits, a_bits = bits(np.float32(np.float64(t0) * 0.99)), bits(t0 + inc)
        assert b_bits != a_bits and bits(t1) in (a_bits, b_bits)
        regimeB_o = bits(t1) == b_bits
        sums = oracle.tv16_block_sums(src)
        qual = np.flatnonzero(sums[:nb] >= t0)
        lim = -(-dst_len // 16)
        c0_o = dst_len if qual.size >= lim else 16 * qual.size
        head = np.concatenate([np.arange(16 * q, 16 * q + 16) for q in qual] + [np.zeros(0, np.int64)])[:c0_o]
        assert np.array_equal(idx[:c0_o], head), name  # the stream begins with the qualifying lines, in order
        tail_at = np.flatnonzero(idx >= 16 * nb)
        # the tail's stage-3 pairs start at c0; a tail that is a candidate pops
        # after a full line in every case built here (asserted per class below)
        ct_o = int(tail_at.size) if tail_at.size and tail_at[0] == c0_o else 0
        if ct_o:
            assert np.array_equal(tail_at, np.arange(c0_o, c0_o + ct_o)), name
        popped_o = bool(tail_at.size) and tail_at[0] > c0_o  # the tail came out of the heap

        # ---- the header's decision ----
        R = run_regime(exe, src, dst_len, t0, inc)
        print(name, R, "oracle:", dict(cnt=cnt_o, regimeB=regimeB_o, c0=c0_o, ct=ct_o, popped=popped_o))
        assert R["next_t"] == bits(t1), name
        assert bool(R["regimeB"]) == regimeB_o, name
        assert R["count"] == cnt_o, name
        assert R["c0"] == c0_o and R["ct"] == ct_o, name
        assert R["Qtot"] == qual.size and R["cnt"] == c0_o + ct_o, name
        assert bool(R["tail_cand"]) == (tl != 0 and c0_o < dst_len and not ct_o), name
        if popped_o:
            assert R["tail_cand"], name

        # ---- the classes, from the oracle's answers ----
        if tl == 0:
            hit.add("tl0")
        if ct_o == tl and tl:
            hit.add("tail_fits")
        if 0 < ct_o < tl and c0_o + ct_o == dst_len:
            hit.add("tail_cut")
        tail_vals = src[16 * nb:]
        if popped_o and regimeB_o and not np.isnan(tail_vals).any():
            # the tail's key as the reference forms it, and its place against the window below t
            key = np.float32(np.float32(tail_vals.sum(dtype=np.float32)) * np.float32(16)) / np.float32(tl)
            inside = bits(t0) - WIN <= bits(key) < bits(t0)
            assert bool(R["tail_in"]) == inside and R["tail_key"] == bits(key), name
            if tl and (tail_vals.view(np.uint32) == 0x80000000).all():
                hit.add("tail_minus_zero")
                assert R["tail_key"] == 0  # the sum starts from +0.f: -0.0 elements leave it +0.0
            elif inside:
                hit.add("cand_in_window")
            else:
                hit.add("cand_below_window")
        if tl and np.isnan(tail_vals).any() and regimeB_o and not ct_o:
            hit.add("tail_nan")
            assert R["tail_cand"] and (R["tail_key"] & 0x7fffffff) > 0x7f800000, name
        if dst_len % 16 and qual.size >= lim:
            hit.add("partial_line")
            assert not regimeB_o and cnt_o == dst_len
        if dst_len > n:
            hit.add("dst_past_bucket")
            assert cnt_o == n and R["M"] == nb - qual.size, name
        if qual.size == 0:
            hit.add("none_qualifies")
            assert c0_o == 0
    assert hit == set(cases(np.float32(1.0))), hit
