#!/usr/bin/env python3
"""Generate tests/golden/golden_layered.npz from the REFERENCE codec itself.

Producer: oracle/_ref/libstg_ref.so (the reference's thresholdv16, thresholdv
and topk sources compiled in place by oracle/Makefile), exactly as
make_golden.py, make_golden_edge.py and make_golden_ratio.py.  The inputs are
tests/layered.py's: buckets whose large values cluster by position.

Inputs are not stored: they are regenerated from (kind, n, seed bucket, it).
The manifest records the sha256 of every input array, so a drift of the
generator shows as a fixture problem.  Outputs per call: count, threshold and
increment bits, sha256 of the stream; the whole (idx, val) stream only at
65,541 floats (the file stays smaller than golden_ratio.npz).  Top-k: the
reference's stream as shipped (it selects among the first quarter of the
bucket), and what an exact top-k must agree with, from the reference's own
selection over the whole bucket (gen_topk says how): the k-th magnitude, the
sha256 of the sorted signed bit patterns above it and the number of elements at
it.

    python tests/golden/make_golden_layered.py
"""
from __future__ import annotations

import json
import os
import platform
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import layered as ly  # noqa: E402
from make_golden_edge import save_npz, sha  # noqa: E402
from oracle.oracle import Reference, build  # noqa: E402


def topk_summary(val: np.ndarray):
    """(bits of the smallest magnitude kept, sha256 of the sorted signed bit
    patterns above it, elements at it)."""
    v = np.asarray(val, np.float32)
    cut = np.abs(v).min()
    above = np.sort(v[np.abs(v) > cut].view(np.uint32))
    return int(cut.view(np.uint32)), sha(above), int(np.count_nonzero(np.abs(v) == cut))


def gen_codec(ref, codec, cases, out):
    meta = []
    for kind, n in cases:
        name, k, bucket = f"{codec}_{kind}_{n}", ly.K[n], ly.seed_bucket_of(kind)
        h = ref.tv16_new() if codec == "tv16" else ref.tv_new()
        counts, tbits, incbits, hashes, inputs = [], [], [], [], []
        for it in range(ly.CALLS):
            src = ly.layered_input(kind, n, bucket, it)
            inputs.append(sha(src.view(np.uint32)))
            if codec == "tv16":
                cnt, idx, val = ref.tv16_compress(h, "5@weight", src, k)
                t, inc = ref.tv16_state(h, "5@weight")
            else:
                cnt, idx, val = ref.tv_compress(h, 1, src, k)
                t, inc = ref.tv_state(h, 1), 0.0
            counts.append(cnt)
            tbits.append(int(np.float32(t).view(np.uint32)))
            incbits.append(int(np.float32(inc).view(np.uint32)))
            hashes.append(sha(idx[:cnt]) + ":" + sha(val[:cnt].view(np.uint32)))
            if n <= ly.FULL_STREAM_MAX_N:
                out[f"{name}/it{it}/idx"] = idx[:cnt].copy()
                out[f"{name}/it{it}/val"] = val[:cnt].view(np.uint32).copy()
        out[f"{name}/counts"] = np.array(counts, np.int64)
        out[f"{name}/t_bits"] = np.array(tbits, np.uint32)
        out[f"{name}/inc_bits"] = np.array(incbits, np.uint32)
        meta.append({"name": name, "kind": kind, "n": n, "k": k, "seed_bucket": bucket, "full": n <= ly.FULL_STREAM_MAX_N,
                     "inputs": inputs, "hashes": hashes})
        (ref.tv16_free if codec == "tv16" else ref.tv_free)(h)
    return meta


def gen_topk(ref, out):
    meta = []
    for kind, n in ly.topk_cases():
        name, k, bucket = f"topk_{kind}_{n}", ly.K[n], ly.seed_bucket_of(kind)
        inputs, hashes, cuts, above, at_cut = [], [], [], [], []
        for it in range(ly.TOPK_CALLS):
            src = ly.layered_input(kind, n, bucket, it)
            inputs.append(sha(src.view(np.uint32)))
            cnt, idx, val = ref.topk_compress(src, k)
            assert cnt == k
            hashes.append(sha(idx) + ":" + sha(val.view(np.uint32)))
            # the reference copies numel bytes, a quarter of the floats
            # (topk.cpp:31), and selects among those: given the bucket as the
            # first quarter of a four times longer array it selects over the
            # whole bucket
            cnt, _, whole = ref.topk_compress(np.concatenate([src, np.zeros(3 * n, np.float32)]), k)
            assert cnt == k and np.count_nonzero(src) >= k
            c, a, m = topk_summary(whole)
            cuts.append(c)
            above.append(a)
            at_cut.append(m)
            if n <= ly.FULL_STREAM_MAX_N:
                out[f"{name}/it{it}/val"] = val.view(np.uint32).copy()  # (the indices are 0 .. k-1)
        out[f"{name}/cut_bits"] = np.array(cuts, np.uint32)
        out[f"{name}/at_cut"] = np.array(at_cut, np.int64)
        meta.append({"name": name, "kind": kind, "n": n, "k": k, "seed_bucket": bucket, "full": n <= ly.FULL_STREAM_MAX_N,
                     "inputs": inputs, "hashes": hashes, "above": above})
    return meta


def main():
    build(ref=True)
    ref = Reference()
    gxx = subprocess.run(["g++", "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    manifest = {"producer": "reference backend/src/compress compiled in place (oracle/Makefile)",
                "flags": "-std=c++17 -g -O3 -march=broadwell", "compiler": gxx, "host": platform.machine(),
                "generator": "tests/layered.py over stellatrain_amd/synth.py (splitmix64, integer-only)"}
    out: dict[str, np.ndarray] = {}
    manifest["tv16"] = gen_codec(ref, "tv16", ly.tv16_cases(), out)
    manifest["tv"] = gen_codec(ref, "tv", ly.tv_cases(), out)
    manifest["topk"] = gen_topk(ref, out)
    save_npz(os.path.join(HERE, "golden_layered.npz"), out)
    with open(os.path.join(HERE, "manifest_layered.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote", len(out), "arrays;", os.path.getsize(os.path.join(HERE, "golden_layered.npz")) >> 10, "KiB")


if __name__ == "__main__":
    main()
