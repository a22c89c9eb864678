#!/usr/bin/env python3
"""Generate tests/golden/golden_ratio.npz from the REFERENCE codec itself.

Producer: oracle/_ref/libstg_ref.so (the reference's thresholdv16 and
thresholdv sources compiled in place by oracle/Makefile), exactly as
make_golden.py and make_golden_edge.py.  The cases are tests/ratio_cases.py's:
one key whose k changes between calls (the engine's
configure_compression_ratio), so a threshold taken at one k meets another.

Inputs are not stored: they are regenerated from (n, dist, seed bucket, it).
The manifest records the sha256 of every input array, so a drift of the
generator shows as a fixture problem.  Outputs per call: count, threshold and
increment bits, sha256 of the stream; the whole (idx, val) stream only for the
one-key schedules at n <= 65541, and there only for calls of at most
FULL_STREAM_MAX_COUNT pairs (the staggered keys and the ratio 0.5 / 0.1 / 0
calls keep hashes alone: the file stays under the size limit for a committed
file).  The manifest's "stored" lists say which calls have arrays.

    python tests/golden/make_golden_ratio.py
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

import ratio_cases as rc  # noqa: E402
from make_golden_edge import save_npz, sha  # noqa: E402
from oracle.oracle import Reference, build  # noqa: E402
from stellatrain_amd.synth import D1, D3  # noqa: E402


def tv16_cases():
    """(name, n, dist, param, seed bucket, key, first schedule entry, ratios, full)."""
    out = []
    for n in rc.SIZES:
        out.append((f"tv16_one_{n}", n, D1, 0, rc.SEED_BUCKET, "5@weight", 0, rc.RATIOS, n <= rc.FULL_STREAM_MAX_N))
    for n in rc.BATCH_SIZES:
        for j in range(rc.BATCH_KEYS):
            ratios = [rc.batch_ratio(j, s) for s in range(rc.BATCH_STEPS)]
            out.append((f"tv16_batch_{n}_key{j}", n, D1, 0, rc.SEED_BUCKET + 1 + j, f"rb{j}@weight", 3 * j, ratios, False))
    for n in rc.D3_SIZES:
        out.append((f"tv16_d3_{n}", n, D3, rc.D3_ZP, rc.D3_SEED_BUCKET, "5@weight", 0, rc.D3_RATIOS,
                    n <= rc.FULL_STREAM_MAX_N))
    return out


def tv_cases():
    return [(f"tv_{sched}_{n}", n, D1, 0, rc.TV_SEED_BUCKET[sched], "ptr", 0, ratios, n <= rc.FULL_STREAM_MAX_N)
            for sched, ratios in rc.TV_SCHEDULES.items() for n in rc.TV_SIZES]


def gen(ref, codec, cases, out):
    meta = []
    for (name, n, dist, param, bucket, key, first, ratios, full) in cases:
        h = ref.tv16_new() if codec == "tv16" else ref.tv_new()
        counts, tbits, incbits, hashes, inputs, ks, stored = [], [], [], [], [], [], []
        for it, r in enumerate(ratios):
            k = rc.merge_k(n, r)
            src = rc.ratio_input(n, it, dist, param, bucket)
            inputs.append(rc.sha(src.view(np.uint32)))
            if codec == "tv16":
                cnt, idx, val = ref.tv16_compress(h, key, src, k)
                t, inc = ref.tv16_state(h, key)
            else:
                cnt, idx, val = ref.tv_compress(h, 1, src, k)
                t, inc = ref.tv_state(h, 1), 0.0
            ks.append(k)
            counts.append(cnt)
            tbits.append(int(np.float32(t).view(np.uint32)))
            incbits.append(int(np.float32(inc).view(np.uint32)))
            hashes.append(sha(idx[:cnt]) + ":" + sha(val[:cnt].view(np.uint32)))
            stored.append(bool(full and cnt <= rc.FULL_STREAM_MAX_COUNT))
            if stored[-1]:
                out[f"{name}/it{it}/idx"] = idx[:cnt].copy()
                out[f"{name}/it{it}/val"] = val[:cnt].view(np.uint32).copy()
        out[f"{name}/counts"] = np.array(counts, np.int64)
        out[f"{name}/t_bits"] = np.array(tbits, np.uint32)
        out[f"{name}/inc_bits"] = np.array(incbits, np.uint32)
        meta.append({"name": name, "n": n, "dist": dist, "param": param, "seed_bucket": bucket, "key": key,
                     "first": first, "ratios": list(ratios), "ks": ks, "stored": stored, "inputs": inputs,
                     "hashes": hashes})
        (ref.tv16_free if codec == "tv16" else ref.tv_free)(h)
    return meta


def main():
    build(ref=True)
    ref = Reference()
    gxx = subprocess.run(["g++", "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    manifest = {"producer": "reference backend/src/compress compiled in place (oracle/Makefile)",
                "flags": "-std=c++17 -g -O3 -march=broadwell", "compiler": gxx, "host": platform.machine(),
                "generator": "tests/ratio_cases.py over stellatrain_amd/synth.py (splitmix64, integer-only)"}
    out: dict[str, np.ndarray] = {}
    manifest["tv16"] = gen(ref, "tv16", tv16_cases(), out)
    manifest["tv"] = gen(ref, "tv", tv_cases(), out)
    save_npz(os.path.join(HERE, "golden_ratio.npz"), out)
    with open(os.path.join(HERE, "manifest_ratio.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote", len(out), "arrays;", os.path.getsize(os.path.join(HERE, "golden_ratio.npz")) >> 10, "KiB")


if __name__ == "__main__":
    main()
