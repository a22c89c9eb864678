#!/usr/bin/env python3
"""Generate tests/golden/golden_edge.npz from the REFERENCE codec itself.

Producer: oracle/_ref/libstg_ref.so (the reference's thresholdv16, thresholdv
and topk sources compiled in place by oracle/Makefile), exactly as
make_golden.py.  The inputs are tests/edge_values.py's: gradient buckets with
infinities, overflowing line sums, denormals, -0.0, the whole exponent range
and (in steady state only) NaNs.

Inputs are not stored: they are regenerated from (kind, n, seed_bucket, it).
The manifest records the sha256 of every input array, so a drift of the
generator shows as a fixture problem.  Outputs: counts, per-call threshold
bits, full (idx, val) streams for n <= 100013, sha256 of the streams for all.

    python tests/golden/make_golden_edge.py
"""
from __future__ import annotations

import hashlib
import io
import json
import os
import platform
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from edge_values import KINDS, edge_input, sha_input  # noqa: E402
from oracle.oracle import Reference, build  # noqa: E402

SEED_BUCKET = 29
ITERS = 8
SMALL = [(4103, 40), (65541, 655), (1000, 7)]
LARGE = ((1 << 20) + 13, 10485)
LARGE_KINDS = ("wide_exp", "denorm_all", "nan_steady")
TOPK_KINDS = ("inf", "huge", "denorm_half", "denorm_all", "negzero", "wide_exp")
TOPK_SIZES = [(4099, 41), (65536, 8192)]

# (kind, n, k, full_arrays)
CODEC_CASES = [(kind, n, k, True) for kind in KINDS for (n, k) in SMALL] + \
              [(kind, LARGE[0], LARGE[1], False) for kind in LARGE_KINDS]


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: a rerun reproduces
    the file byte for byte."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def gen_codec(ref, codec, out):
    meta = []
    for (kind, n, k, full) in CODEC_CASES:
        name = f"{codec}_{kind}_{n}"
        h = ref.tv16_new() if codec == "tv16" else ref.tv_new()
        counts, tbits, incbits, hashes, inputs = [], [], [], [], []
        for it in range(ITERS):
            src = edge_input(kind, n, SEED_BUCKET, it)
            inputs.append(sha_input(src))
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
            if full:
                out[f"{name}/it{it}/idx"] = idx[:cnt].copy()
                out[f"{name}/it{it}/val"] = val[:cnt].view(np.uint32).copy()
        out[f"{name}/counts"] = np.array(counts, np.int64)
        out[f"{name}/t_bits"] = np.array(tbits, np.uint32)
        out[f"{name}/inc_bits"] = np.array(incbits, np.uint32)
        meta.append({"name": name, "kind": kind, "n": n, "k": k, "iters": ITERS, "full": full,
                     "seed_bucket": SEED_BUCKET, "key": "5@weight" if codec == "tv16" else "ptr",
                     "inputs": inputs, "hashes": hashes})
        (ref.tv16_free if codec == "tv16" else ref.tv_free)(h)
    return meta


def gen_topk(ref, out):
    meta = []
    for kind in TOPK_KINDS:
        for (n, k) in TOPK_SIZES:
            name = f"topk_{kind}_{n}"
            src = edge_input(kind, n, SEED_BUCKET + 1, 0)
            cnt, idx, val = ref.topk_compress(src, k)
            out[f"{name}/idx"] = idx.copy()
            out[f"{name}/val"] = val.view(np.uint32).copy()
            meta.append({"name": name, "kind": kind, "n": n, "k": k, "seed_bucket": SEED_BUCKET + 1, "count": cnt,
                         "inputs": [sha_input(src)]})
    return meta


def main():
    build(ref=True)
    ref = Reference()
    gxx = subprocess.run(["g++", "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    manifest = {"producer": "reference backend/src/compress compiled in place (oracle/Makefile)",
                "flags": "-std=c++17 -g -O3 -march=broadwell", "compiler": gxx, "host": platform.machine(),
                "generator": "tests/edge_values.py over stellatrain_amd/synth.py (splitmix64, integer-only)"}
    out: dict[str, np.ndarray] = {}
    manifest["tv16"] = gen_codec(ref, "tv16", out)
    manifest["tv"] = gen_codec(ref, "tv", out)
    manifest["topk"] = gen_topk(ref, out)
    save_npz(os.path.join(HERE, "golden_edge.npz"), out)
    with open(os.path.join(HERE, "manifest_edge.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote", len(out), "arrays;", os.path.getsize(os.path.join(HERE, "golden_edge.npz")) >> 10, "KiB")


if __name__ == "__main__":
    main()
