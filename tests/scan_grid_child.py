"""Child process of tests/test_gpu_scan_grid.py (not a test module).

Runs six thresholdv16 AIMD calls of one batched launch of three buckets with
the scan's grid forced by STG_DEBUG_TV16_GRID (set by the parent; read once
per process) and its counters on (STG_DEBUG_TV16_COUNT=1).  The buckets are
130 chunks + 21 floats (a ragged tail), one chunk, and 66 chunks; a chunk is
32,768 floats, so the bucket boundaries fall where a look-back that crossed
them would pick up the neighbour's counts.  Call 0 takes the first
thresholds; from call 1 on D1 data at k = 1 % alternates regime B / regime A.
Every call's whole stream and count is compared bit-exactly with the oracle,
the device check must be clean, and the counters (debug words 1, 2, 4:
workgroups that never took a chunk, the most of them in one launch, scan
launches) are printed as one JSON line.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHUNK = 32768  # floats per scan chunk (2048 lines of 16)
SIZES = [130 * CHUNK + 21, CHUNK, 66 * CHUNK]
CALLS = 6


def chunks_per_call() -> int:
    return sum(max(1, (n // 16 + 2047) // 2048) for n in SIZES)


def main():
    import torch
    from oracle.oracle import Oracle
    from parity import assert_same_stream
    from stellatrain_amd import ThresholdvCompressor16, merge_numel
    from stellatrain_amd._capi import check, lib
    from stellatrain_amd.synth import D1, seed_for, synth
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    o = Oracle()
    ho = o.tv16_new()
    comp = ThresholdvCompressor16()
    ks = [merge_numel(n, 0.99) for n in SIZES]
    regimes = []
    for it in range(CALLS):
        items, ref, reg = [], [], ""
        for j, (n, k) in enumerate(zip(SIZES, ks)):
            x = synth(n, seed_for(900 + j, it), D1)
            t0 = o.tv16_state(ho, f"sg{j}")[0] if it else None
            ref.append(o.tv16_compress(ho, f"sg{j}", x, k))
            # AIMD: the threshold falls after a regime-B call and rises after a regime-A one
            reg += "-" if t0 is None else ("B" if o.tv16_state(ho, f"sg{j}")[0] < t0 else "A")
            items.append((f"sg{j}", torch.from_numpy(x).to(dev), k, torch.zeros(k, dtype=torch.int32, device=dev),
                          torch.zeros(k, dtype=torch.float32, device=dev)))
        regimes.append(reg)
        counts = comp.compress_batch_async(items).cpu().numpy()
        torch.cuda.synchronize()
        for j, ((_, _, k, ig, vg), (co, io, vo)) in enumerate(zip(items, ref)):
            assert counts[j] == co, (it, j, int(counts[j]), co)
            assert_same_stream(ig.cpu().numpy().view(np.uint32), vg.cpu().numpy(), io, vo, co,
                               f"call {it} bucket {j} regime {reg[j]}")
    comp.check_device()
    seen = "".join(regimes)
    assert "A" in seen and "B" in seen, regimes
    w = (C.c_uint32 * 8)()
    check(lib().stg_codec_debug_words(comp._h, C.c_void_p(st.cuda_stream), w, 8))
    print(json.dumps({"ok": True, "calls": CALLS, "chunks": chunks_per_call(), "dead": w[1], "dead_max": w[2],
                      "launches": w[4], "regimes": regimes,
                      "grid": os.environ.get("STG_DEBUG_TV16_GRID")}), flush=True)


if __name__ == "__main__":
    main()
