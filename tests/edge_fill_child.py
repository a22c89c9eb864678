"""Child process of tests/test_gpu_edge_values.py::test_edge_fill_modes (not a
test module).

Runs thresholdv16 sequences on denorm_all, wide_exp, huge and negzero buckets
(tests/edge_values.py; n = 2^20 + 13, k = 10485, 6 one-bucket calls per kind,
the last two scaled by 1/100: a window miss) with STG_DEBUG_TV16_FILL set by
the parent (read once per process: 0 = production, 1 = always the shadow heap,
2 = always the literal heap, 3 = always the leader over the window, 4 = always
the crew), checks every call's count, whole stream and state bits against the
oracle, asserts that one fill's pops tie, and prints the path counters (debug
words 44..59, named as in fill_mode_child.py) as one JSON line, per kind and
summed.
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

KINDS = ("denorm_all", "wide_exp", "huge", "negzero")
# The seed bucket at which one regime-B fill inside the window (negzero, call
# 1) pops two lines with equal sums, so that the forced shadow heap has a tie
# to order: found on the CPU (buckets 75..89 scanned), asserted below.
SEED_BUCKET = 76


def main():
    import torch
    from edge_values import edge_input
    from oracle.oracle import Oracle
    from parity import assert_same_stream, bits
    from stellatrain_amd import ThresholdvCompressor16
    from stellatrain_amd._capi import check, lib
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    o = Oracle()
    ho = o.tv16_new()
    comp = ThresholdvCompressor16()
    n, k = (1 << 20) + 13, 10485

    def words():
        w = (C.c_uint32 * 64)()
        check(lib().stg_codec_debug_words(comp._h, C.c_void_p(st.cuda_stream), w, 64))
        return np.array(list(w), np.int64)

    calls, per_kind, prev, tied_fills = 0, {}, words(), 0
    idx = torch.zeros(k, dtype=torch.int32, device=dev)
    val = torch.zeros(k, dtype=torch.float32, device=dev)
    for kind in KINDS:
        for it in range(6):
            x = edge_input(kind, n, SEED_BUCKET, it)
            if it >= 4:
                x = x * np.float32(0.01)
            cnt = comp.compress(kind, torch.from_numpy(x).to(dev), k, idx, val)
            t_before = o.tv16_state(ho, kind)
            co, io, vo = o.tv16_compress(ho, kind, x, k)
            if t_before is not None and o.tv16_state(ho, kind)[0] < t_before[0]:  # regime B: equal sums among the pops?
                sums = o.tv16_block_sums(x)
                head = 16 * int(np.count_nonzero(sums >= np.float32(t_before[0])))
                lines = io[head:co:16].astype(np.int64) // 16
                s = sums[lines[lines < sums.size]]
                tied_fills += int(np.unique(s).size < s.size)
            assert cnt == co, (kind, it)
            assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, co, f"{kind} call {it}")
            assert bits(np.array(o.tv16_state(ho, kind), np.float32)).tolist() == \
                bits(np.array(comp.state(kind), np.float32)).tolist(), (kind, it)
            calls += 1
        now = words()
        per_kind[kind] = (now - prev)[44:60].tolist()
        prev = now
    comp.check_device()
    assert tied_fills  # the shadow heap (mode 1) runs only for a fill whose pops tie
    w = words().tolist()
    print(json.dumps({"ok": True, "calls": calls, "paths": w[56:60], "lfin": w[48:52], "scan_ranked": w[44:46],
                      "wide": w[52:56], "words_44_59": w[44:60], "per_kind_44_59": per_kind,
                      "mode": os.environ.get("STG_DEBUG_TV16_FILL")}), flush=True)


if __name__ == "__main__":
    main()
