"""Child process of tests/test_gpu_ratio.py (not a test module).

Runs the ratio schedule of tests/ratio_cases.py on one thresholdv16 key of
(1 << 18) + 5 floats through one-bucket calls, with STG_DEBUG_TV16_FILL and
STG_TV16_LFIN set by the parent (both read once per process; see
tests/fill_mode_child.py for the modes), checks every call's count, whole
stream and state bits against the oracle, and prints the fill's path counters
(debug words 44..45, 48..59) as one JSON line.
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


def main():
    import torch
    import ratio_cases as rc
    from oracle.oracle import Oracle
    from parity import assert_same_stream, fbits
    from stellatrain_amd import ThresholdvCompressor16
    from stellatrain_amd._capi import check, lib
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    o = Oracle()
    ho = o.tv16_new()
    comp = ThresholdvCompressor16()
    n = (1 << 18) + 5
    key = "rc@weight"
    d = torch.empty(n, dtype=torch.float32, device=dev)
    big = 0
    for it, r, k in rc.schedule(n):
        x = rc.ratio_input(n, it)
        tb = o.tv16_state(ho, key)
        co, io, vo = o.tv16_compress(ho, key, x, k)
        d.copy_(torch.from_numpy(x))
        idx = torch.zeros(k, dtype=torch.int32, device=dev)
        val = torch.zeros(k, dtype=torch.float32, device=dev)
        cnt = comp.compress(key, d, k, idx, val)
        what = f"call {it}: ratio {r}, k {k}"
        assert cnt == co, what
        assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, co, what)
        so, sg = o.tv16_state(ho, key), comp.state(key)
        assert [fbits(v) for v in so] == [fbits(v) for v in sg], what
        if tb is not None and so[0] < tb[0]:
            big = max(big, rc.fill_probe(o, x, k, tb[0], co)[2])
    comp.check_device()
    w = (C.c_uint32 * 64)()
    check(lib().stg_codec_debug_words(comp._h, C.c_void_p(st.cuda_stream), w, 64))
    w = list(w)
    print(json.dumps({"ok": True, "calls": len(rc.RATIOS), "largest_fill": big, "scan_ranked": w[44:46], "lfin": w[48:52],
                      "wide": w[52:56], "paths": w[56:60], "mode": os.environ.get("STG_DEBUG_TV16_FILL"),
                      "lfin_env": os.environ.get("STG_TV16_LFIN")}), flush=True)


if __name__ == "__main__":
    main()
