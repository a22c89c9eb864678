"""Child process of tests/test_gpu_layered.py (not a test module).

Runs the ramp and plateau keys of tests/layered.py at 2^18 + 5 floats -- regime-B
pops that are heap neighbours, window bins past their capacity, long runs of
equal sums -- through one-bucket calls and then as two keys of a batched
launch, with STG_DEBUG_TV16_FILL, STG_TV16_LFIN and STG_TV16_LF2 set by the
parent (all read once per process; see tests/fill_mode_child.py for the
modes), checks every call's count, whole stream and state bits against the
oracle, and prints the fill's path counters (debug words 44..45, 48..59) as one
JSON line.
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
    import layered as ly
    from oracle.oracle import Oracle
    from parity import assert_same_stream, fbits
    from stellatrain_amd import ThresholdvCompressor16
    from stellatrain_amd._capi import check, lib
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    o = Oracle()
    ho = o.tv16_new()
    comp = ThresholdvCompressor16()
    n = ly.SIZES[1]
    k = ly.K[n]
    kinds = ("ramp", "plateau")
    d = [torch.empty(n, dtype=torch.float32, device=dev) for _ in kinds]
    calls = 0

    def same(key, what, cnt, idx, val, exp):
        co, io, vo = exp
        assert cnt == co, what
        assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, co, what)
        so, sg = o.tv16_state(ho, key), comp.state(key)
        assert [fbits(v) for v in so] == [fbits(v) for v in sg], what

    for j, kind in enumerate(kinds):
        for it in range(ly.CALLS):
            x = ly.layered_input(kind, n, ly.seed_bucket_of(kind), it)
            exp = o.tv16_compress(ho, f"one_{kind}", x, k)
            d[j].copy_(torch.from_numpy(x))
            idx = torch.zeros(k, dtype=torch.int32, device=dev)
            val = torch.zeros(k, dtype=torch.float32, device=dev)
            cnt = comp.compress(f"one_{kind}", d[j], k, idx, val)
            same(f"one_{kind}", f"one-bucket {kind}, call {it}", cnt, idx, val, exp)
            calls += 1
    for it in range(ly.CALLS):
        items, exps = [], []
        for j, kind in enumerate(kinds):
            x = ly.layered_input(kind, n, ly.seed_bucket_of(kind), it)
            exps.append(o.tv16_compress(ho, f"batch_{kind}", x, k))
            d[j].copy_(torch.from_numpy(x))
            items.append((f"batch_{kind}", d[j], k, torch.zeros(k, dtype=torch.int32, device=dev),
                          torch.zeros(k, dtype=torch.float32, device=dev)))
        counts = comp.compress_batch_async(items).cpu().numpy().tolist()
        torch.cuda.synchronize()
        for j, kind in enumerate(kinds):
            same(f"batch_{kind}", f"batched {kind}, launch {it}", counts[j], items[j][3], items[j][4], exps[j])
            calls += 1
    comp.check_device()
    w = (C.c_uint32 * 64)()
    check(lib().stg_codec_debug_words(comp._h, C.c_void_p(st.cuda_stream), w, 64))
    w = list(w)
    print(json.dumps({"ok": True, "calls": calls, "scan_ranked": w[44:46], "lfin": w[48:52], "wide": w[52:56],
                      "paths": w[56:60], "mode": os.environ.get("STG_DEBUG_TV16_FILL"),
                      "lfin_env": os.environ.get("STG_TV16_LFIN"), "lf2_env": os.environ.get("STG_TV16_LF2")}), flush=True)


if __name__ == "__main__":
    main()
