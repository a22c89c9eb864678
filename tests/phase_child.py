"""Child process of tests/test_gpu_geometry.py (not a test module).

One thresholdv16 key of 2^20 + 13 floats through seven one-bucket calls, the
last three scaled by 1/100 (window misses: the crew's calls), every fourth pair
of lines tied (geometry.TIES_CHILD: the orderers have equal sums to order), with source,
index and value buffer carved at the 16-byte phases given in argv (bytes:
src idx val).  The parent sets how the regime-B fill is finished and ordered
(STG_DEBUG_TV16_FILL, STG_TV16_LF2, STG_TV16_LFIN, STG_TV16_LFIN_RANKERS: read
once per process).  Every call's count, whole stream and state are checked
against the oracle, the guards around the three buffers and the source bucket
after every call, and the path counters of tests/fill_mode_child.py are
printed as one JSON line.
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
    import geometry as G
    from oracle.oracle import Oracle
    from parity import assert_same_stream, bits
    from stellatrain_amd import ThresholdvCompressor16
    from stellatrain_amd._capi import check, lib
    phases = tuple(int(a) for a in sys.argv[1:4])
    assert len(phases) == 3
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    n, k = G.CHILD
    seq = G.tv16_sequence(Oracle(), n, k, G.BUCKET_CHILD, G.SCALES_CHILD, ties=G.TIES_CHILD)
    comp = ThresholdvCompressor16()
    src = G.carve(torch, dev, n, torch.float32, phases[0])
    idx = G.carve(torch, dev, k, torch.int32, phases[1])
    val = G.carve(torch, dev, k, torch.float32, phases[2])
    for it, (x, co, io, vo, state, _head, _regime) in enumerate(seq):
        src.copy_(torch.from_numpy(np.array(x, np.float32)))
        idx.zero_()
        val.zero_()
        cnt = comp.compress("p@w", src, k, idx, val)
        what = f"phases {phases} call {it}"
        assert cnt == co, (what, cnt, co)
        assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, co, what)
        for v, name in ((idx, "idx"), (val, "val"), (src, "src")):
            G.assert_guards(v, f"{what}: {name}")
        assert np.array_equal(bits(src.cpu().numpy()), bits(x)), f"{what}: source bucket differs"
        assert bits(np.array(comp.state("p@w"), np.float32)).tolist() == bits(np.array(state, np.float32)).tolist(), what
    comp.check_device()
    w = (C.c_uint32 * 64)()
    check(lib().stg_codec_debug_words(comp._h, C.c_void_p(st.cuda_stream), w, 64))
    print(json.dumps({"ok": True, "calls": len(seq), "phases": list(phases), "paths": list(w)[56:60],
                      "lfin": list(w)[48:52], "scan_ranked": list(w)[44:46], "stale": w[31], "wide": list(w)[52:56],
                      "mode": os.environ.get("STG_DEBUG_TV16_FILL")}), flush=True)


if __name__ == "__main__":
    main()
