"""Child process of tests/test_gpu_edge_nan.py (not a test module).

One NaN case per process, named by argv[1], so that the parent's time limit
ends whatever a NaN might keep running:

  tv16:<kind>:<n>:<k>   8 one-bucket thresholdv16 calls
  tv16_batch            8 batched launches: both NaN kinds at both sizes, a
                        finite bucket between them, one repeated key
  tv:<kind>:<n>:<k>     8 threshold-v calls into buffers of 4 k slots, so
                        that the count shows k < cnt
  send                  the one-call send path with a NaN born in the gather
                        (inf + -inf) from call 2 on

NaNs start at a key's third call (tests/edge_values.py).  Every call's count,
whole stream and state bits are compared with the oracle; the result and the
fill's path counters (debug words 44..63) go out as one JSON line.
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


# threshold-v's seed bucket: of 93..111 on the CPU oracle, one at which both
# kinds have k < cnt on NaN calls of both sorts (asserted below)
TV_SEED_BUCKET = 102


def _state_bits(s):
    return np.array(s, np.float32).view(np.uint32).tolist()


def main():
    import torch
    from edge_values import edge_input
    from oracle.oracle import Oracle
    from parity import assert_same_stream, fbits
    from stellatrain_amd import ThresholdvCompressor, ThresholdvCompressor16
    from stellatrain_amd._capi import check, lib
    dev = torch.device("cuda", 0)
    o = Oracle()
    case = sys.argv[1].split(":")
    out = {"ok": False, "case": sys.argv[1]}

    def words(comp):
        w = (C.c_uint32 * 64)()
        check(lib().stg_codec_debug_words(comp._h, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), w, 64))
        return list(w)[44:64]

    def nan_in(a):
        return bool(((np.ascontiguousarray(a, np.float32).view(np.uint32) & 0x7FFFFFFF) > 0x7F800000).any())

    if case[0] == "tv16":
        kind, n, k = case[1], int(case[2]), int(case[3])
        comp, ho = ThresholdvCompressor16(), o.tv16_new()
        regimes, nan_sent = "", 0
        for it in range(8):
            x = edge_input(kind, n, 91, it)
            tb = o.tv16_state(ho, "nan@w")
            co, io, vo = o.tv16_compress(ho, "nan@w", x, k)
            so = o.tv16_state(ho, "nan@w")
            idx = torch.zeros(k, dtype=torch.int32, device=dev)
            val = torch.zeros(k, dtype=torch.float32, device=dev)
            assert comp.compress("nan@w", torch.from_numpy(x).to(dev), k, idx, val) == co, it
            assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, co, f"call {it}")
            assert _state_bits(so) == _state_bits(comp.state("nan@w")), it
            if tb is not None:
                regimes += "B" if so[0] < tb[0] else "A"
            nan_sent += int(nan_in(vo[:co]))
        comp.check_device()
        out.update(regimes=regimes, nan_sent=nan_sent, words_44_63=words(comp))
    elif case[0] == "tv16_batch":
        spec = [("n0@w", "nan_steady", 4103, 40, 0), ("n1@w", "nan_tail_only", 65541, 655, 9),
                ("f@w", "denorm_half", 65541, 655, 0), ("n1@w", "nan_tail_only", 65541, 655, 9),
                ("n2@w", "nan_steady", 65541, 655, 0), ("n3@w", "nan_tail_only", 4103, 40, 3)]
        comp, ho = ThresholdvCompressor16(), o.tv16_new()
        for it in range(8):
            items, ref = [], []
            for j, (key, kind, n, k, off) in enumerate(spec):
                # (the repeated key's second call of a launch is call 2 it + 1 of its key: NaN from launch 1 on)
                x = edge_input(kind, n, 92 + j, it if key != "n1@w" else 2 * it + (j == 3))
                co, io, vo = o.tv16_compress(ho, key, x, k, idx_offset=off)
                ref.append((co, io, vo, o.tv16_state(ho, key)))
                items.append((key, torch.from_numpy(x).to(dev), k, torch.zeros(k, dtype=torch.int32, device=dev),
                              torch.zeros(k, dtype=torch.float32, device=dev), off))
            counts = comp.compress_batch_async(items).cpu().numpy()
            torch.cuda.synchronize()
            last = {}
            for j, ((key, _, k, idx, val, off), (co, io, vo, so)) in enumerate(zip(items, ref)):
                assert counts[j] == co, (it, j)
                assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, co, f"call {it} {key}")
                last[key] = so
            for key, so in last.items():
                assert _state_bits(so) == _state_bits(comp.state(key)), (it, key)
        comp.check_device()
        out.update(words_44_63=words(comp))
    elif case[0] == "tv":
        kind, n, k = case[1], int(case[2]), int(case[3])
        cap = 4 * k
        comp, ho = ThresholdvCompressor(), o.tv_new()
        d = torch.empty(n, dtype=torch.float32, device=dev)  # one stable buffer: pointer-keyed state
        counts, tbits = [], []
        for it in range(8):
            x = edge_input(kind, n, TV_SEED_BUCKET, it)
            co, io, vo = o.tv_compress(ho, 1, x, k, cap=cap)
            d.copy_(torch.from_numpy(x))
            idx = torch.zeros(cap, dtype=torch.int32, device=dev)
            val = torch.zeros(cap, dtype=torch.float32, device=dev)
            assert comp.compress("ignored", d, k, idx, val) == co, it
            assert_same_stream(idx.cpu().numpy().view(np.uint32), val.cpu().numpy(), io, vo, co, f"call {it}")
            assert fbits(comp.state("", key_ptr=d.data_ptr())[0]) == fbits(o.tv_state(ho, 1)), it
            counts.append(co)
            tbits.append(fbits(o.tv_state(ho, 1)))
        comp.check_device()
        # gmax enters the next threshold only when k < cnt: on a call with NaNs in
        # the bucket, once with elements after the last NaN (a finite threshold
        # follows) and once ending in a NaN (the threshold is NaN from then on)
        over = [(tb & 0x7FFFFFFF) > 0x7F800000 for c, tb in zip(counts[2:], tbits[2:]) if c > k]
        assert False in over and True in over, (counts, tbits)
        out.update(counts=counts, t_bits=tbits)
    elif case[0] == "send":
        from test_gpu_edge_values import send_edge_cases
        from test_gpu_send_batch import _run
        seen = []

        def hook(it, j, c, idx, g0):
            seen.append((it, nan_in(g0) or int(c._pos()[1]) in idx))

        _run(dev, o, send_edge_cases(nan_from=2), calls=4, mode="engine", hook=hook)
        # the NaN is in the gathered bucket (sent, or left in the residual) in every call from 2 on
        assert not any(has for it, has in seen if it < 2) and all(has for it, has in seen if it >= 2), seen
        out.update(nan_calls=sum(int(has) for _, has in seen))
    else:
        raise SystemExit("unknown case " + sys.argv[1])
    out["ok"] = True
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
