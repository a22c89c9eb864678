#!/usr/bin/env python3
"""Sender side of one MERGE iteration, timed three ways on one GPU:

  loop      today's per-tensor sequence: merge_gather_compress_async into
            u32 / f32 temporaries per tensor, then wire_encode_batch of all
  batch     Compressor.merge_send_batch_async, marshalled from tensors per call
  prebuilt  the same call on a SendTasks built once

on two sets of 256 tensors: the first 256 sizes of the C4 list, and 256 tensors
of 60,000 floats; N = 2 gradient sources, k = 1 %, the residual carried, the
wire flag queueTx would pick per tensor.  An iteration is timed with device
events from an idle stream (so a launch-bound path pays its host time); before
each one grad[0] of the set in turn is refilled (untimed), the sets rotating so
no iteration finds its buffers where the previous one left them in the caches.
The ways alternate within every round and each has a codec handle of its own;
the median of --iters rounds after --warmup is reported, one JSON line per set.

  --only loop       runs on a tree without the batched call (the parent commit)
  --codec thresholdv  the same on a threshold-v handle (its loop zeroes the
                    temporaries first: the engine sends every slot)
  --codec topk_exact  the same on an exact top-k handle (k <= n pairs are
                    always written, so its loop needs no zeroing)
  --trace WAY       for a kernel trace run: warm up the 60,000-float set, then
                    one iteration of WAY between two stg_synth_fill_device
                    launches of 1 float (the only synth kernels of the run)
  --count-trace CSV count the kernels between those two markers in a
                    rocprofv3 kernel-trace CSV (needs no GPU)
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_sets(torch, sizes, nsets, dev):
    from stellatrain_amd import merge_numel, wire_flag
    gen = torch.Generator(device=dev).manual_seed(31)
    sets = []
    for s in range(nsets):
        ts = []
        for j, n in enumerate(sizes):
            k = merge_numel(n, 0.99)
            flag = wire_flag(n)
            fresh = torch.randn(n, generator=gen, device=dev) * 1e-3
            g1 = torch.randn(n, generator=gen, device=dev) * 1e-3
            ts.append({"key": f"{j}@s", "n": n, "k": k, "flag": flag, "fresh": fresh, "g": [torch.empty_like(fresh), g1],
                       "r": torch.zeros(n, dtype=torch.float32, device=dev),
                       "ti": torch.zeros(k, dtype=torch.int32, device=dev),
                       "tv": torch.zeros(k, dtype=torch.float32, device=dev),
                       "di": torch.zeros(k, dtype=torch.int16 if flag & 1 else torch.int32, device=dev),
                       "dv": torch.zeros(k, dtype=torch.int16 if flag & 2 else torch.float32, device=dev)})
        sets.append(ts)
    return sets


def ways_for(torch, sets, only, codec="thresholdv16"):
    import stellatrain_amd as S
    ways = {}
    make = lambda: S.make_compressor(codec)  # noqa: E731
    # threshold-v's count varies and the engine sends every slot, the unused
    # ones zero (compress.cpp:60-64): its loop zeroes the temporaries first
    # (torch._foreach_zero_; it may still run as one fill per tensor)
    temps = [[t["ti"] for t in ts] + [t["tv"] for t in ts] for ts in sets] if codec == "thresholdv" else None
    for name in ("loop", "loop_control"):  # loop_control: the loop again, on a handle of its own
        if name not in only:
            continue
        comp = make()
        cnts = [torch.zeros(len(ts), dtype=torch.int32, device=ts[0]["r"].device) for ts in sets]

        def loop(si, comp=comp, cnts=cnts):
            ts = sets[si]
            if temps:
                torch._foreach_zero_(temps[si])
            for j, t in enumerate(ts):
                comp.merge_gather_compress_async(t["key"], t["g"], t["k"], t["ti"], t["tv"], residual=t["r"],
                                                 count=cnts[si][j:j + 1])
            S.wire_encode_batch([(t["ti"], t["tv"], t["flag"], t["di"], t["dv"]) for t in ts])
        ways[name] = (loop, comp)
    items = [[(t["key"], t["g"], t["k"], t["di"], t["dv"], t["r"], t["flag"]) for t in ts] for ts in sets]
    if "batch" in only:
        comp_b = make()
        ways["batch"] = (lambda si: comp_b.merge_send_batch_async(items[si]), comp_b)
    if "prebuilt" in only:
        comp_p = make()
        pre = [S.SendTasks(it) for it in items]
        ways["prebuilt"] = (lambda si: comp_p.merge_send_batch_async(pre[si]), comp_p)
    return ways


def refill(ts):
    for t in ts:
        t["g"][0].copy_(t["fresh"])


def measure(torch, label, sizes, nsets, only, warmup, iters, codec="thresholdv16", order=None):
    """order: the ways in the order a round runs them (default: as built)."""
    dev = torch.device("cuda", 0)
    sets = build_sets(torch, sizes, nsets, dev)
    ways = ways_for(torch, sets, only, codec)
    if order:
        ways = {w: ways[w] for w in order}
    t = {w: [] for w in ways}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    turn = 0
    for r in range(warmup + iters):
        for w, (fn, _) in ways.items():
            si = turn % nsets
            turn += 1
            refill(sets[si])
            torch.cuda.synchronize()
            e0.record()
            fn(si)
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                t[w].append(e0.elapsed_time(e1))
    row = {"config": f"SEND one iteration's sender side, {label}, N=2, k=1%, residual carried"
                     + ("" if codec == "thresholdv16" else f", {codec}"), "tensors": len(sizes),
           "floats": int(sum(sizes)), "buffer_sets": nsets, "warmup": warmup, "iters": iters}
    for w, (_, comp) in ways.items():
        comp.check_device()
        row[f"{w}_ms"] = round(float(np.median(t[w])), 4)
        row[f"{w}_ms_min_max"] = [round(min(t[w]), 4), round(max(t[w]), 4)]
    if "loop" in t:
        for w in t:
            if w not in ("loop", "loop_control"):
                row[f"loop_over_{w}"] = round(row["loop_ms"] / row[f"{w}_ms"], 2)
    return row


def trace(torch, way, codec="thresholdv16"):
    from stellatrain_amd._capi import check, lib
    dev = torch.device("cuda", 0)
    sets = build_sets(torch, [60000] * 256, 1, dev)
    fn, comp = ways_for(torch, sets, {way}, codec)[way]
    mark = torch.zeros(1, dtype=torch.float32, device=dev)
    sp = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    for _ in range(4):
        refill(sets[0])
        fn(0)
    refill(sets[0])
    torch.cuda.synchronize()
    check(lib().stg_synth_fill_device(C.c_void_p(mark.data_ptr()), 1, 1, 0, 0, sp))
    fn(0)
    check(lib().stg_synth_fill_device(C.c_void_p(mark.data_ptr()), 1, 2, 0, 0, sp))
    torch.cuda.synchronize()
    comp.check_device()


def count_trace(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    marks = [i for i, n in enumerate(names) if "synth" in n]
    assert len(marks) == 2, f"{len(marks)} marker kernels in {path}"
    per = {}
    for n in names[marks[0] + 1:marks[1]]:
        n = n.replace("void ", "").replace("stg::(anonymous namespace)::", "").split("(")[0]
        per[n] = per.get(n, 0) + 1
    return {"kernels": marks[1] - marks[0] - 1, "by_name": dict(sorted(per.items(), key=lambda kv: -kv[1]))}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--root", default=ROOT, help="the tree whose stellatrain_amd is measured")
    p.add_argument("--only", default="loop,batch,prebuilt")
    p.add_argument("--sets", default="c4,small")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--iters", type=int, default=21)
    p.add_argument("--trace", default=None)
    p.add_argument("--count-trace", default=None)
    p.add_argument("--tag", default="")
    p.add_argument("--codec", default="thresholdv16", choices=["thresholdv16", "thresholdv", "topk_exact"])
    a = p.parse_args()
    if a.count_trace:
        print(json.dumps(dict({"config": f"SEND kernels of one 256-tensor iteration ({a.tag})"}, **count_trace(a.count_trace))),
              flush=True)
        return
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    if not torch.cuda.is_available():
        sys.exit("send_bench: no HIP device")
    if a.trace:
        trace(torch, a.trace, a.codec)
        return
    from stellatrain_amd.shard import c4_sizes
    only = set(a.only.split(","))
    for s in a.sets.split(","):
        label, sizes, nsets = {"c4": ("first 256 sizes of the C4 list", c4_sizes()[:256], 2),
                               "small": ("256 tensors of 60,000 floats", [60000] * 256, 4)}[s]
        row = measure(torch, label, sizes, nsets, only, a.warmup, max(20, a.iters), a.codec)
        if a.tag:
            row["tree"] = a.tag
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
