#!/usr/bin/env python3
"""Publishing one step's changed parameters to R same-device replicas, timed
five ways on one GPU:

  items     publish_params marshalled from tensors per call
  prebuilt  the same call on a PublishTasks built once
  single    the same tasks one call each (prebuilt one-task arrays)
  scalar    `prebuilt` with STG_DEBUG_PUBLISH_SCALAR=1: the kernel without
            run detection, every element a store of its own
  dense     the alternative: replica.copy_(param) per tensor per replica

on two shapes, at R = 1 and R = 7 float32 replicas:

  small  256 tensors of 60,000 floats, each with the index-ascending union of
         eight ranks' thresholdv16-shaped streams (k = merge_numel(n, 0.99, 8)
         per rank: whole lines of 16 and one cut line)
  big    one tensor of 16 Mi floats with a thresholdv16-shaped k = 1 % stream
         (aligned lines of 16 in scan order)

and `prebuilt`, `scalar` and `dense` on the big tensor with the stream grown
to 2 .. 64 % of it (the fraction above which the dense copy wins; the two
kernels where the launch no longer hides them).

A call is timed with device events from an idle stream, so a launch-bound way
pays its host time.  Before every timed call a 512 MiB buffer is overwritten
(untimed), twice the Infinity Cache, and the calls rotate over buffer sets
with streams of their own, so no call finds parameters, indices or replicas
in a cache.  The ways alternate within every round; the median, minimum and
maximum of --iters rounds after --warmup are reported, one JSON line per
shape and R.  After the timing every replica is checked against the
parameter at the published indices.

Peer (xGMI) replicas are not measured: every replica is on the master's GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLUSH_BYTES = 512 << 20


def lines_stream(rng, n, k):
    """k indices as thresholdv16 emits them: whole aligned lines of 16 in
    ascending line order, the last one cut."""
    lines = np.sort(rng.choice(n // 16, (k + 15) // 16, replace=False))
    return (lines[:, None] * 16 + np.arange(16)[None, :]).reshape(-1)[:k].astype(np.uint32)


def union_stream(rng, n, per_rank, world):
    """The MERGE output of `world` such streams: each index once, ascending."""
    return np.unique(np.concatenate([lines_stream(rng, n, per_rank) for _ in range(world)])).astype(np.uint32)


def build_set(torch, dev, rng, sizes, stream_of, R):
    ts = []
    for n in sizes:
        idx, cap = stream_of(n)
        buf = np.zeros(cap, np.uint32)
        buf[:idx.size] = idx
        ts.append({"p": torch.randn(n, device=dev), "idx": torch.from_numpy(buf.view(np.int32)).to(dev),
                   "cnt": torch.tensor([idx.size], dtype=torch.int32, device=dev), "k": int(idx.size),
                   "reps": [torch.zeros(n, device=dev) for _ in range(R)]})
    return ts


def ways_for(sets, only):
    import stellatrain_amd as S
    items = [[(t["p"], t["idx"], t["cnt"], t["reps"]) for t in ts] for ts in sets]
    pre = [S.PublishTasks(it) for it in items]
    ways = {}
    if "items" in only:
        ways["items"] = lambda si: S.publish_params(items[si])
    if "prebuilt" in only:
        ways["prebuilt"] = lambda si: S.publish_params(pre[si])
    if "single" in only:
        one = [[S.PublishTasks([x]) for x in it] for it in items]

        def single(si):
            for x in one[si]:
                S.publish_params(x)
        ways["single"] = single
    if "scalar" in only:
        def scalar(si):
            os.environ["STG_DEBUG_PUBLISH_SCALAR"] = "1"
            try:
                S.publish_params(pre[si])
            finally:
                del os.environ["STG_DEBUG_PUBLISH_SCALAR"]
        ways["scalar"] = scalar
    if "dense" in only:
        def dense(si):
            for t in sets[si]:
                for r in t["reps"]:
                    r.copy_(t["p"])
        ways["dense"] = dense
    return ways


def verify(torch, sets):
    for ts in sets:
        for t in ts:
            j = t["idx"][:t["k"]].long()
            for r in t["reps"]:
                assert torch.equal(r[j], t["p"][j]), "a replica differs from the parameter at a published index"


def measure(torch, label, sizes, stream_of, R, nsets, only, warmup, iters, flush):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(41)
    sets = [build_set(torch, dev, rng, sizes, stream_of, R) for _ in range(nsets)]
    ways = ways_for(sets, only)
    t = {w: [] for w in ways}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    turn = 0
    for r in range(warmup + iters):
        for w, fn in ways.items():
            si = turn % nsets
            turn += 1
            flush.add_(1)
            torch.cuda.synchronize()
            e0.record()
            fn(si)
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                t[w].append(e0.elapsed_time(e1))
    verify(torch, sets)
    k = sum(x["k"] for x in sets[0])
    row = {"config": f"PUBLISH {label}, R={R} float32 replicas on the master's GPU", "tensors": len(sizes),
           "floats": int(sum(sizes)), "published": k, "fraction": round(k / sum(sizes), 5), "R": R,
           "buffer_sets": nsets, "flush_MiB": FLUSH_BYTES >> 20, "warmup": warmup, "iters": iters}
    for w in ways:
        row[f"{w}_ms"] = round(float(np.median(t[w])), 4)
        row[f"{w}_ms_min_max"] = [round(min(t[w]), 4), round(max(t[w]), 4)]
    if "dense" in t and "prebuilt" in t:
        row["dense_over_prebuilt"] = round(row["dense_ms"] / row["prebuilt_ms"], 2)
    if "scalar" in t and "prebuilt" in t:
        row["scalar_over_prebuilt"] = round(row["scalar_ms"] / row["prebuilt_ms"], 2)
    del sets, ways
    torch.cuda.empty_cache()
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--root", default=ROOT, help="the tree whose stellatrain_amd is measured")
    p.add_argument("--only", default="items,prebuilt,single,scalar,dense")
    p.add_argument("--shapes", default="small,big,sweep")
    p.add_argument("--replicas", default="1,7")
    p.add_argument("--sweep", default="2,4,8,16,32,64", help="stream sizes of the sweep, in percent of the tensor")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--iters", type=int, default=21)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_publish.jsonl"))
    a = p.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    if not torch.cuda.is_available():
        sys.exit("publish_bench: no HIP device")
    from stellatrain_amd import merge_numel
    only = set(a.only.split(","))
    flush = torch.zeros(FLUSH_BYTES // 4, device="cuda:0")
    big_n = 16 << 20
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))

    for R in [int(x) for x in a.replicas.split(",")]:
        for s in a.shapes.split(","):
            if s == "small":
                def stream_of(n, rng=np.random.default_rng(43)):
                    per = merge_numel(n, 0.99, 8)
                    return union_stream(rng, n, per, 8), per * 8
                emit(measure(torch, "256 tensors of 60,000 floats, world-8 unions", [60000] * 256, stream_of, R, 4,
                             only, a.warmup, a.iters, flush))
            elif s == "big":
                def stream_of(n, rng=np.random.default_rng(47)):
                    k = merge_numel(n, 0.99)
                    return lines_stream(rng, n, k), k
                emit(measure(torch, "one tensor of 16 Mi floats, thresholdv16-shaped k = 1 % stream", [big_n], stream_of,
                             R, 2, only, a.warmup, a.iters, flush))
            elif s == "sweep":
                for pct in [int(x) for x in a.sweep.split(",")]:
                    def stream_of(n, rng=np.random.default_rng(53 + pct), pct=pct):
                        k = n * pct // 100
                        return lines_stream(rng, n, k), k
                    emit(measure(torch, f"one tensor of 16 Mi floats, lines-of-16 stream of {pct} %", [big_n], stream_of,
                                 R, 2, only & {"prebuilt", "scalar", "dense"}, a.warmup, a.iters, flush))


if __name__ == "__main__":
    main()
