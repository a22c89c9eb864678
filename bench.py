#!/usr/bin/env python3
"""bench.py -- grad-codec GB/s (dense fp32 in), thresholdv16 k=1%.

N = 1 (the headline, BASELINE.json metric on configs[1]'s bucket size): one
*step* compresses the 64 gradient buckets of one iteration with thresholdv16:
64 keys ("<layer>@weight") x 64 MiB fp32 (n = 16,777,216, dst_len = 167,772 =
merge_numel(n, 0.99)), device resident -- 4 GiB, the fp32 gradient of a
1-billion-parameter model.  The engine issues its MERGE-compress tasks from
several pool workers at once (engine/modules/compress.cpp:141, config.h:7);
here the step is sixteen batched C-ABI calls (stg_codec_compress_batch_device)
of 4 buckets each, call j on stream j % 4 = four concurrent persistent
launches, so one launch's tail and regime-B heap fill overlap the others'
streaming.  (A timed region of K steps carries a fixed start and drain of
~0.1 ms: at the driver's K = 20, a 16-key step lost ~3 % to it, a 64-key step
~0.5 %; profiles/r06_keys_per_step_ab.txt.)  Each rank holds 8 buffer sets of
its buckets (32 GiB, >> the 256 MB Infinity Cache; --sets): step s compresses set
s % 8, so every key sees a fresh bucket on every step (the engine
alternates two shm buffers per layer, core.cpp:967, whose contents are fresh
each iteration) and its AIMD threshold runs its real regime A/B sequence.
``--jitter J`` scales each bucket by a seeded factor in [1 - J, 1 + J], so
that AIMD window misses happen at a gradient-noise rate.  Keys are initialised
(first-threshold call) before the warmup.  value = 64 x 64 MiB x steps / time.

N > 1: the same step on every rank (each its own 64 keys and buckets, seeded
by rank): buckets are independent (core.cpp:1052-1087), so the path shards
with no collective; "scaling": "weak", value = all ranks' bytes / the slowest
rank's time, and per_rank_GBps lists each rank's rate.

With ``--full`` every N also carries a ``c4`` sub-object (BASELINE.json configs[3]): the
1,024-bucket stream (256 KiB - 64 MiB, log-uniform, seeded: shard.c4_sizes)
sharded over the N ranks by shard.ShardPlan (key-affine, bytes-balanced), one
sweep = every bucket once in batched launches of <= 32 on four streams; the
list is fixed, so that is strong scaling (N = 1 runs the whole stream on one
GPU).  RCCL carries only the timing barriers and the max / sum reductions.

``--gpus N`` with N > 1 outside torchrun relaunches this script under
``torch.distributed.run`` (one process per GPU) before any GPU call.
``--backend oracle`` rehearses the multi-rank path on CPU (gloo; the CPU
restatement stands in for the device; small sizes) for tests/test_bench_cli.py.

A plain run does what the headline needs and no more: it sets up, warms up,
times the ``--steps`` steps, writes its outputs if ``--dump-outputs DIR`` is
given, and prints the result line (``ms_per_step`` = the timed region over
``--steps``).  The clock warm-up (``--warmup-seconds``) steps a twin codec
handle with its own AIMD state on the same buckets, so the measured handle has
made exactly 1 + warmup calls per key when the timed region starts and its
output does not depend on how many steps fitted into the warm-up time.
``--dump-outputs DIR`` writes what the last timed step returned to its caller,
every key's stream in key order: DIR/indices.npy (float64), DIR/values.npy
(float32) -- a fixed, seeded, sorted sample of 2 Mi positions of the
concatenated streams where they hold more, the positions in DIR/positions.npy
(float64) -- and DIR/counts.npy (float64, one per key); with N > 1 each rank writes
``<name>_rank<r>.npy``.  Equal arguments give equal inputs on every run.

``--full`` adds everything else: the ``c4`` sub-object above, and the extra
fields ``roofline`` for the dominant (only) kernel, tv16_batch, timed
live with HIP events over the profiled steps on stream 0, the other streams
joined to it (algorithmic bytes = 4n + 8k per bucket; achieved = those bytes
over the interval; pitch_us = interval x concurrent launches / launches, the
per-launch share of the chip's time -- launches overlap, so rocprofv3's
per-launch duration is longer than the pitch by the overlap factor);
``cpu_baseline`` (rank 0 at N = 1): the reference's own
backend/src/compress build (oracle/_ref, kind "reference") or the restatement
(kind "port"), timed on this host on 1 thread and on T = min(cpus, 32) threads
with distinct keys, as the engine's pool runs them (config.h:7).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md, chip-level table)
METRIC = "grad-codec GB/s (dense fp32 in) per GPU; thresholdv16 k=1% on 64 MiB bucket"


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=50)
    p.add_argument("--mib", type=int, default=64)
    p.add_argument("--ratio", type=float, default=0.99)
    p.add_argument("--keys", type=int, default=64)
    p.add_argument("--per-launch", type=int, default=4,
                   help="headline: buckets per batched call; call j runs on stream j %% S")
    p.add_argument("--method", default="thresholdv16")
    p.add_argument("--workload", choices=["auto", "headline", "c4"], default="auto",
                   help="the main line's workload (auto: the 64 MiB headline at every N; c4: the C4 stream)")
    p.add_argument("--c4-sweeps", type=int, default=3, help="timed sweeps of the c4 sub-object (0: none)")
    p.add_argument("--c4-count", type=int, default=1024)
    p.add_argument("--c4-lo", type=int, default=65536)
    p.add_argument("--c4-hi", type=int, default=16777216)
    p.add_argument("--c4-per-launch", type=int, default=32,
                   help="c4: buckets per batched call (MAX_BATCH = 32; profiles/r06_c4_per_launch_sweep.txt)")
    p.add_argument("--backend", choices=["hip", "oracle"], default="hip")
    p.add_argument("--dump-shards", default="", help="rank 0 writes every rank's bucket ids here (tests)")
    p.add_argument("--cpu-seconds", type=float, default=8.0)
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--profile-steps", type=int, default=64)
    p.add_argument("--warmup-seconds", type=float, default=2.0)
    p.add_argument("--streams", type=int, default=4,
                   help="issue batch j on stream j %% S, like the engine's worker pool; S persistent launches "
                        "share the chip")
    p.add_argument("--sets", type=int, default=8,
                   help="buffer sets rotated over the steps: each key sees a fresh bucket on every step for "
                        "SETS steps running (SURVEY 8(d)); 8 x 64 x 64 MiB = 32 GiB per GPU")
    p.add_argument("--jitter", type=float, default=0.0,
                   help="scale each (key, set) bucket by a seeded factor in [1 - J, 1 + J] (gradient-scale "
                        "noise: AIMD window misses at a realistic rate)")
    p.add_argument("--master-port", type=int, default=29517)
    p.add_argument("--dump-outputs", default="", metavar="DIR",
                   help="write what the last timed step returned (indices, values, counts) as DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also measure what the headline does not need: the c4 sub-object, the live roofline "
                        "timing, the committed profile summaries and the CPU baseline")
    return p.parse_args()


# ---------------------------------------------------------------------------
# CPU baseline (rank 0, N = 1): the reference's own compress build when it
# travelled with the tree (oracle/_ref/libstg_ref.so), else the restatement.
# ---------------------------------------------------------------------------
def cpu_model() -> str:
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_threads() -> int:
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    omp = os.environ.get("OMP_NUM_THREADS")  # the box's CPU share
    if omp and omp.isdigit():
        n = min(n, int(omp))
    return max(1, min(n, 32))


def cpu_baseline(n: int, k: int, seconds: float):
    """thresholdv16 on host buckets: 1 thread, then T threads on distinct keys
    (each with its own two alternating buckets), steady-state calls only."""
    from oracle.oracle import Oracle, Reference, REF_SO
    o = Oracle()
    kind = "reference" if os.path.exists(REF_SO) else "port"
    impl = Reference() if kind == "reference" else o
    T = cpu_threads()
    bufs = []
    for t in range(T):
        pair = []
        for s in range(2):
            b = np.empty(n, np.float32)
            o.lib.orc_synth_fill(b, n, 0x5EED0000 + t * 1000 + s, 0, 0)
            pair.append(b)
        bufs.append(pair)

    def run(nthreads, secs):
        calls = [0] * nthreads
        stop = time.perf_counter() + secs
        hs = [impl.tv16_new() for _ in range(nthreads)]
        for t in range(nthreads):  # first calls (nth_element) excluded
            impl.tv16_compress(hs[t], f"{t}@weight", bufs[t][0], k)
        barrier = threading.Barrier(nthreads + 1)

        def worker(t):
            barrier.wait()
            c = 0
            while time.perf_counter() < stop or c == 0:
                impl.tv16_compress(hs[t], f"{t}@weight", bufs[t][(c + 1) % 2], k)
                c += 1
            calls[t] = c
        ths = [threading.Thread(target=worker, args=(t,)) for t in range(nthreads)]
        for th in ths:
            th.start()
        t0 = time.perf_counter()
        barrier.wait()
        for th in ths:
            th.join()
        dt = time.perf_counter() - t0
        for h in hs:
            impl.tv16_free(h)
        return 4.0 * n * sum(calls) / dt / 1e9, sum(calls), dt

    v1, c1, d1 = run(1, seconds / 2)
    vT, cT, dT = run(T, seconds / 2)
    src = ("oracle/_ref/libstg_ref.so = the reference's compress/thresholdv16.cpp built in place, -O3 -march=broadwell"
           if kind == "reference" else "oracle/stg_oracle.cpp restatement, -O3 -march=broadwell")
    return {"value": round(vT, 3), "unit": "GB/s", "cores": T, "kind": kind, "cpu": cpu_model(),
            "value_1thread": round(v1, 3),
            "sample": f"thresholdv16 {4 * n >> 20} MiB k={k}: {T} threads x distinct keys, {cT} steady-state calls "
                      f"in {dT:.1f} s ({c1} calls in {d1:.1f} s on 1 thread); 2 alternating synthetic buckets per "
                      f"key, first call excluded; {src}"}


def jitter_factor(bucket: int, par: int, jitter: float) -> float:
    """A seeded factor in [1 - jitter, 1 + jitter] for (bucket, set): the
    splitmix64 of synth.py, so every run and world size sees the same inputs."""
    from stellatrain_amd.synth import _splitmix64, seed_for
    r = int(_splitmix64(np.array([seed_for(bucket, par) ^ 0x7A11], np.uint64))[0]) >> 11
    return float(1.0 + jitter * (2.0 * r / float(1 << 53) - 1.0))


DUMP_SAMPLE = 1 << 21  # positions of the concatenated streams kept by --dump-outputs (20 B each: 40 MiB)


def dump_outputs(dirname, world, rank, idx, val, counts):
    """What the last timed step handed its caller: the streams of all keys
    back to back (idx, val: host arrays of sum(k) entries) and each key's
    count.  Larger outputs are cut to a fixed, seeded, sorted sample."""
    os.makedirs(dirname, exist_ok=True)
    sfx = f"_rank{rank}" if world > 1 else ""
    pos = np.arange(idx.size, dtype=np.int64)
    if idx.size > DUMP_SAMPLE:
        pos = np.sort(np.random.default_rng(0x5EED).choice(idx.size, DUMP_SAMPLE, replace=False))
    for name, a in (("indices", idx[pos].astype(np.float64)), ("values", val[pos].astype(np.float32)),
                    ("positions", pos.astype(np.float64)), ("counts", np.asarray(counts, np.float64))):
        np.save(os.path.join(dirname, f"{name}{sfx}.npy"), a)


def fill_profile():
    """tv16_fill per-launch durations (p50 / p99 / max) from the committed
    rocprofv3 kernel trace summary of the headline (profiles/fill_profile.json,
    written by tools/fill_profile.py)."""
    path = os.path.join(ROOT, "profiles", "fill_profile.json")
    try:
        return json.load(open(path))
    except Exception:
        return None


def load_traffic(buckets_per_launch: int):
    """HBM bytes per tv16_batch launch from the committed rocprofv3 PMC summary
    (profiles/pmc_tv16_batch.json, written by tools/pmc_summary.py), scaled to
    this run's buckets per launch."""
    path = os.path.join(ROOT, "profiles", "pmc_tv16_batch.json")
    if not os.path.exists(path):
        return None
    try:
        d = json.load(open(path))
        return int(d["hbm_bytes_per_bucket"] * buckets_per_launch)
    except Exception:
        return None


# ---------------------------------------------------------------------------
# workloads: a list of buckets (key, n) per rank, compressed per step
# ---------------------------------------------------------------------------
def workload(args, world, rank):
    from stellatrain_amd.engine import merge_numel
    from stellatrain_amd.shard import ShardPlan, c4_sizes
    wl = args.workload
    if wl == "auto":
        wl = "headline"
    if wl == "headline":
        n = args.mib * (1 << 20) // 4
        ids = list(range(args.keys))
        span = max(64, args.keys)  # (bucket ids, hence seeds, distinct over the ranks)
        items = [(f"{rank * span + i}@weight", n, merge_numel(n, args.ratio, 1), rank * span + i) for i in ids]
        pl = max(1, min(32, args.per_launch))
        desc = {"workload": f"{args.method} k={merge_numel(n, args.ratio, 1)} (1%) on {args.mib} MiB fp32 buckets; "
                            f"step = {args.keys} keys ({args.keys * args.mib} MiB) per GPU in "
                            f"{(args.keys + pl - 1) // pl} batched calls of {pl}, call j on stream j % {args.streams}",
                "n": n, "dst_len": merge_numel(n, args.ratio, 1)}
        return wl, items, desc, {"all": [[b for *_, b in items]]}
    sizes = c4_sizes(args.c4_count, args.c4_lo, args.c4_hi)
    plan = ShardPlan(sizes, world)
    mine = plan.local(rank)
    items = [(plan.key(b), sizes[b], merge_numel(sizes[b], args.ratio, 1), b) for b in mine]
    desc = {"workload": f"C4: stream of {len(sizes)} {args.method} buckets k=1% ({args.c4_lo * 4 >> 10} KiB - "
                        f"{args.c4_hi * 4 >> 20} MiB, log-uniform, seeded) sharded over {world} GPU(s) by "
                        f"ShardPlan; step = one sweep", "buckets": len(sizes), "bytes_total": 4 * sum(sizes),
            "imbalance": round(plan.imbalance(), 5)}
    return wl, items, desc, {r: plan.local(r) for r in range(world)}


def c4_measure(args, world, rank, comp, streams, dist):
    """The c4 sub-object: this rank's ShardPlan share of the C4 stream, two
    buffer sets, one sweep = every bucket once (batches of <= 32 distinct keys,
    batch j on stream j % S); max over ranks of the timed sweeps."""
    import ctypes as C

    import torch
    from stellatrain_amd._capi import check, lib
    from stellatrain_amd.engine import merge_numel
    from stellatrain_amd.shard import ShardPlan, c4_sizes
    from stellatrain_amd.synth import seed_for
    dev = streams[0].device
    sizes = c4_sizes(args.c4_count, args.c4_lo, args.c4_hi)
    plan = ShardPlan(sizes, world)
    mine = plan.local(rank)
    ns = len(streams)
    tot = sum(sizes[b] for b in mine)
    offs = np.concatenate([[0], np.cumsum([sizes[b] for b in mine])]).astype(np.int64)
    ks = [merge_numel(sizes[b], args.ratio, 1) for b in mine]
    koffs = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
    sets = [torch.empty(max(tot, 1), dtype=torch.float32, device=dev) for _ in range(2)]
    for par in range(2):
        for j, b in enumerate(mine):
            check(lib().stg_synth_fill_device(C.c_void_p(sets[par][offs[j]:].data_ptr()), sizes[b], seed_for(b, par),
                                              0, 0, C.c_void_p(streams[0].cuda_stream)))
    oidx = torch.zeros(max(sum(ks), 1), dtype=torch.int32, device=dev)
    oval = torch.zeros(max(sum(ks), 1), dtype=torch.float32, device=dev)
    counts = torch.zeros(max(len(mine), 1), dtype=torch.int32, device=dev)
    cpl = max(1, min(32, args.c4_per_launch))
    groups = [list(range(j, min(j + cpl, len(mine)))) for j in range(0, len(mine), cpl)]
    plans = []
    for par in range(2):
        calls = []
        for j, g in enumerate(groups):
            rows = [(plan.key(mine[i]).encode(), sets[par][offs[i]:].data_ptr(), sizes[mine[i]], ks[i],
                     oidx[koffs[i]:].data_ptr(), ks[i], oval[koffs[i]:].data_ptr(), counts.data_ptr() + 4 * i)
                    for i in g]
            calls.append((comp.bucket_array(rows), len(rows), streams[j % ns].cuda_stream))
        plans.append(calls)

    def sweep(s):
        for arr, n_, sp in plans[s % 2]:
            comp.compress_batch_raw(arr, n_, sp)

    def sync():
        for st in streams[1:]:
            streams[0].wait_stream(st)
        torch.cuda.synchronize()
    for s in range(3):  # first calls (first thresholds) and warm-up
        sweep(s)
    sync()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(args.c4_sweeps):
        sweep(s)
    sync()
    el = time.perf_counter() - t0
    comp.check_device()
    assert bool((counts[:len(mine)].cpu().numpy() == np.array(ks, np.int32)).all()), "count != dst_len"
    my = torch.tensor([el, 4.0 * tot], dtype=torch.float64, device=dev)
    per_rank = [None] * world
    if world > 1:
        ts = [torch.zeros(2, dtype=torch.float64, device=dev) for _ in range(world)]
        dist.all_gather(ts, my)
        per_rank = [(float(t[0]), float(t[1])) for t in ts]
    else:
        per_rank = [(el, 4.0 * tot)]
    slow = max(e for e, _ in per_rank)
    total = sum(b for _, b in per_rank)
    return {"workload": f"C4: stream of {len(sizes)} {args.method} buckets k=1% ({args.c4_lo * 4 >> 10} KiB - "
                        f"{args.c4_hi * 4 >> 20} MiB, log-uniform, seeded) sharded over {world} GPU(s) by ShardPlan; "
                        "one sweep = every bucket once", "scaling": "strong", "buckets": len(sizes),
            "bytes_per_sweep": int(total), "sweeps": args.c4_sweeps,
            "value": round(total * args.c4_sweeps / slow / 1e9, 2), "unit": "GB/s",
            "ms_per_sweep": round(slow * 1e3 / args.c4_sweeps, 4),
            "per_rank_GBps": [round(b * args.c4_sweeps / e / 1e9, 2) for e, b in per_rank],
            "per_rank_buckets": [len(plan.local(r)) for r in range(world)],
            "rccl_world_size": dist.get_world_size() if world > 1 else 1,
            "imbalance": round(plan.imbalance(), 5)}


def spawn_ranks(args):
    """--gpus N outside torchrun: relaunch under torch.distributed.run (one
    process per GPU) before this process touches any GPU, exit with its code."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr=127.0.0.1", f"--master-port={args.master_port}", os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "0") or 0)
    if args.gpus > 1 and world == 0:
        sys.exit(spawn_ranks(args))
    world = max(world, 1)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.backend == "oracle":
        return main_oracle(args, world, rank)
    import torch
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group("nccl", init_method="env://")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    import ctypes as C

    from stellatrain_amd import make_compressor
    from stellatrain_amd._capi import check, lib
    from stellatrain_amd.synth import seed_for

    wl, items, desc, shards = workload(args, world, rank)
    nb = len(items)
    ns = max(1, min(args.streams, nb))
    comp = make_compressor(args.method, device=local)
    heat = make_compressor(args.method, device=local)  # the clock warm-up's handle: its own per-key state
    stream = torch.cuda.current_stream(dev)
    streams = [stream] + [torch.cuda.Stream(dev) for _ in range(ns - 1)]

    # args.sets buffer sets rotated over the steps (each key sees a fresh bucket
    # on every step), data seeded by bucket id and set: identical for any world
    # size; --jitter scales each (bucket, set) by a seeded factor
    tot = sum(n for _, n, _, _ in items)
    offs = np.concatenate([[0], np.cumsum([n for _, n, _, _ in items])]).astype(np.int64)
    nsets = max(1, args.sets)
    sets = [torch.empty(max(tot, 1), dtype=torch.float32, device=dev) for _ in range(nsets)]
    for par in range(nsets):
        for j, (_, n, _, b) in enumerate(items):
            check(lib().stg_synth_fill_device(C.c_void_p(sets[par][offs[j]:].data_ptr()), n, seed_for(b, par), 0, 0,
                                              C.c_void_p(stream.cuda_stream)))
            if args.jitter > 0:
                sets[par][offs[j]:offs[j] + n].mul_(jitter_factor(b, par, args.jitter))
    ks = [k for _, _, k, _ in items]
    koffs = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
    oidx = torch.zeros(max(sum(ks), 1), dtype=torch.int32, device=dev)
    oval = torch.zeros(max(sum(ks), 1), dtype=torch.float32, device=dev)
    counts = torch.zeros(max(nb, 1), dtype=torch.int32, device=dev)

    # per-step arguments resolved once: batches of --per-launch buckets (headline)
    # or of 32 (c4 as the main line), batch j on stream j % S
    if wl == "headline":
        pl = max(1, min(32, args.per_launch))
        groups = [list(range(j, min(j + pl, nb))) for j in range(0, nb, pl)]
    else:
        groups = [list(range(j, min(j + 32, nb))) for j in range(0, nb, 32)]
    plans = []
    for par in range(nsets):
        calls = []
        for j, g in enumerate(groups):
            rows = [(items[i][0].encode(), sets[par][offs[i]:].data_ptr(), items[i][1], ks[i],
                     oidx[koffs[i]:].data_ptr(), ks[i], oval[koffs[i]:].data_ptr(), counts.data_ptr() + 4 * i)
                    for i in g]
            calls.append((comp.bucket_array(rows), len(rows), streams[j % ns].cuda_stream))
        plans.append(calls)

    def step(s, c=comp):
        for arr, n_, sp in plans[s % nsets]:
            c.compress_batch_raw(arr, n_, sp)

    def sync_streams():
        for st in streams[1:]:
            stream.wait_stream(st)
        torch.cuda.synchronize()

    # first call per key: first threshold (reported, untimed for the metric)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step(0)
    sync_streams()
    first_ms = (time.perf_counter() - t0) * 1e3
    for s in range(args.warmup):
        step(s + 1)
    sync_streams()
    # the GPU holds low clocks for a while after going busy: keep stepping
    # until --warmup-seconds have passed before anything is timed (on the twin
    # handle: the measured handle's call history stays 1 + warmup per key)
    t0 = time.perf_counter()
    s = args.warmup + 1
    while time.perf_counter() - t0 < args.warmup_seconds:
        for _ in range(4):
            step(s, heat)
            s += 1
        sync_streams()
    heat.check_device()

    # ---- timed region ----
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(args.steps):
        step(s)
    t_enq = time.perf_counter() - t0
    sync_streams()
    if world > 1:
        dist.barrier()
    el = time.perf_counter() - t0
    el_mine = el
    tt = torch.tensor([el], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    el = float(tt.item())
    comp.check_device()
    if not os.environ.get("STG_DEBUG_TV16_STAGE"):  # diagnostic stages skip the fill
        assert bool((counts[:nb].cpu().numpy() == np.array(ks, np.int32)).all()), "count != dst_len"
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, world, rank, oidx[:sum(ks)].cpu().numpy().view(np.uint32),
                     oval[:sum(ks)].cpu().numpy(), counts[:nb].cpu().numpy())

    # ---- live kernel timing (--full; HIP events, no per-launch instrumentation) ----
    # events on stream 0 bracketing the profile steps of all streams: with S
    # streams, S launches overlap, so algorithmic bytes / interval is the
    # chip's rate and S x interval / launches the per-launch duration
    # rocprofv3 reports.
    def profile_interval_ms():
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ev0.record(stream)
        for st in streams[1:]:
            st.wait_event(ev0)
        for s in range(args.profile_steps):
            step(s)
        for st in streams[1:]:
            stream.wait_stream(st)
        ev1.record(stream)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)
    chip_ms = profile_interval_ms() if args.full else None

    my_bytes = 4.0 * tot
    all_bytes = torch.tensor([my_bytes], dtype=torch.float64, device=dev)
    per_rank_gbps = [round(my_bytes * args.steps / el_mine / 1e9, 2)]
    if world > 1:
        dist.all_reduce(all_bytes)
        rates = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(world)]
        dist.all_gather(rates, torch.tensor([my_bytes * args.steps / el_mine / 1e9], dtype=torch.float64, device=dev))
        per_rank_gbps = [round(float(r.item()), 2) for r in rates]
    total_bytes = float(all_bytes.item()) * args.steps
    value = total_bytes / el / 1e9
    shard_meta = None
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, {"rank": rank, "buckets": [b for *_, b in items], "bytes": my_bytes})
        shard_meta = gathered
    c4 = None
    if args.full and wl == "headline" and args.c4_sweeps > 0:
        del sets
        torch.cuda.empty_cache()
        c4 = c4_measure(args, world, rank, comp, streams, dist)
    if rank == 0:
        per_launch = nb / max(len(groups), 1)
        out = {
            "metric": METRIC,
            "value": round(value, 2),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(el * 1e3 / args.steps, 5),
            "higher_is_better": True,
            "scaling": "weak" if wl == "headline" else "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": f"synthetic (splitmix64 Irwin-Hall D1, {nsets} buffer sets of {nb} distinct buckets per GPU "
                    f"rotated over the steps: a fresh bucket per key every step"
                    + (f", each scaled by a seeded factor in [{1 - args.jitter:g}, {1 + args.jitter:g}]"
                       if args.jitter > 0 else "") + ", device resident)",
            "config": dict(desc, streams=ns, buckets_per_launch=round(per_launch, 2),
                           parallelism=f"bucket-sharded x{world}, no collective"),
            "per_gpu_GBps": round(value / world, 2),
            "per_rank_GBps": per_rank_gbps,
            "rccl_world_size": dist.get_world_size() if world > 1 else 1,
            "per_bucket_us": round(el * 1e6 / (args.steps * nb), 3),
            "first_call_ms": round(first_ms, 3),
            "host_enqueue_us_per_step": round(t_enq * 1e6 / args.steps, 2),
        }
        if shard_meta:
            out["shards"] = [{"rank": g["rank"], "buckets": len(g["buckets"]), "bytes": int(g["bytes"])}
                             for g in shard_meta]
            if args.dump_shards:
                json.dump(shard_meta, open(args.dump_shards, "w"))
        if args.full:
            alg_step = sum(4.0 * n + 8.0 * k for _, n, k, _ in items)  # 4n + 8k per bucket
            achieved = alg_step * args.profile_steps / (chip_ms * 1e-3) / 1e9
            launches = args.profile_steps * len(groups)
            conc = min(ns, len(groups))
            pitch_us = chip_ms * 1e3 * conc / max(launches, 1)
            out["roofline"] = {
                "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4),
                "traffic": load_traffic(per_launch) if wl == "headline" else None,
                "kernel": "tv16_batch", "alg_bytes_per_launch": int(alg_step / max(len(groups), 1)),
                "pitch_us": round(pitch_us, 2), "concurrent_launches": conc, "launches_timed": int(launches),
                "interval_us": round(chip_ms * 1e3, 1), "rank": 0,
                "basis": "step-level: algorithmic bytes of the profiled steps over their chip interval "
                         "(HIP events on stream 0, the other streams joined); the per-launch kernel "
                         "durations overlap (concurrent_launches in flight), so a per-kernel figure "
                         "cannot reproduce this frac",
                # the same algorithmic bytes over the timed region's wall clock (the clock
                # `value` uses, barriers and the last launches' drain included), per GPU
                "frac_timed_region": round(alg_step * args.steps / el / 1e9 / HBM_PEAK_GBS, 4)}
            fp = fill_profile() if wl == "headline" else None
            if fp:
                out["fill_profile"] = fp
        if c4 is not None:
            out["c4"] = c4
        if args.full and world == 1 and not args.no_cpu_baseline and wl == "headline":
            out["cpu_baseline"] = cpu_baseline(items[0][1], items[0][2], args.cpu_seconds)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main_oracle(args, world, rank):
    """CPU rehearsal of the rank layout (tests): gloo, the restatement standing
    in for the device, the same workloads (the headline per rank, the c4
    sub-object's ShardPlan shares), timing and reductions."""
    import torch
    import torch.distributed as dist
    from oracle.oracle import Oracle
    from stellatrain_amd.engine import merge_numel
    from stellatrain_amd.shard import ShardPlan, c4_sizes
    from stellatrain_amd.synth import seed_for
    if world > 1:
        dist.init_process_group("gloo", init_method="env://")
    wl, items, desc, _ = workload(args, world, rank)
    o = Oracle()
    h = o.tv16_new()

    def timed(items_, steps, dump=""):
        nsets = max(1, args.sets)
        data = [[o.synth(n, seed_for(b, par)) * np.float32(jitter_factor(b, par, args.jitter) if args.jitter > 0 else 1)
                 for (_, n, _, b) in items_] for par in range(nsets)]

        def step(s):
            return [o.tv16_compress(h, key, data[s % nsets][j], k) for j, (key, _, k, _) in enumerate(items_)]
        step(0)
        for s in range(args.warmup):
            step(s + 1)
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        res = None
        for s in range(steps):
            res = step(s)
        el = time.perf_counter() - t0
        cnt = [c for c, _, _ in res]
        assert cnt == [k for _, _, k, _ in items_]
        if dump:
            dump_outputs(dump, world, rank, np.concatenate([i[:c] for c, i, _ in res]).view(np.uint32),
                         np.concatenate([v[:c] for c, _, v in res]), cnt)
        mine = torch.tensor([el, 4.0 * sum(n for _, n, _, _ in items_)], dtype=torch.float64)
        if world > 1:
            allr = [torch.zeros(2, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(allr, mine)
        else:
            allr = [mine]
        slow = max(float(t[0]) for t in allr)
        total = sum(float(t[1]) for t in allr)
        return total * steps / slow / 1e9, slow, [round(float(t[1]) * steps / float(t[0]) / 1e9, 4) for t in allr]

    value, slow, per_rank = timed(items, args.steps, args.dump_outputs)
    c4 = None
    gathered = []
    if args.full and wl == "headline" and args.c4_sweeps > 0:
        sizes = c4_sizes(args.c4_count, args.c4_lo, args.c4_hi)
        plan = ShardPlan(sizes, world)
        c4_items = [(plan.key(b), sizes[b], merge_numel(sizes[b], args.ratio, 1), b) for b in plan.local(rank)]
        c4_value, c4_slow, c4_rates = timed(c4_items, args.c4_sweeps)
        c4 = {"scaling": "strong", "buckets": len(sizes), "value": round(c4_value, 4), "unit": "GB/s",
              "ms_per_sweep": round(c4_slow * 1e3 / args.c4_sweeps, 3), "per_rank_GBps": c4_rates,
              "per_rank_buckets": [len(plan.local(r)) for r in range(world)],
              "rccl_world_size": dist.get_world_size() if world > 1 else 1}
        gathered = [{"rank": rank, "buckets": plan.local(rank)}]
        if world > 1:
            gathered = [None] * world
            dist.all_gather_object(gathered, {"rank": rank, "buckets": plan.local(rank)})
    if rank == 0:
        out = {"metric": METRIC, "value": round(value, 4), "unit": "GB/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": round(slow * 1e3 / args.steps, 3),
               "higher_is_better": True, "scaling": "weak" if wl == "headline" else "strong", "vs_baseline": None,
               "dtype": "f32", "data": "synthetic (CPU rehearsal: oracle restatement standing in for the device)",
               "config": dict(desc, backend="oracle", parallelism=f"bucket-sharded x{world}, no collective"),
               "per_rank_GBps": per_rank, "rccl_world_size": dist.get_world_size() if world > 1 else 1}
        if c4 is not None:
            out["c4"] = c4
        if args.dump_shards:
            json.dump(gathered, open(args.dump_shards, "w"))
        print(json.dumps(out), flush=True)
    o.tv16_free(h)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
