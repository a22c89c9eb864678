"""bench.py's multi-GPU entry on CPU: ``--gpus 2`` relaunches the script under
torch.distributed.run (one process per rank) before any device call; each
rank runs the headline step on its own keys (weak scaling) and then its
ShardPlan share of the C4 bucket stream (BASELINE.json configs[3], the ``c4``
sub-object, strong scaling) -- here with the CPU restatement standing in for
the device (``--backend oracle``, gloo, scaled-down sizes) -- and rank 0
prints the one JSON line with n_gpus equal to the ranks that joined.  N = 1
carries the same c4 sub-object, so the 1..N curve has one workload.  The c4
sub-object belongs to ``--full``; a plain run times the headline steps alone
and ``--dump-outputs DIR`` writes what its last step returned.
"""
from __future__ import annotations

import json
import os
import socket
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _bench(args, tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--backend", "oracle", "--c4-count", "48",
                        "--c4-hi", "131072", "--c4-sweeps", "1", "--mib", "1", "--keys", "4", "--steps", "2",
                        "--warmup", "1", "--master-port", str(_free_port())] + args,
                       capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # only rank 0 prints
    return json.loads(lines[0])


def _run(args, tmp_path):
    dump = tmp_path / "shards.json"
    out = _bench(["--full", "--dump-shards", str(dump)] + args, tmp_path)
    return out, json.load(open(dump))


def test_bench_gpus2_spawns_two_ranks_with_disjoint_shards(tmp_path):
    out, shards = _run(["--gpus", "2"], tmp_path)
    assert out["n_gpus"] == 2 and out["rccl_world_size"] == 2
    assert out["scaling"] == "weak" and out["config"]["n"] == (1 << 20) // 4
    assert len(out["per_rank_GBps"]) == 2 and min(out["per_rank_GBps"]) > 0
    c4 = out["c4"]
    assert c4["scaling"] == "strong" and c4["buckets"] == 48 and c4["rccl_world_size"] == 2
    assert len(c4["per_rank_GBps"]) == 2 and sum(c4["per_rank_buckets"]) == 48
    assert sorted(g["rank"] for g in shards) == [0, 1]
    a, b = (set(g["buckets"]) for g in sorted(shards, key=lambda g: g["rank"]))
    assert a and b and not (a & b)
    assert a | b == set(range(48))
    sys.path.insert(0, ROOT)
    from stellatrain_amd.shard import ShardPlan, c4_sizes
    plan = ShardPlan(c4_sizes(48, 65536, 131072), 2)
    assert sorted(a) == plan.local(0) and sorted(b) == plan.local(1)
    assert out["value"] > 0 and out["steps"] == 2


def test_bench_single_rank_headline_layout(tmp_path):
    """N = 1: the headline workload (keys x one bucket size) and the whole C4
    stream on the one rank in the c4 sub-object."""
    out, shards = _run(["--gpus", "1"], tmp_path)
    assert out["n_gpus"] == 1 and out["scaling"] == "weak" and out["rccl_world_size"] == 1
    assert out["config"]["n"] == (1 << 20) // 4
    assert out["c4"]["buckets"] == 48 and out["c4"]["per_rank_buckets"] == [48]
    assert len(shards) == 1 and len(shards[0]["buckets"]) == 48


def test_bench_plain_run_is_the_headline_alone_and_dumps_its_last_step(tmp_path):
    """Without --full: the result line, no c4 sub-object, no CPU baseline.
    --dump-outputs: the last timed step's streams of the 4 keys back to back
    (float64 indices, float32 values, float64 counts), equal on a second run
    and equal to the oracle called 1 + warmup + steps times per key on the
    buckets the bench rotates."""
    outs = []
    for d in ("a", "b"):
        out = _bench(["--gpus", "1", "--dump-outputs", str(tmp_path / d)], tmp_path)
        assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
        assert out["unit"] == "GB/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
        assert "c4" not in out and "cpu_baseline" not in out and "roofline" not in out
        outs.append({n: np.load(tmp_path / d / f"{n}.npy") for n in ("indices", "values", "counts", "positions")})
    a, b = outs
    n = (1 << 20) // 4
    sys.path.insert(0, ROOT)
    from oracle.oracle import Oracle
    from stellatrain_amd.engine import merge_numel
    from stellatrain_amd.synth import seed_for
    k = merge_numel(n, 0.99, 1)
    assert a["indices"].dtype == np.float64 and a["values"].dtype == np.float32 and a["counts"].dtype == np.float64
    assert a["counts"].tolist() == [k] * 4 and a["indices"].shape == a["values"].shape == (4 * k,)
    assert np.array_equal(a["positions"], np.arange(4 * k))
    for name in a:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), name
    o = Oracle()
    h = o.tv16_new()
    for key in range(4):
        # step s reads buffer set s % 8: the first call and the timed steps 0, 1 bracket warm-up step 1
        for par in (0, 1, 0, 1):
            cnt, idx, val = o.tv16_compress(h, f"{key}@weight", o.synth(n, seed_for(key, par)), k)
        assert cnt == k
        assert np.array_equal(a["indices"][key * k:(key + 1) * k], idx.astype(np.float64))
        assert np.array_equal(a["values"][key * k:(key + 1) * k].view(np.uint32), val.view(np.uint32))
    o.tv16_free(h)
