"""GPU parity of the tile-bucketed sparse MERGE decompress
(``scatter_merge_sparse``, ``merge_optimize_sparse``) against a plain numpy
model written out here -- per rank the last occurrence of every in-range
index, np.float32 adds in rank order from +0.0, one np.float32 division,
ascending order -- bit for bit, and, where the dense path can run, against
``scatter_merge_wire`` / ``merge_optimize_wire``."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 4096
VALS = np.arange(-8, 9, dtype=np.float32) / np.float32(4)  # exact in fp16; holds 0.0


def decode(w_idx, w_val, flag, per_rank):
    """The receiver's decode: blocks sign-extend and widen fp16, the tail zero-extends and takes (float)."""
    wend = 8 * ((per_rank - 1) // 8)
    idx, val = w_idx.astype(np.uint32), w_val
    if flag & 1:
        idx[:wend] = w_idx[:wend].view(np.int16).astype(np.int32).view(np.uint32)
    if flag & 2:
        val = w_val.astype(np.float32)
        val[:wend] = w_val[:wend].view(np.float16).astype(np.float32)
    return idx, val


def model(decoded, n):
    last = [{int(j): v for j, v in zip(i, x) if j < n} for i, x in decoded]
    union = sorted(set().union(*last)) if last else []
    out = []
    for j in union:
        s = np.float32(0.0)
        for d in last:
            if j in d:
                s = np.float32(s + d[j])
        out.append(s / np.float32(len(decoded)))
    return np.array(union, np.uint32), np.array(out, np.float32)


def make(n, per_rank, world, seed, plants=()):
    """`world` wire streams from one seeded generator, flags mixed per rank (u16 only where n < 65,536);
    planted in every rank: n, n + 1, each tile's first and last slot, an index twice, a -0.0."""
    rng = np.random.default_rng([n % (1 << 31), per_rank, world, seed])
    tiles = [t for t in sorted({0, 1, 2, (n - 1) // TILE}) if t * TILE < n]
    plants = [min(n, 2 ** 32 - 1), min(n + 1, 2 ** 32 - 1)] + list(plants)
    twice = plants[-1] if len(plants) > 2 else 0
    plants += [j for t in tiles for j in (t * TILE, min(n, (t + 1) * TILE) - 1)] + [twice]
    streams = []
    for r in range(world):
        flag = (r + seed) % 4 & (3 if n < 65536 else 2)
        idx = rng.integers(0, min(n + 3, 2 ** 32), per_rank, dtype=np.uint64)
        val = VALS[rng.integers(0, VALS.size, per_rank)]
        for k, j in enumerate(plants):
            idx[(5 * k + r) % per_rank] = j
        val[(3 + r) % per_rank] = np.float32(-0.0)
        wi = idx.astype(np.uint16 if flag & 1 else np.uint32)
        wv = val.astype(np.float16).view(np.uint16) if flag & 2 else val
        streams.append((wi, wv, flag))
    return streams


def upload(torch, gpu, streams):
    def t(a):
        dt = {2: np.int16, 4: np.int32}[a.itemsize] if a.dtype.kind == "u" else a.dtype
        return torch.from_numpy(a.view(dt).copy()).to(gpu)
    return [(t(wi), t(wv), f) for wi, wv, f in streams]


def host(t, c=None):
    return t.cpu().numpy().view(np.uint32)[:c]


def run(torch, gpu, streams, n, per_rank, dense=True, what=None):
    """One case through scatter_merge_sparse against the model (and the dense path)."""
    from stellatrain_amd import scatter_merge_sparse, scatter_merge_wire
    world = len(streams)
    ei, ev = model([decode(wi, wv, f, per_rank) for wi, wv, f in streams], n)
    dev = upload(torch, gpu, streams)
    oi = torch.full((per_rank * world,), -91, dtype=torch.int32, device=gpu)
    ov = torch.full((per_rank * world,), -91.0, dtype=torch.float32, device=gpu)
    _, _, cnt = scatter_merge_sparse(dev, per_rank, n, out_idx=oi, out_val=ov)
    c = int(host(cnt)[0])
    assert c == ei.size, (what, c, ei.size)
    assert np.array_equal(host(oi, c), ei) and np.array_equal(host(ov, c), ev.view(np.uint32)), what
    assert (oi[c:] == -91).all() and (ov[c:] == -91.0).all(), what  # nothing written past the count
    if dense:
        di, dv, dc = scatter_merge_wire(dev, per_rank, n)
        d = int(host(dc)[0])
        gi, gv = host(di, d), host(dv, d)
        if world == 1:  # the dense path keeps stream order there
            o = np.argsort(gi, kind="stable")
            gi, gv = gi[o], gv[o]
        assert d == c and np.array_equal(gi, ei) and np.array_equal(gv, ev.view(np.uint32)), what
    return c


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 33, 4095, 4096, 4097, 3 * 4096 + 5, 70001])
def test_small_shapes(gpu, n, world):
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    for per_rank in (1, 9, 600):
        assert run(torch, gpu, make(n, per_rank, world, per_rank), n, per_rank, what=(n, world, per_rank)) >= 1
    scatter_merge_check()


@pytest.mark.parametrize("case", ["index0", "one_tile", "one_per_tile"])
def test_pathological_occupancy(gpu, case):
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    rng = np.random.default_rng(11)
    if case == "index0":       # every pair of every rank at index 0
        n, world, per_rank = 70001, 8, 5000
        idx = [np.zeros(per_rank, np.uint32) for _ in range(world)]
    elif case == "one_tile":   # every pair inside tile 1: segments past the register-held records
        n, world, per_rank = 70001, 3, 5000
        idx = [rng.integers(TILE, 2 * TILE, per_rank).astype(np.uint32) for _ in range(world)]
    else:                      # exactly one pair per tile over 64 tiles
        n, world, per_rank = 64 * TILE, 2, 32
        idx = [((r * per_rank + np.arange(per_rank)) * TILE + rng.integers(0, TILE, per_rank)).astype(np.uint32)
               for r in range(world)]
    streams = [(i, VALS[rng.integers(0, VALS.size, per_rank)], 0) for i in idx]
    c = run(torch, gpu, streams, n, per_rank, what=case)
    assert c == {"index0": 1, "one_per_tile": 64}.get(case, c)
    scatter_merge_check()


def test_large_n_without_a_dense_array(gpu):
    """n = 2^32 - 1: first tile, last (partial) tile, a few between, shared indices, n dropped.  The
    model only (13 n bytes of dense scratch would be 55 GB); the scratch is the documented formula."""
    import torch
    from stellatrain_amd import merge_sparse_scratch_bytes
    from stellatrain_amd.engine import scatter_merge_check, scatter_merge_release
    n, world, per_rank = 2 ** 32 - 1, 3, 600
    plants = [0, 5, TILE - 1, 2 ** 32 - 2, 2 ** 32 - TILE, 2 ** 32 - TILE - 1, 1 << 31, (1 << 31) + TILE, 123456789]
    streams = make(n, per_rank, world, 7, plants)
    scatter_merge_release()
    c = run(torch, gpu, streams, n, per_rank, dense=False, what="2^32-1")
    assert c > 1000
    T, P = (n + TILE - 1) // TILE, world * per_rank
    want = 4 * world * T + 12 * min(T, P) + 12 * P + 16
    assert merge_sparse_scratch_bytes(per_rank, world, n) == want == 12626128  # nothing of n's size
    scatter_merge_check()


def test_scratch_reuse(gpu):
    """Counters that were not re-zeroed show in the third call."""
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    for seed, n in enumerate((3 * 4096 + 5, (1 << 20) + 13, 33)):
        run(torch, gpu, make(n, 600, 3, seed), n, 600, what=("reuse", n))
    scatter_merge_check()


OPTS = {"sgd": ("sgd", dict(lr=0.05, momentum=0.9)),
        "smart": ("sgd", dict(lr=0.05, momentum=0.9, smart_momentum=True)),
        "adam": ("adam", dict(lr=0.01)),
        "amsgrad": ("adam", dict(lr=0.01, amsgrad=True))}


@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("opt", list(OPTS))
def test_fused_steps(gpu, opt, world):
    """Three calls on one name, bitwise merge_optimize_wire's on a second handle with the same history."""
    import torch
    from stellatrain_amd import SparseAdam, SparseSGD
    from stellatrain_amd.engine import scatter_merge_check
    kind, kw = OPTS[opt]
    n, per_rank = 3 * 4096 + 5, 600
    a, b = ((SparseSGD if kind == "sgd" else SparseAdam)(**kw) for _ in range(2))
    p0 = torch.from_numpy(np.random.default_rng(5).standard_normal(n).astype(np.float32)).to(gpu)
    pa, pb = p0.clone(), p0.clone()
    for call in range(3):
        streams = make(n, per_rank, world, call)
        ei, ev = model([decode(wi, wv, f, per_rank) for wi, wv, f in streams], n)
        dev = upload(torch, gpu, streams)
        ai, av, ac = a.merge_optimize_sparse(pa, "w", dev, per_rank)
        bi, bv, bc = b.merge_optimize_wire(pb, "w", dev, per_rank)
        c = int(host(ac)[0])
        assert c == int(host(bc)[0]) == ei.size, (opt, world, call)
        assert np.array_equal(host(ai, c), ei) and np.array_equal(host(av, c), ev.view(np.uint32)), (opt, world, call)
        assert np.array_equal(host(ai, c), host(bi, c)) and np.array_equal(host(av, c), host(bv, c)), (opt, world, call)
        assert np.array_equal(host(pa), host(pb)), (opt, world, call)
    assert not np.array_equal(host(pa), host(p0))
    if kind == "sgd":
        assert np.array_equal(a.momentum_buffer("w", n).view(np.uint32), b.momentum_buffer("w", n).view(np.uint32))
        assert a.iteration == b.iteration == 3
        if kw.get("smart_momentum"):
            assert np.array_equal(a.last_buffer("w", n), b.last_buffer("w", n))
        a.check()
    else:
        sa, sb = a.state("w", n), b.state("w", n)
        assert all(np.array_equal(sa[q].view(np.uint32), sb[q].view(np.uint32)) for q in (0, 1))
        assert np.float32(sa[2]).view(np.uint32) == np.float32(sb[2]).view(np.uint32) and sa[3] == sb[3]
        a.check_device()
    scatter_merge_check()


def test_refusals(gpu):
    """Each refusal gives the status the wire entry gives; per_rank == 0 gives count 0."""
    import torch
    from stellatrain_amd._capi import StgRankStream, lib
    L = lib()
    buf = torch.zeros(64, dtype=torch.int32, device=gpu)
    p, scr = buf.data_ptr(), C.c_void_p(buf.data_ptr() + 128)
    out = C.c_void_p(p + 64)
    cases = {"world 0": ([(p, p, 0)], 4, 0), "flag bit": ([(p, p, 0), (p, p, 4)], 4, 2),
             "null buffer": ([(None, p, 0)], 4, 1), "misaligned": ([(p + 2, p, 2)], 4, 1)}
    for what, (rs, per_rank, world) in cases.items():
        ranks = (StgRankStream * len(rs))(*[StgRankStream(*r) for r in rs])
        got = L.stg_scatter_merge_sparse_device(ranks, per_rank, world, 100, out, out, out, None)
        err = L.stg_last_error()
        assert got == L.stg_scatter_merge_wire_device(ranks, per_rank, world, 100, scr, scr, out, out, out, None) == -1, what
        assert err == L.stg_last_error(), what
    from stellatrain_amd import scatter_merge_sparse
    cnt = torch.full((1,), 5, dtype=torch.int32, device=gpu)
    scatter_merge_sparse([(buf, buf.view(torch.float32), 0)] * 2, 0, 100, count=cnt)
    assert int(cnt.cpu()[0]) == 0
