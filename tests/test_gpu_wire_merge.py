"""GPU parity of the MERGE decompress and the fused optimizer steps read
straight from wire-form rank streams (``stg_scatter_merge_wire_device``,
``stg_merge_optimize_{sgd,adam}_wire_device``, ``stg_wire_decode_batch_device``).

Everything is a bit-for-bit comparison against (a) the oracle pair --
``oracle.wire_decode`` per rank, then ``oracle.merge_decompress`` -- and (b)
the sequence the call replaces, on the device: ``wire_decode`` per rank into
one buffer, then the decoded entry point.  Inputs and (a) come from
tests/wire_merge_cases.py, which tests/test_wire_merge_host.py checks.
"""
from __future__ import annotations

import numpy as np
import pytest

import wire_merge_cases as W

pytestmark = pytest.mark.gpu


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.itemsize == 2 else a.view(np.uint32)


def _up(torch, gpu, a):
    """A wire array on the device, int16-typed for the 16-bit forms."""
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _place(torch, gpu, a, how):
    """The wire array in a device buffer: 'plain'; 'odd' -- one element into a
    larger tensor, so only element-aligned; 'exact' -- exactly its elements
    inside a larger tensor whose other elements hold 0x7fff (as an index: a
    valid one that would join the union; as a value: a NaN / a large float)."""
    t = _up(torch, gpu, a)
    if how == "plain":
        return t
    lead = 1 if how == "odd" else 8
    big = torch.full((lead + t.numel() + 24,), 0x7fff, dtype=t.dtype, device=gpu)
    big[lead:lead + t.numel()] = t
    return big[lead:lead + t.numel()]


def _sorted_stream(oi, ov, cnt):
    c = int(cnt.cpu().numpy().view(np.uint32)[0])
    assert c != 0xffffffff
    i = oi.cpu().numpy().view(np.uint32)[:c]
    v = ov.cpu().numpy().view(np.uint32)[:c]
    o = np.argsort(i, kind="stable")
    return i[o], v[o]


class _Scratch:
    """dense / mark of the largest n, shared by the calls (left zero by each)."""

    def __init__(self, torch, gpu):
        self.dense = torch.zeros(1 << 20, dtype=torch.float32, device=gpu)
        self.mark = torch.zeros(1 << 20, dtype=torch.uint8, device=gpu)


@pytest.fixture(scope="module")
def scratch(gpu):
    import torch
    return _Scratch(torch, gpu)


def _check_merge(torch, gpu, oracle, scratch, family, per_rank, flag, world, how="plain"):
    from stellatrain_amd import scatter_merge, scatter_merge_wire, wire_decode
    n = W.n_of(flag)
    streams = W.make_streams(oracle, family, per_rank, flag, world)
    idx, val, ei, ev, st = W.expected(oracle, streams, per_rank, n)
    dev = [(_place(torch, gpu, wi, how), _place(torch, gpu, wv, how), f) for wi, wv, f in streams]
    dense, mark = scratch.dense[:n], scratch.mark[:n]
    got = _sorted_stream(*scatter_merge_wire(dev, per_rank, n, dense=dense, mark=mark))
    case = (family, per_rank, flag, world, how)
    # (a) the oracle pair
    assert np.array_equal(got[0], ei), case
    assert np.array_equal(got[1], ev.view(np.uint32)), case
    # (b) decode per rank into one buffer, then the decoded merge, on the device
    di = torch.empty(per_rank * world, dtype=torch.int32, device=gpu)
    dv = torch.empty(per_rank * world, dtype=torch.float32, device=gpu)
    for r, (wi, wv, f) in enumerate(dev):
        wire_decode(wi.contiguous(), wv.contiguous(), f, di[r * per_rank:(r + 1) * per_rank],
                    dv[r * per_rank:(r + 1) * per_rank])
    assert np.array_equal(di.cpu().numpy().view(np.uint32), idx), case
    assert np.array_equal(dv.cpu().numpy().view(np.uint32), val.view(np.uint32)), case
    two = _sorted_stream(*scatter_merge(di, dv, per_rank, world, n, dense=dense, mark=mark))
    assert np.array_equal(got[0], two[0]) and np.array_equal(got[1], two[1]), case


@pytest.mark.parametrize("world", W.WORLDS)
@pytest.mark.parametrize("flag", W.FLAGS)
def test_merge_parity(gpu, oracle, scratch, flag, world):
    """1. scatter_merge_wire against the oracle pair and the device two-step,
    every per_rank of the grid, both input families."""
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    for family in W.FAMILIES:
        for per_rank in W.PER_RANK:
            _check_merge(torch, gpu, oracle, scratch, family, per_rank, flag, world)
    scatter_merge_check()
    assert not bool(scratch.dense.view(torch.int32).any()) and not bool(scratch.mark.any())


@pytest.mark.parametrize("how", ["odd", "exact"])
@pytest.mark.parametrize("flag", W.FLAGS)
def test_merge_misaligned_and_buffer_end(gpu, oracle, scratch, flag, how):
    """2. every rank buffer one element into its tensor (only element-aligned:
    the single-load path); 3. rank buffers of exactly per_rank elements with a
    pattern behind them that would change the result if read."""
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    for family in W.FAMILIES:
        for per_rank in ([1025, 4099] if how == "odd" else [1, 7, 9, 1023, 1025, 4099]):
            for world in W.WORLDS:
                _check_merge(torch, gpu, oracle, scratch, family, per_rank, flag, world, how)
    scatter_merge_check()
    assert not bool(scratch.dense.view(torch.int32).any()) and not bool(scratch.mark.any())


def _unique_streams(oracle, flag, world, per_rank, seed):
    """Streams whose ranks each hold distinct indices below 32768 (exact as
    u16): no repeat and nothing dropped, so world 1 takes the emission's
    copy-through path."""
    rng = np.random.default_rng([per_rank, flag, world, seed])
    out = []
    for r in range(world):
        idx = rng.choice(32768, per_rank, replace=False).astype(np.uint32)
        val = (rng.standard_normal(per_rank) * 10.0 ** rng.integers(-3, 4, per_rank)).astype(np.float32)
        wi, wv = oracle.wire_encode(idx, val, flag)
        out.append((wi, wv, flag))
    return out


def _calls(oracle, flag, world, n, seed):
    """Five calls' streams on one name: index sets that differ per call, so
    elements skip iterations.  Calls 0, 2, 4: the encoded family (indices over
    [0, n): saturated repeats, so world 1 elects through the tickets); calls
    1, 3: no repeats (its copy-through path)."""
    return [W.make_streams(oracle, "encoded", 1025, flag, world, seed=seed + c, specials=False) if c % 2 == 0
            else _unique_streams(oracle, flag, world, 1025, seed + c) for c in range(5)]


def _decoded(torch, gpu, dev, per_rank):
    from stellatrain_amd import wire_decode
    world = len(dev)
    di = torch.empty(per_rank * world, dtype=torch.int32, device=gpu)
    dv = torch.empty(per_rank * world, dtype=torch.float32, device=gpu)
    for r, (wi, wv, f) in enumerate(dev):
        wire_decode(wi, wv, f, di[r * per_rank:(r + 1) * per_rank], dv[r * per_rank:(r + 1) * per_rank])
    return di, dv


SGD_OPTS = {
    "plain": dict(lr=0.05),
    "nesterov_wd": dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=0.01),
    "smart": dict(lr=0.05, momentum=0.9, dampening=0.1, smart_momentum=True),
}


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("flag", [1, 3])
@pytest.mark.parametrize("opt", list(SGD_OPTS))
def test_sgd_parity(gpu, oracle, scratch, opt, flag, world):
    """4. merge_optimize_wire against wire_decode + merge_optimize on a twin
    handle: parameters, momentum, last, iteration() and the returned stream."""
    import torch
    from stellatrain_amd import SparseSGD
    from stellatrain_amd.engine import scatter_merge_check
    n, per_rank = W.n_of(flag), 1025
    a, b = SparseSGD(**SGD_OPTS[opt]), SparseSGD(**SGD_OPTS[opt])
    p0 = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    pa, pb = torch.from_numpy(p0).to(gpu), torch.from_numpy(p0).to(gpu)
    dense, mark = scratch.dense[:n], scratch.mark[:n]
    touched = np.zeros(n, np.int64)
    for c, streams in enumerate(_calls(oracle, flag, world, n, 40)):
        dev = [(_up(torch, gpu, wi), _up(torch, gpu, wv), f) for wi, wv, f in streams]
        ga = _sorted_stream(*a.merge_optimize_wire(pa, "w", dev, per_rank, dense=dense, mark=mark))
        di, dv = _decoded(torch, gpu, dev, per_rank)
        gb = _sorted_stream(*b.merge_optimize(pb, "w", di, dv, per_rank, world, dense=dense, mark=mark))
        assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[1], gb[1]), c
        ei, ev = W.expected(oracle, streams, per_rank, n)[2:4]  # the merged stream is the oracle pair's too
        assert np.array_equal(ga[0], ei) and np.array_equal(ga[1], ev.view(np.uint32)), c
        touched[ei] += 1
        assert a.iteration == b.iteration == c + 1
        assert np.array_equal(pa.cpu().numpy().view(np.uint32), pb.cpu().numpy().view(np.uint32)), c
    assert ((touched > 0) & (touched < 5)).any()  # some index skipped an iteration
    assert not np.array_equal(pa.cpu().numpy(), p0)
    if SGD_OPTS[opt].get("momentum"):
        assert np.array_equal(a.momentum_buffer("w", n).view(np.uint32), b.momentum_buffer("w", n).view(np.uint32))
    if opt == "smart":
        la, lb = a.last_buffer("w", n), b.last_buffer("w", n)
        assert np.array_equal(la, lb) and la.max() == 4
    a.check()
    b.check()
    scatter_merge_check()


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("flag", [1, 3])
@pytest.mark.parametrize("amsgrad", [False, True])
def test_adam_parity(gpu, oracle, scratch, amsgrad, flag, world):
    """5. The same for Adam, compared through state()."""
    import torch
    from stellatrain_amd import SparseAdam
    from stellatrain_amd.engine import scatter_merge_check
    n, per_rank = W.n_of(flag), 1025
    kw = dict(lr=0.01, weight_decay=0.01, amsgrad=amsgrad)
    a, b = SparseAdam(**kw), SparseAdam(**kw)
    p0 = np.random.default_rng(6).standard_normal(n).astype(np.float32)
    pa, pb = torch.from_numpy(p0).to(gpu), torch.from_numpy(p0).to(gpu)
    dense, mark = scratch.dense[:n], scratch.mark[:n]
    for c, streams in enumerate(_calls(oracle, flag, world, n, 60)):
        dev = [(_up(torch, gpu, wi), _up(torch, gpu, wv), f) for wi, wv, f in streams]
        ga = _sorted_stream(*a.merge_optimize_wire(pa, "w", dev, per_rank, dense=dense, mark=mark))
        di, dv = _decoded(torch, gpu, dev, per_rank)
        gb = _sorted_stream(*b.merge_optimize(pb, "w", di, dv, per_rank, world, dense=dense, mark=mark))
        assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[1], gb[1]), c
        assert np.array_equal(pa.cpu().numpy().view(np.uint32), pb.cpu().numpy().view(np.uint32)), c
    sa, sb = a.state("w", n), b.state("w", n)
    assert np.array_equal(sa[0].view(np.uint32), sb[0].view(np.uint32))
    assert np.array_equal(sa[1].view(np.uint32), sb[1].view(np.uint32))
    assert np.float32(sa[2]).view(np.uint32) == np.float32(sb[2]).view(np.uint32) and sa[3] == sb[3] == 6
    assert sa[0].any() and not np.array_equal(pa.cpu().numpy(), p0)
    a.check_device()
    b.check_device()
    scatter_merge_check()


@pytest.mark.parametrize("world", [1, 3])
def test_flag0_equals_scatter_merge_on_the_concatenation(gpu, oracle, scratch, world):
    """6. All flags 0 and non-adjacent buffers: scatter_merge on the
    concatenation."""
    import torch
    from stellatrain_amd import scatter_merge, scatter_merge_wire
    n, per_rank = W.n_of(0), 4099
    streams = W.make_streams(oracle, "encoded", per_rank, 0, world)
    dev = []
    for wi, wv, f in streams:  # each rank in a tensor of its own, with a gap allocation between them
        dev.append((_up(torch, gpu, wi), _up(torch, gpu, wv), 0))
        _ = torch.empty(4096 + 64 * len(dev), dtype=torch.uint8, device=gpu)
    cat_i, cat_v = torch.cat([d[0] for d in dev]), torch.cat([d[1] for d in dev])
    dense, mark = scratch.dense[:n], scratch.mark[:n]
    a = scatter_merge_wire(dev, per_rank, n, dense=dense, mark=mark)
    b = scatter_merge(cat_i, cat_v, per_rank, world, n, dense=dense, mark=mark)
    ca = int(a[2].cpu()[0])
    assert ca == int(b[2].cpu()[0]) and 0 < ca < per_rank * world
    # unsorted: world 1 keeps the stream order, world > 1 is index-ascending
    assert torch.equal(a[0][:ca], b[0][:ca]) and torch.equal(a[1][:ca].view(torch.int32), b[1][:ca].view(torch.int32))


def test_wire_decode_batch_matches_single(gpu, oracle):
    """7. 37 streams (three launches of <= 16), mixed flags, lengths incl. 0
    and < 8: the bytes of single wire_decode calls and of the oracle.  The
    random value words include signalling fp16 NaNs (about one word in 64),
    which widen quiet on both sides (tests/test_wire_isa_host.py)."""
    import torch
    from stellatrain_amd import wire_decode, wire_decode_batch
    rng = np.random.default_rng(11)
    lens = [0, 1, 7, 8, 9, 655, 4099] + [int(x) for x in rng.integers(1, 20000, 30)]
    assert len(lens) == 37
    items, expect = [], []
    for j, m in enumerate(lens):
        flag = j % 4
        wi = rng.integers(0, 1 << 16, m).astype(np.uint16) if flag & 1 else rng.integers(0, 1 << 32, m, dtype=np.uint32)
        wv = (rng.integers(0, 1 << 16, m).astype(np.uint16) if flag & 2
              else rng.standard_normal(m).astype(np.float32))
        di, dv = _up(torch, gpu, wi), _up(torch, gpu, wv)
        io = torch.full((max(m, 1),), -1, dtype=torch.int32, device=gpu)[:m]
        vo = torch.full((max(m, 1),), -1, dtype=torch.float32, device=gpu)[:m]
        items.append((di, dv, flag, io, vo))
        expect.append(oracle.wire_decode(wi, wv, flag))
    wire_decode_batch(items)
    torch.cuda.synchronize()
    for (di, dv, flag, io, vo), (ei, ev) in zip(items, expect):
        assert np.array_equal(_u(io.cpu().numpy()), ei)
        assert np.array_equal(_u(vo.cpu().numpy()), _u(ev))
        si, sv = wire_decode(di, dv, flag)
        assert torch.equal(si, io) and torch.equal(sv.view(torch.int32), vo.view(torch.int32))


@pytest.mark.parametrize("world", [1, 2])
def test_shared_scratch(gpu, oracle, scratch, world):
    """8. A decoded scatter_merge before and after a wire call on the same
    stream: both give their usual result; the shared scratch is left zero."""
    import torch
    from stellatrain_amd import scatter_merge, scatter_merge_wire
    from stellatrain_amd.engine import scatter_merge_check
    flag, per_rank = 3, 1025
    n = W.n_of(flag)
    dense, mark = scratch.dense[:n], scratch.mark[:n]
    streams = W.make_streams(oracle, "encoded", per_rank, flag, world, seed=7)
    idx, val, ei, ev, _ = W.expected(oracle, streams, per_rank, n)
    di = torch.from_numpy(idx.view(np.int32)).to(gpu)
    dv = torch.from_numpy(val).to(gpu)
    dev = [(_up(torch, gpu, wi), _up(torch, gpu, wv), f) for wi, wv, f in streams]
    for step in ("decoded", "wire", "decoded"):
        if step == "wire":
            got = _sorted_stream(*scatter_merge_wire(dev, per_rank, n, dense=dense, mark=mark))
        else:
            got = _sorted_stream(*scatter_merge(di, dv, per_rank, world, n, dense=dense, mark=mark))
        assert np.array_equal(got[0], ei) and np.array_equal(got[1], ev.view(np.uint32)), step
        assert not bool(dense.view(torch.int32).any()) and not bool(mark.any()), step
    scatter_merge_check()
