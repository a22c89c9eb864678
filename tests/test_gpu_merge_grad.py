"""GPU parity of ``merge_grad`` (the MERGE decompress as a dense float32 /
bfloat16 / float16 gradient) against plain numpy float32: per rank a zero array
with the decoded pairs assigned (the last occurrence wins), the arrays summed in
rank order from zeros, one division by float32(world), torch's CPU cast for the
16-bit types.  Bitwise wherever the result is not a NaN; NaN positions match."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 4096
VALS = np.arange(-8, 9, dtype=np.float32) / np.float32(4)  # exact in fp16; holds 0.0
SPECIAL = np.array([np.inf, -np.inf, np.nan, 1e-41, -0.0], np.float32)
DTYPES = ["float32", "bfloat16", "float16"]
PER_RANK = [0, 1, 9, 1025]
# (label, n, index pool): "gaps" has pairs in tiles 0 and 3 only; 40000 takes u16 indices >= 0x8000
SHAPES = [(str(n), n, None) for n in (1, 33, 4095, 4096, 4097, 2 * TILE + 5, 40000, 70001)]
SHAPES.append(("gaps", 5 * TILE, np.r_[0:TILE, 3 * TILE:4 * TILE]))
CASES = [(lab, n, pool, w) for lab, n, pool in SHAPES for w in (1, 2, 3, 8)]


def make(oracle, n, per_rank, world, seed, pool=None):
    """(wire streams, decoded pairs): flags mixed per rank (u16 indices only where n < 65,536); in every rank an
    index twice, one the other ranks hold too, n itself, the specials, and a u16 block index >= 0x8000."""
    rng = np.random.default_rng([n, per_rank, world, seed])
    pool = np.arange(min(n + 3, 1 << 17)) if pool is None else pool
    streams, dec = [], []
    for r in range(world):
        flag = (r + seed) % 4 & (3 if n < 65536 else 2)
        idx = rng.choice(pool, per_rank).astype(np.uint32)
        val = VALS[rng.integers(0, VALS.size, per_rank)]
        if per_rank >= 9:
            idx[[0, 7]] = idx[8]                      # a repeat across the block / tail edge
            idx[1], idx[2] = pool[0], n               # shared by every rank; dropped
            val[3:8] = SPECIAL
            if flag & 1:
                idx[4] = 0x8000 + n // 8              # sign-extends past n in the block part
        wi = idx.astype(np.uint16 if flag & 1 else np.uint32)
        wv = val.astype(np.float16).view(np.uint16) if flag & 2 else val
        streams.append((wi, wv, flag))
        dec.append(oracle.wire_decode(wi, wv, flag))
    return streams, dec


def expect(dec, n):
    acc, union = np.zeros(n, np.float32), np.zeros(n, bool)
    with np.errstate(invalid="ignore"):
        for i, v in dec:
            d, k = np.zeros(n, np.float32), i < n
            d[i[k]] = v[k]
            union[i[k]] = True
            acc = acc + d
        return acc / np.float32(len(dec)), union


def upload(torch, gpu, streams):
    def t(a):
        dt = {2: np.int16, 4: np.int32}[a.itemsize] if a.dtype.kind == "u" else a.dtype
        return torch.from_numpy(a.view(dt).copy()).to(gpu)
    return [(t(wi), t(wv), f) for wi, wv, f in streams]


def bits(torch, t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()


def prior_of(torch, n, dtype, seed):
    """What `out` holds before a call: values, some -0.0, some NaNs with payloads."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).to(dtype)
    p[::5] = -0.0
    raw = p.view(torch.int16 if p.element_size() == 2 else torch.int32)
    raw[2::7] = -0x5b if p.element_size() == 2 else -0x5b5b5b  # 0xffa5 / 0xffa4a4a5: NaNs
    return p


def check(torch, dec, n, prior, got, accumulate, what):
    """`got` (the device's result over `prior`) against the numpy model."""
    merged, union = expect(dec, n) if dec else (np.zeros(n, np.float32), np.zeros(n, bool))
    m = torch.from_numpy(merged)
    want = torch.where(torch.from_numpy(union), (prior.float() + m).to(prior.dtype), prior) if accumulate \
        else m.to(prior.dtype)
    got = got.cpu()
    nan = torch.isnan(want).numpy() & ~(accumulate & ~union)  # untouched elements keep even a NaN's bits
    assert np.array_equal(torch.isnan(got).numpy()[nan], nan[nan]), what
    assert np.array_equal(bits(torch, got)[~nan], bits(torch, want)[~nan]), what


def run(torch, gpu, oracle, n, per_rank, world, dtype, accumulate, seed, pool=None, out=None):
    from stellatrain_amd import merge_grad
    streams, dec = make(oracle, n, per_rank, world, seed, pool)
    prior = prior_of(torch, n, dtype, seed)
    out = torch.empty(n, dtype=dtype, device=gpu) if out is None else out
    out.copy_(prior)
    merge_grad(upload(torch, gpu, streams), per_rank, out, accumulate=accumulate)
    return lambda: check(torch, dec, n, prior, out, accumulate, (n, per_rank, world, dtype, accumulate))


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{c[0]}-w{c[3]}" for c in CASES])
def test_small_shapes(gpu, oracle, k):
    """Every per_rank in both modes; the output type rotates so that each meets every shape and world."""
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    _, n, pool, world = CASES[k]
    for j, per_rank in enumerate(PER_RANK):
        for acc in (False, True):
            run(torch, gpu, oracle, n, per_rank, world, getattr(torch, DTYPES[(k + j) % 3]), acc, k + j, pool)()
    scatter_merge_check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_output_phase_between_guards(gpu, oracle, dtype):
    import torch
    from geometry import assert_guards, carve
    from stellatrain_amd.engine import scatter_merge_check
    dt = getattr(torch, dtype)
    item = torch.empty(0, dtype=dt).element_size()
    for n in (2 * TILE + 5, 3):  # three tiles with a ragged last one; a tensor shorter than its head
        for phase in range(0, 16, item):
            for acc in (False, True):
                out = carve(torch, gpu, n, dt, phase)
                run(torch, gpu, oracle, n, 1025, 2, dt, acc, phase, out=out)()
                assert_guards(out, (dtype, n, phase, acc))
    scatter_merge_check()


def test_back_to_back_calls_leave_the_counters_zero(gpu, oracle):
    """Two shapes on one stream with no sync between: the second buckets into the counters the first left."""
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    a = run(torch, gpu, oracle, 5 * TILE, 1025, 3, torch.float32, False, 1)
    b = run(torch, gpu, oracle, 2 * TILE + 5, 1025, 2, torch.bfloat16, True, 2)
    c = run(torch, gpu, oracle, 5 * TILE, 9, 3, torch.float16, False, 3)
    for verify in (a, b, c):
        verify()
    scatter_merge_check()
