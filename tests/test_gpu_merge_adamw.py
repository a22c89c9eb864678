"""GPU parity of ``merge_adamw`` (the MERGE decompress fused with the dense
torch-rule Adam / AdamW step) against the step's formula in numpy float64 over
the float32 state and the float32 merged gradient of tests/test_gpu_merge_grad.py's
model, with the constants the host rounds.

Tolerance on fp32 outputs, derived: every operation is correctly rounded or
within 1 ulp and a chain is at most 12 roundings long, so
|got - ref| <= 16 * 2^-24 * (|ref| + s), s the magnitude of what was summed
(m': |m| + |g|; v': v + g^2; x': |x| + ss (|m| + |g|) / den; under the coupled
decay |g| stands for |g| + wd |x|).  A 16-bit parameter without a master is
within one unit in the last place of the reference rounded to its type; with a
master it is the returned master's cast, bit for bit (a NaN at a NaN: the
payload is merge_grad's cast's).  Where the reference is not finite the class
must match (NaN, +inf, -inf)."""
from __future__ import annotations

import math

import numpy as np
import pytest

from test_gpu_merge_grad import TILE, expect, make, upload

pytestmark = pytest.mark.gpu

HYP = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1)
VARIANTS = [("float32", False), ("bfloat16", False), ("bfloat16", True), ("float16", False), ("float16", True)]
PER_RANK = [0, 1, 9, 1025]
SHAPES = [(str(n), n, None) for n in (1, 3, 15, 17, 4095, 4096, 4097, 2 * TILE + 5)]
SHAPES.append(("gaps", 5 * TILE, np.r_[0:TILE, 3 * TILE:4 * TILE]))
CASES = [(lab, n, pool, w) for lab, n, pool in SHAPES for w in (1, 2, 8)]
EPS = 16 * 2.0 ** -24


def reference(p, m, v, g, step, decoupled, lr, betas, eps, weight_decay):
    """float64 (x', m', v') and their error scales from float32 inputs and the host's float32 constants."""
    f = lambda d: np.float64(np.float32(d))  # noqa: E731
    b1, b2 = betas
    decay, wd, omb1, omb2 = f(1.0 - lr * weight_decay), f(weight_decay), f(1.0 - b1), f(1.0 - b2)
    bc2s, ss = f(math.sqrt(1.0 - math.pow(b2, step))), f(lr / (1.0 - math.pow(b1, step)))
    x, m, v, g = (a.astype(np.float64) for a in (p, m, v, g))
    with np.errstate(all="ignore"):
        ag = np.abs(g)
        if decoupled:
            x1 = x * decay
        else:
            x1, ag, g = x, ag + wd * np.abs(x), g + wd * x
        m1 = f(b1) * m + omb1 * g
        v1 = f(b2) * v + omb2 * (g * g)
        den = np.sqrt(v1) / bc2s + f(eps)
        out = x1 - ss * (m1 / den)
        return (out, m1, v1), (np.abs(x) + ss * (np.abs(m) + ag) / den, np.abs(m) + ag, v + ag * ag)


def close(got, ref, scale, what):
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        assert np.all(np.abs(got[fin] - ref[fin]) <= EPS * (np.abs(ref[fin]) + scale[fin])), what
    assert np.array_equal(np.isnan(got[~fin]), np.isnan(ref[~fin])) and np.array_equal(got[~fin] > 0, ref[~fin] > 0), what


def ordered(torch, t):
    """16-bit float bits as integers that ascend with the value."""
    b = t.view(torch.int16).numpy().astype(np.int32)
    return np.where(b >= 0, b, -(b & 0x7fff))


def state(torch, n, dtype, seed):
    """(param in its type, m, v) on the host: p in +-[0.5, 2], m in +-[2^-3, 2], v in [2^-6, 4]."""
    rng = np.random.default_rng([n, seed, 77])
    sign = lambda: rng.choice(np.float32([-1, 1]), n)  # noqa: E731
    p = torch.from_numpy(sign() * rng.uniform(0.5, 2, n).astype(np.float32))
    m = torch.from_numpy(sign() * rng.uniform(2.0 ** -3, 2, n).astype(np.float32))
    v = torch.from_numpy(rng.uniform(2.0 ** -6, 4, n).astype(np.float32))
    return p.to(dtype), m, v


def run(torch, gpu, oracle, n, per_rank, world, variant, decoupled, step, seed, pool=None, alloc=None, hyp=HYP):
    """One call; returns (verify, the device tensors)."""
    from stellatrain_amd import merge_adamw
    dtype, with_master = getattr(torch, variant[0]), variant[1]
    alloc = alloc or (lambda numel, dt, kind: torch.empty(numel, dtype=dt, device=gpu))
    streams, dec = make(oracle, n, per_rank, world, seed, pool)
    p0, m0, v0 = state(torch, n, torch.float32 if with_master else dtype, seed)
    dev = {"param": alloc(n, dtype, "p"), "m": alloc(n, torch.float32, "f"), "v": alloc(n, torch.float32, "f"),
           "master": alloc(n, torch.float32, "f") if with_master else None}
    dev["param"].copy_(p0.to(dtype))
    dev["m"].copy_(m0)
    dev["v"].copy_(v0)
    if with_master:
        dev["master"].copy_(p0)
    got = merge_adamw(upload(torch, gpu, streams), per_rank, dev["param"], dev["m"], dev["v"], step,
                      decoupled=decoupled, master=dev["master"], **hyp)
    assert got is dev["param"]

    def verify():
        what = (n, per_rank, world, variant, decoupled, step)
        g = expect(dec, n)[0]
        (x1, m1, v1), (sx, sm, sv) = reference(p0.float().numpy(), m0.numpy(), v0.numpy(), g, step, decoupled, **hyp)
        close(dev["m"].cpu().numpy().astype(np.float64), m1, sm, what + ("m",))
        close(dev["v"].cpu().numpy().astype(np.float64), v1, sv, what + ("v",))
        param = dev["param"].cpu()
        if with_master or dtype == torch.float32:
            x = dev["master"].cpu() if with_master else param
            close(x.numpy().astype(np.float64), x1, sx, what + ("x",))
            if with_master:  # (a NaN stays a NaN; its payload is the kernel's cast's, not torch's)
                nan = torch.isnan(x)
                assert torch.equal(torch.isnan(param), nan), what + ("cast",)
                assert torch.equal(param.view(torch.int16)[~nan], x.to(dtype).view(torch.int16)[~nan]), what + ("cast",)
        else:
            fin = np.isfinite(x1)
            want = torch.from_numpy(x1).to(dtype)
            assert np.all(np.abs(ordered(torch, param) - ordered(torch, want))[fin] <= 1), what + ("x16",)
            assert np.array_equal(np.isnan(param.float().numpy()[~fin]), np.isnan(x1[~fin])), what + ("x16 class",)
    return verify, dev


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{c[0]}-w{c[3]}" for c in CASES])
def test_small_shapes(gpu, oracle, k):
    """Every per_rank under both decay rules; type, master and step rotate so that each meets every shape and world."""
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    _, n, pool, world = CASES[k]
    for j, per_rank in enumerate(PER_RANK):
        for decoupled in (True, False):
            r = k + 2 * j + decoupled
            run(torch, gpu, oracle, n, per_rank, world, VARIANTS[r % 5], decoupled, (1, 7)[r % 2], r, pool)[0]()
    scatter_merge_check()


@pytest.mark.parametrize("label,n,pool", [SHAPES[7], SHAPES[8]], ids=["ragged", "gaps"])
def test_first_moment_is_merge_grad_bit_for_bit(gpu, oracle, label, n, pool):
    """beta1 = 0 and no decay: exp_avg is the merged gradient itself."""
    import torch
    from stellatrain_amd import merge_grad
    hyp = dict(HYP, betas=(0.0, 0.999), weight_decay=0.0)
    for world, variant in ((8, VARIANTS[0]), (2, VARIANTS[2])):
        _, dev = run(torch, gpu, oracle, n, 1025, world, variant, True, 1, 5, pool, hyp=hyp)
        streams = upload(torch, gpu, make(oracle, n, 1025, world, 5, pool)[0])
        want = merge_grad(streams, 1025, torch.empty(n, device=gpu)).cpu()
        got, nan = dev["m"].cpu(), torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan)
        assert torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan])


@pytest.mark.parametrize("variant", VARIANTS, ids=[f"{d}{'-master' if w else ''}" for d, w in VARIANTS])
def test_every_phase_between_guards(gpu, oracle, variant):
    """The fp32 arrays together at each 16-byte phase, a 16-bit parameter at each of its eight beside them."""
    import torch
    from geometry import assert_guards, carve
    from stellatrain_amd.engine import scatter_merge_check
    for n in (2 * TILE + 5, 3):  # three tiles with a ragged last one; a tensor shorter than a word
        for fph in range(0, 16, 4):
            for hph in range(0, 16, 2) if variant[0] != "float32" else (fph,):
                held = []

                def alloc(numel, dt, kind):
                    held.append(carve(torch, gpu, numel, dt, fph if kind == "f" or dt == torch.float32 else hph))
                    return held[-1]
                run(torch, gpu, oracle, n, 1025, 2, variant, fph % 8 == 0, 7, fph + hph, alloc=alloc)[0]()
                for t in held:
                    assert_guards(t, (variant, n, fph, hph))
    scatter_merge_check()


def test_batch_is_the_loop_bit_for_bit(gpu, oracle):
    """Two groups of world 2 (16 + 1), a per_rank == 0 item, a group of world 8: as a list, and prebuilt at steps 1, 2."""
    import torch
    from stellatrain_amd import AdamWTasks, merge_adamw, merge_adamw_batch, merge_batch_launches
    from stellatrain_amd.engine import scatter_merge_check
    shapes = [((1, 4097, 33, 2 * TILE + 5, 4096)[j % 5], (1, 9, 1025)[j % 3], 2) for j in range(17)]
    shapes += [(4097, 0, 2), (1, 9, 8), (4097, 1025, 8), (2 * TILE + 5, 1, 8)]
    streams, start = [], []
    for j, (n, per_rank, world) in enumerate(shapes):
        dtype, with_master = VARIANTS[j % 5]
        p, m, v = state(torch, n, torch.float32, j)
        streams.append(upload(torch, gpu, make(oracle, n, per_rank, world, j)[0]))
        start.append([p.to(getattr(torch, dtype)).to(gpu), m.to(gpu), v.to(gpu)] + ([p.to(gpu)] if with_master else []))

    def items():
        return [(s, shape[1]) + tuple(t.clone() for t in st) for s, shape, st in zip(streams, shapes, start)]

    def same(a, b, what):
        for j, (x, y) in enumerate(zip(a, b)):
            for q, (t, u) in enumerate(zip(x[2:], y[2:])):
                w = torch.int16 if t.element_size() == 2 else torch.int32
                assert torch.equal(t.view(w), u.view(w)), (what, j, q, shapes[j])

    loop, refs = items(), []
    for step in (1, 2):
        for it in loop:
            merge_adamw(it[0], it[1], it[2], it[3], it[4], step, master=it[5] if len(it) == 6 else None, **HYP)
        refs.append([it[:2] + tuple(t.clone() for t in it[2:]) for it in loop])
    listed = items()
    outs = merge_adamw_batch(listed, 1, **HYP)
    assert all(o is it[2] for o, it in zip(outs, listed))
    same(listed, refs[0], "list")
    built = items()
    tasks = AdamWTasks(built)
    for step in (1, 2):
        before = merge_batch_launches()
        merge_adamw_batch(tasks, step, **HYP)
        # world 2: two groups of 1 + 2 + 1 launches; the per_rank == 0 item: one; world 8: 1 + 4 + 1
        assert merge_batch_launches() - before == 2 * 4 + 1 + 6
        same(built, refs[step - 1], f"prebuilt step {step}")
    scatter_merge_check()
