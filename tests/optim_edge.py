"""Edge-valued inputs of the receiving side: MERGE decompress and the SGD / Adam
steps (shared by tests/golden/make_golden_optim_edge.py,
test_oracle_golden_optim_edge.py and test_gpu_optim_edge.py; not a test module).

Everything is drawn from synth.py's splitmix64 through ``edge_values.draws`` /
``edge_input`` (never numpy.random): the GPU side regenerates the same bits.

Optimizer run (``optim_run``): CALLS calls on one name.  Calls 0-1 touch the
index set A, calls 2-3 the set B that shares half of A (state re-used after
gaps of 1 and 2 iterations).  The gradient of call ``it`` is
``edge_input(kind, K, bucket, it)`` in stream order, so ``nan_steady`` has NaNs
from call 2 on.  The parameter is ``synth * 1000`` (itself wide-exponent for
the ``wide_exp`` kind) with +-inf, -0.0, subnormals and +-FLT_MAX planted among
the touched indices.

amsgrad plants (``AMS_PLANTS``, stream position matters):
    ams_inf_mid     call 0, position 1024 + 511: a gradient of 2e19, so vt is
                    finite and (float)vt_hat = inf; before it elements move,
                    behind it num / inf = 0 and they do not
    ams_nan_ends    a NaN gradient at position 0 and at the last position
    ams_carry       call 0 a thousand times larger than the later calls: every
                    later call's vt_hat stays below the carried-in vmax
    ams_subnormal   every gradient about 1e-20: vmax a nonzero subnormal

MERGE plants (``merge_planted``): n = 4099, per_rank = 400, half the indices
shared by every rank (make_golden_merge.rank_streams).  Shared index s holds,
rank by rank: 0 (+inf, finite...), 1 (+inf, -inf, finite...), 2 (3e38, 3e38,
finite...), 3 a subnormal on every rank, 4 -0.0 on every rank; rank 0's first
own index holds 1e-38 (a subnormal whose quotient loses bits), rank 1's
FLT_MAX.  ``merge_kind`` fills every rank's values with one gradient kind.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

from edge_values import distinct, draws, edge_input
from stellatrain_amd.synth import seed_for, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_merge import rank_streams  # noqa: E402

GRAD_KINDS = ("inf", "huge", "denorm_half", "denorm_all", "negzero", "wide_exp", "nan_steady")
K = 2 * 1024 + 37       # three ADAM_TILE / win_emit1t tiles, the last one ragged
N = 8192 + 7
N16 = 60000             # where u16 wire indices are used
CALLS = 4
BUCKET = 61
NAN_CAP = 0.01          # NaN positions per compared array, as a share of the touched elements
FLT_MAX = np.float32(3.4028234663852886e38)
FLT_MIN = np.float32(1.1754943508222875e-38)

SGD_CFG = {
    "a": dict(lr=0.1, momentum=0.9),
    "b": dict(lr=0.1, momentum=0.9, nesterov=True, dampening=0.1, weight_decay=1e-4),
    "c": dict(lr=0.1, momentum=0.0, weight_decay=1e-4),
    "d": dict(lr=0.1, momentum=0.9, maximize=True),
    "e": dict(lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4, smart_momentum=True),
}
ADAM_CFG = {
    "a": dict(lr=1e-2),
    "b": dict(lr=1e-2, weight_decay=1e-2, maximize=True),
    "c": dict(lr=1e-2, amsgrad=True),
    "d": dict(lr=1e-2, eps=0.0),
    "e": dict(lr=1e-2, b1=0.5, b2=0.9, eps=1e-4),
}
AMS_PLANTS = ("ams_inf_mid", "ams_nan_ends", "ams_carry", "ams_subnormal")
AMS_POS = 1024 + 511
HUGE_KEEP = 4
EPS0_POS = np.array([5, 300, 1023, 1024, 1500, 2047, 2048, 2084])
EPS0_ZERO = (700, 2060)


def _cross(cfgs):
    """Every kind twice, every configuration two or three times."""
    c = sorted(cfgs)
    out = []
    for j, kind in enumerate(GRAD_KINDS):
        out.append((c[j % len(c)], kind))
        out.append((c[(j + 2) % len(c)], kind))
    return out


SGD_CASES = [dict(name=f"sgd_{c}_{k}", opt="sgd", cfg=c, kind=k, plant=None) for c, k in _cross(SGD_CFG)]
ADAM_CASES = [dict(name=f"adam_{c}_{k}", opt="adam", cfg=c, kind=k, plant=None) for c, k in _cross(ADAM_CFG)]
AMS_CASES = [dict(name=p, opt="adam", cfg="c", kind="tame", plant=p) for p in AMS_PLANTS]
OPT_CASES = SGD_CASES + ADAM_CASES + AMS_CASES
WHOLE = ("sgd_e_negzero", "adam_c_inf", "ams_inf_mid", "adam_d_denorm_all")  # cases stored as whole arrays
assert set(WHOLE) <= {c["name"] for c in OPT_CASES}


def case_by_name(name):
    return next(c for c in OPT_CASES if c["name"] == name)


def cfg_of(case):
    return dict((SGD_CFG if case["opt"] == "sgd" else ADAM_CFG)[case["cfg"]])


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def index_sets(n: int, k: int = K, salt: str = "idx"):
    """(A, B): k distinct indices each in draw order, B = the second half of A
    and k - k // 2 ... fresh ones."""
    p = distinct(draws(salt, BUCKET, n, 8 * k), n, k + k // 2).astype(np.uint32)
    return p[:k].copy(), p[k // 2:k // 2 + k].copy()


def optim_run(case, n: int = N, k: int = K):
    """(param0, [(idx, grad)] * CALLS) of an optimizer case."""
    kind, plant = case["kind"], case["plant"]
    A, B = index_sets(n, k)
    seed = sum(case["name"].encode()) % 97
    if kind == "wide_exp":
        param = edge_input("wide_exp", n, BUCKET + 1, seed)
    else:
        param = synth(n, seed_for(BUCKET + 1, seed)) * np.float32(1000.0)
    if plant == "ams_subnormal":  # steps of 1e-14 must show
        param = (synth(n, seed_for(BUCKET + 1, seed)).astype(np.float64) * 1e-8).astype(np.float32)
    if plant is None:  # the amsgrad plants keep a tame parameter: one inf would hide the planted one
        param[A[3]] = np.inf
        param[A[k // 2 + 5]] = -np.inf       # in A and in B
        param[A[10]] = np.float32(-0.0)
        param[A[k - 3]] = np.float32(1e-40)
        param[B[k - 2]] = np.float32(-3e-41)  # B only
        param[A[1030]] = FLT_MAX
        param[A[k // 2 + 50]] = -FLT_MAX
    calls = []
    for it in range(CALLS):
        idx = A if it < 2 else B
        if plant is None:
            g = edge_input(kind, k, BUCKET, 100 * seed + it)
            if kind == "huge":  # 64 values of +-3e38 a call turn 5 % of the state into inf - inf: keep four
                big = np.flatnonzero(np.abs(g) == np.float32(3e38))
                g[big[HUGE_KEEP:]] = synth(k, seed_for(BUCKET, 100 * seed + it))[big[HUGE_KEEP:]]
            if kind == "denorm_all" and case["opt"] == "adam" and case["cfg"] == "d":
                # eps = 0: every denormal gradient is an x / 0 = inf, and inf - inf a call later (a third of
                # the parameter NaN).  Keep eight denormals, over the three tiles, and +0.0 / -0.0 for 0 / 0.
                t = synth(k, seed_for(BUCKET, 100 * seed + it))
                t[EPS0_POS] = g[EPS0_POS]
                t[EPS0_ZERO[0]], t[EPS0_ZERO[1]] = np.float32(0.0), np.float32(-0.0)
                g = t
            elif case["opt"] == "adam" and case["cfg"] == "d":
                g = thin_for_eps0(g, it)
        else:
            g = synth(k, seed_for(BUCKET, 100 * seed + it)) * np.float32(100.0)
            if plant == "ams_inf_mid" and it == 0:
                g[AMS_POS] = np.float32(2e19)
            elif plant == "ams_nan_ends":
                g[0] = np.uint32(0xFFC00001).view(np.float32)
                g[k - 1] = np.uint32(0x7FD2345F).view(np.float32)
            elif plant == "ams_carry":
                g = g * np.float32(1000.0 if it == 0 else 1e-3)
            elif plant == "ams_subnormal":
                g = (g.astype(np.float64) * 1e-19).astype(np.float32)
        calls.append((idx.copy(), np.ascontiguousarray(g, np.float32)))
    return np.ascontiguousarray(param, np.float32), calls


def thin_where(g: np.ndarray, mask: np.ndarray, it: int, keep: int) -> np.ndarray:
    """g with the masked values past the first `keep` replaced by tame ones."""
    g = g.copy()
    pos = np.flatnonzero(mask)
    g[pos[keep:]] = synth(g.size, seed_for(BUCKET + 3, it))[pos[keep:]]
    return g


def thin_for_eps0(g: np.ndarray, it: int, keep: int = 8) -> np.ndarray:
    """A gradient for Adam with eps = 0: a value whose square underflows to 0
    (|g| < 1e-18, zeros included) is an x / 0 or a 0 / 0, and inf - inf a call
    later.  The first `keep` stay."""
    with np.errstate(invalid="ignore"):
        return thin_where(g, np.abs(g) < np.float32(1e-18), it, keep)


def thin_for_fp16(g: np.ndarray, it: int) -> np.ndarray:
    """A gradient for the fp16 wire forms: of the values binary16 turns into inf
    (|g| >= 65520; half of a wide-exponent stream, which would leave a fifth of
    the state inf - inf) the first HUGE_KEEP stay, the others become tame."""
    with np.errstate(invalid="ignore"):
        return thin_where(g, np.isfinite(g) & (np.abs(g) >= np.float32(65520.0)), it, HUGE_KEEP)


def input_hashes(param, calls):
    return [sha(param)] + [sha(i) + ":" + sha(g) for i, g in calls]


# -- oracle side ------------------------------------------------------------
def oracle_new(oracle, case):
    cfg = cfg_of(case)
    return oracle.sgd_new(**cfg) if case["opt"] == "sgd" else oracle.adam_new(**cfg)


def oracle_free(oracle, case, h):
    (oracle.sgd_free if case["opt"] == "sgd" else oracle.adam_free)(h)


def oracle_step(oracle, case, h, name, param, g, idx):
    (oracle.sgd_apply if case["opt"] == "sgd" else oracle.adam_apply)(h, name, param, g, idx)


def oracle_state(oracle, case, h, name, n):
    """dict of what is compared after a call (besides the parameter)."""
    if case["opt"] == "sgd":
        cfg = cfg_of(case)
        out = {"iter": oracle.sgd_iter(h)}
        if cfg.get("momentum", 0.0) != 0.0:
            out["mom"] = oracle.sgd_momentum(h, name, n)
        if cfg.get("smart_momentum"):
            out["last"] = oracle.sgd_last(h, name, n)
        return out
    m, v, vmax, tick = oracle.adam_state(h, name, n)
    return {"m": m, "v": v, "vmax": np.float32(vmax), "tick": int(tick)}


def state_arrays(p, st):
    """The float arrays compared after a call: the parameter and mom / m / v."""
    return [p] + [st[f] for f in ("mom", "m", "v") if st.get(f) is not None]


def nan_share(arrays, touched: int) -> float:
    return max((int(np.isnan(a).sum()) for a in arrays), default=0) / max(touched, 1)


def run_oracle(oracle, case, n: int = N, k: int = K):
    """(param0, calls, [(param, state)] after every call)."""
    param0, calls = optim_run(case, n, k)
    h = oracle_new(oracle, case)
    p = param0.copy()
    out = []
    for idx, g in calls:
        oracle_step(oracle, case, h, "w", p, g, idx)
        st = oracle_state(oracle, case, h, "w", n)
        out.append((p.copy(), st))
    oracle_free(oracle, case, h)
    return param0, calls, out


def stats(case, param0, calls, results):
    """What the case exercised, from the (reference or oracle) results."""
    n = param0.size
    s = {"nan_share": 0.0}
    seen = np.zeros(n, bool)
    prev = param0
    s["moved"] = []
    for (idx, g), (p, st) in zip(calls, results):
        seen[idx] = True
        s["nan_share"] = max(s["nan_share"], nan_share(state_arrays(p, st), int(seen.sum())))
        s["moved"].append(int((p.view(np.uint32) != prev.view(np.uint32)).sum()))
        prev = p
    p, st = results[-1]
    fin = np.isfinite(p)
    if case["opt"] == "adam":
        v = st["v"]
        s["subnormal_v"] = int(((v > 0) & (v < FLT_MIN)).sum())
        m = np.abs(st["m"])
        s["subnormal_m_zero_v"] = int(((m > 0) & (m < FLT_MIN) & (v == 0)).sum())  # g * g underflowed to 0
        s["inf_param"] = int(np.isinf(p).sum())
        s["inf_v_finite_param"] = int((np.isinf(v) & fin).sum())
        s["vmax_bits"] = int(np.float32(st["vmax"]).view(np.uint32))
        s["vmax_calls"] = [int(np.float32(r[1]["vmax"]).view(np.uint32)) for r in results]
    else:
        mom = st.get("mom")
        if mom is not None:
            s["subnormal_mom"] = int(((np.abs(mom) > 0) & (np.abs(mom) < FLT_MIN)).sum())
            s["inf_mom"] = int(np.isinf(mom).sum())
            s["big_mom"] = int((np.abs(mom) > np.float32(1e38)).sum())  # inf included
        s["inf_param"] = int(np.isinf(p).sum())
    s["nan_param"] = int(np.isnan(p).sum())
    s["negzero_param"] = int((p.view(np.uint32) == 0x80000000).sum())
    s["subnormal_param"] = int(((np.abs(p) > 0) & (np.abs(p) < FLT_MIN)).sum())
    if case["plant"] == "ams_inf_mid":
        idx0 = calls[0][0]
        p0 = results[0][0]
        ch = p0[idx0].view(np.uint32) != param0[idx0].view(np.uint32)
        s["moved_before_plant"] = int(ch[:AMS_POS].sum())
        s["moved_from_plant"] = int(ch[AMS_POS:].sum())
    return s


def check_stats(case, s):
    """The edge a case is named for occurred."""
    assert s["nan_share"] <= NAN_CAP, (case["name"], s["nan_share"])
    kind, plant = case["kind"], case["plant"]
    if plant is None and not (case["opt"] == "adam" and case["cfg"] == "c"):  # an inf vmax freezes amsgrad
        assert all(m > 0 for m in s["moved"]), s["moved"]
    if case["opt"] == "adam":
        if kind == "wide_exp" or plant == "ams_subnormal":
            assert s["subnormal_v"] > 0
        if kind in ("denorm_all", "denorm_half"):
            assert s["subnormal_m_zero_v"] > 0
        if kind == "denorm_all" and case["cfg"] == "d":
            assert s["inf_param"] > 2 and s["nan_param"] > 0  # eps = 0: x / 0 and 0 / 0
        if kind == "huge":
            assert s["inf_v_finite_param"] > 0
        if kind in ("inf", "huge") and case["cfg"] == "c":
            assert s["vmax_bits"] == 0x7F800000
        if plant == "ams_inf_mid":
            assert s["vmax_bits"] == 0x7F800000
            assert s["moved_before_plant"] >= AMS_POS - 8 and s["moved_from_plant"] == 0, s
            assert s["moved"][1:] == [0, 0, 0]  # vmax stays inf for good
        if plant == "ams_nan_ends":
            assert 0 < s["vmax_bits"] < 0x7F800000 and s["nan_param"] >= 2
        if plant == "ams_subnormal":
            assert 0 < s["vmax_bits"] < 0x00800000 and all(m > 2000 for m in s["moved"])
        if plant == "ams_carry":
            assert 0x00800000 <= s["vmax_bits"] < 0x7F800000
            # the carried-in vmax beat every vt_hat of calls 1-3, and they still moved
            assert len(set(s["vmax_calls"])) == 1 and all(m > 1000 for m in s["moved"])
    else:
        if kind == "inf" and case["cfg"] != "c":
            assert s["inf_mom"] > 0
        if kind == "huge" and case["cfg"] != "c":
            assert s["big_mom"] > 0
        if kind == "denorm_all" and case["cfg"] != "c":
            assert s["subnormal_mom"] > 0
        if kind == "inf":
            assert s["inf_param"] > 2  # beyond the two planted ones
    if kind == "nan_steady":
        assert s["nan_param"] >= 5


# -- MERGE plants -------------------------------------------------------------
MERGE_N, MERGE_PER_RANK = 4099, 400
MERGE_WORLDS = (2, 3, 5, 6, 7, 8)
MERGE_CASES = ([dict(name=f"merge_planted_w{w}", world=w, kind=None) for w in MERGE_WORLDS] +
               [dict(name=f"merge_{k}_w{MERGE_WORLDS[j % len(MERGE_WORLDS)]}",
                     world=MERGE_WORLDS[j % len(MERGE_WORLDS)], kind=k) for j, k in enumerate(GRAD_KINDS)])
MERGE_WHOLE = ("merge_planted_w3", "merge_planted_w7")
assert set(MERGE_WHOLE) <= {c["name"] for c in MERGE_CASES}


def merge_case_by_name(name):
    return next(c for c in MERGE_CASES if c["name"] == name)


def merge_case(case, n: int = MERGE_N, per_rank: int = MERGE_PER_RANK, plant: bool = True):
    """(idx, val) of the world streams back to back, and the planted indices
    (`plant=False`: the tame streams the plants go into)."""
    world = case["world"]
    seed = 50 + world + (0 if case["kind"] is None else 10 + GRAD_KINDS.index(case["kind"]))
    idx, val = rank_streams(n, per_rank, world, 4, False, seed)
    idx, val = idx.copy(), val.copy()
    plants = {}
    if case["kind"] is not None:
        for r in range(world):
            # nan_steady plants its NaNs from call 2 on: rank 0 alone gets them (five NaNs of 600 values)
            val[r * per_rank:(r + 1) * per_rank] = edge_input(case["kind"], per_rank, BUCKET + 2 + seed + r,
                                                              2 if r == 0 else 0)
        return idx, val, plants
    if not plant:
        return idx, val, plants
    h = per_rank // 2
    r0 = idx[:per_rank]
    shared = [int(i) for i in r0 if all(i in idx[r * per_rank:(r + 1) * per_rank] for r in (1, world - 1))]
    assert len(shared) == h
    own = [[int(i) for i in idx[r * per_rank:(r + 1) * per_rank] if int(i) not in set(shared)] for r in range(2)]

    def put(r, index, v):
        seg = idx[r * per_rank:(r + 1) * per_rank]
        pos = np.flatnonzero(seg == index)
        assert pos.size == 1
        val[r * per_rank + int(pos[0])] = np.float32(v)

    for r in range(world):
        put(r, shared[0], np.inf if r == 0 else 1.5 + r)
        put(r, shared[1], np.inf if r == 0 else (-np.inf if r == 1 else 2.5))
        put(r, shared[2], 3e38 if r < 2 else 1.0)
        put(r, shared[3], 1e-40 * (r + 1))
        put(r, shared[4], -0.0)
    put(0, own[0][0], 1e-38)
    put(1, own[1][0], FLT_MAX)
    plants = {"inf_finite": shared[0], "inf_minus_inf": shared[1], "overflow": shared[2], "subnormal": shared[3],
              "negzero": shared[4], "subnormal_quotient": own[0][0], "flt_max": own[1][0]}
    return idx, val, plants


def merge_check_stats(case, plants, out_idx, out_val):
    """The merged values hold what the plants are for."""
    out_idx, out_val = np.asarray(out_idx, np.uint32), np.asarray(out_val, np.float32)
    assert np.isnan(out_val).sum() <= max(1, int(NAN_CAP * out_val.size)), case["name"]
    if case["kind"] is not None:
        return
    at = lambda k: out_val[np.flatnonzero(out_idx == plants[k])[0]]  # noqa: E731
    w = np.float32(case["world"])
    assert at("inf_finite") == np.inf
    assert np.isnan(at("inf_minus_inf"))
    assert at("overflow") == np.inf
    assert 0 < at("subnormal") < FLT_MIN
    assert at("negzero").view(np.uint32) == 0  # zeros + -0.0 = +0.0
    assert 0 < at("subnormal_quotient") < FLT_MIN and at("subnormal_quotient") == np.float32(1e-38) / w
    assert at("flt_max") == FLT_MAX / w
