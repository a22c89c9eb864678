"""Loader of tests/golden/golden_smart_sgd.npz (made by
tests/golden/make_golden_smart_sgd.py from the reference's own optim/sgd.cpp
with smart_momentum on): the calls of a case, and the parameter the reference
left after each of them."""
from __future__ import annotations

import json
import os

import numpy as np

from stellatrain_amd.synth import seed_for, synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NPZ = os.path.join(GOLD, "golden_smart_sgd.npz")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest_smart_sgd.json")))
CASES = MANIFEST["smart_sgd"]

_arr = None


def arrays():
    global _arr
    if _arr is None:
        with np.load(NPZ) as z:
            _arr = {k: z[k] for k in z.files}
    return _arr


def case_by_name(name):
    return next(c for c in CASES if c["name"].startswith(name))


def opts(case):
    return {k: case[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize")}


def initial_params(case):
    return [synth(n, seed_for(case["seed_bucket"], 90 + j)) * np.float32(1000.0) for j, n in enumerate(case["lens"])]


def calls(case):
    """(name number, smart option, idx uint32, grad float32, param[idx] after the call) per call."""
    a, p = arrays(), case["name"]
    lens = a[f"{p}/calls/len"]
    off = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
    out = []
    for s in range(case["calls"]):
        sl = slice(int(off[s]), int(off[s + 1]))
        out.append((int(a[f"{p}/calls/name"][s]), bool(a[f"{p}/calls/smart"][s]), a[f"{p}/idx"][sl],
                    a[f"{p}/grad"][sl], a[f"{p}/after"][sl]))
    return out


def final_state(case, j):
    """(param, momentum buffer, last) of name number j after the last call."""
    a, p, nm = arrays(), case["name"], case["names"][j]
    return a[f"{p}/{nm}/param"], a[f"{p}/{nm}/mom"], a[f"{p}/{nm}/last"]
