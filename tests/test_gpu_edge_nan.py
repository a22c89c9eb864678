"""GPU parity with NaNs in the gradient, in steady state (from a key's third
call on; a NaN in a first call is undefined in the reference, DESIGN.md
section 2): thresholdv16 one-bucket calls and a batched launch, threshold-v,
and the send path with a NaN born inside the gather.

Every case runs in a child process (edge_nan_child.py) under a time limit, so
that nothing a NaN key might keep running outlives the test.  The waits and
search loops of the fill, the crew, both one-bucket finishes and threshold-v
were read for exits a NaN could defeat before this file first ran: every spin
wait compares tags and gives up after 200 ms, and every search loop narrows an
integer interval whatever its float comparison says.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(case: str):
    r = subprocess.run([sys.executable, os.path.join(HERE, "edge_nan_child.py"), case],
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["ok"], out
    return out


@pytest.mark.parametrize("kind", ["nan_steady", "nan_tail_only"])
@pytest.mark.parametrize("n,k", [(4103, 40), (65541, 655)])
def test_thresholdv16_nan(gpu, kind, n, k):
    out = _child(f"tv16:{kind}:{n}:{k}")
    assert "A" in out["regimes"] and "B" in out["regimes"], out


def test_thresholdv16_nan_batch(gpu):
    _child("tv16_batch")


@pytest.mark.parametrize("kind", ["nan_steady", "nan_tail_only"])
def test_thresholdv_nan(gpu, kind):
    """k < cnt on a NaN call (asserted in the child from the oracle's count):
    the only case in which gmax, whose fold a NaN restarts, enters the next
    threshold."""
    _child(f"tv:{kind}:65541:655")


def test_send_nan_born_in_gather(gpu):
    _child("send")
