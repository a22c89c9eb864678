"""The batched thresholdv16 scan gives the reference's streams at any grid.

The scan's workgroups take chunks dynamically, so its result must not depend
on how many there are (csrc/scan_grid.h sizes the grid by the streams in
use).  The grid is read once per process (STG_DEBUG_TV16_GRID), so each value
runs in a fresh child (tests/scan_grid_child.py: six AIMD calls of a
three-bucket launch of 198 chunks, both regimes, compared bit-exactly with
the oracle):

  1    one workgroup takes every chunk in order;
  8    a few workgroups, each taking chunk after chunk;
  512  one chunk per workgroup, all in flight at once, so the finishers'
       look-backs poll aggregates that are not published yet; the other 314
       workgroups find the chunk counter exhausted and leave.

The children run one after the other; the first that does not exit 0 ends
the test, and none is tried again.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_scan_grids(gpu):
    out = {}
    for grid in (1, 8, 512):
        env = dict(os.environ, STG_DEBUG_TV16_GRID=str(grid), STG_DEBUG_TV16_COUNT="1")
        r = subprocess.run(["timeout", "-k", "10", "100", sys.executable, os.path.join(HERE, "scan_grid_child.py")],
                           capture_output=True, text=True, env=env)
        assert r.returncode == 0, (grid, r.returncode, r.stderr[-4000:])
        out[grid] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        print(out[grid])
    for grid in (1, 8, 512):
        assert out[grid]["ok"] and out[grid]["launches"] == out[grid]["calls"], out[grid]
    # no workgroup of a grid within the chunk count leaves without a chunk
    assert out[1]["dead"] == 0 and out[8]["dead"] == 0, out
    # ... and of 512 exactly those past the chunk count do
    assert out[512]["dead"] == out[512]["calls"] * (512 - out[512]["chunks"]), out[512]
    assert out[512]["dead_max"] == 512 - out[512]["chunks"], out[512]
