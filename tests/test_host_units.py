"""The host layer's building blocks on a CPU: the owning device buffer
(csrc/devbuf.h) and the batched-launch table packer (csrc/batch_pack.h),
driven by tests/cpp/host_units.cpp against a fake allocator.  A plain
executable built with the address and undefined-behaviour sanitizers; no HIP
library is linked and nothing is preloaded."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_and_packer_under_sanitizers(tmp_path):
    exe = tmp_path / "host_units"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        "-I" + os.path.join(rocm, "include"), "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tests", "cpp", "host_units.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_units: ok" in r.stdout
