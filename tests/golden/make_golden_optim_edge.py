#!/usr/bin/env python3
"""Generate tests/golden/golden_optim_edge.npz and manifest_optim_edge.json:
the receiving side (sparse SGD, smart-momentum SGD, Adam, amsgrad, the MERGE
decompress) on the edge-valued inputs of tests/optim_edge.py.

Producers:
* SGD / Adam: oracle/_ref/libstg_ref_sgd.so and libstg_ref_adam.so -- the
  reference's optim/sgd.cpp and optim/adam.cpp compiled in place by
  oracle/Makefile (-g -O3 -march=broadwell, no NDEBUG: the assertions are live)
  behind oracle/ref_sgd_driver.cpp / ref_adam_driver.cpp.
* MERGE: ``torch_merge`` of make_golden_merge.py (torch's CPU kernels).

Stored per optimizer case: the sha256 of every regenerated input (checked first
by the tests), and after every call the sha256 of the parameter and of every
state array (NaNs mapped to 0x7fc00000 first: x86 and the GPU pick different
payloads for inf - inf and 0 / 0), vmax bits, tick / iter.  The cases of
``optim_edge.WHOLE`` / ``MERGE_WHOLE`` also store the touched elements of each
array after each call.  The maker asserts the 1 % NaN cap and every case's
``stats`` on the reference's output.

Both files are reproduced byte for byte by a second run (fixed zip timestamps,
sorted keys).

    python tests/golden/make_golden_optim_edge.py
"""
from __future__ import annotations

import ctypes as C
import io
import json
import os
import platform
import re
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import optim_edge as E  # noqa: E402
from make_golden_merge import torch_merge  # noqa: E402
from oracle.oracle import REF_SO, build  # noqa: E402
from parity import canon_nan  # noqa: E402

# the flags the reference was built with: oracle/Makefile's own line
REFFLAGS = re.search(r"^REFFLAGS\s*:=\s*(.+)$", open(os.path.join(ROOT, "oracle", "Makefile")).read(),
                     re.M).group(1).strip()
_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")


class Ref:
    """The surface of oracle.Oracle that optim_edge drives, on the reference."""

    def __init__(self):
        d = os.path.dirname(REF_SO)
        s = self.s = C.CDLL(os.path.join(d, "libstg_ref_sgd.so"))
        a = self.a = C.CDLL(os.path.join(d, "libstg_ref_adam.so"))
        s.ref_sgd_new.restype = C.c_void_p
        s.ref_sgd_new.argtypes = [C.c_float] * 4 + [C.c_int, C.c_int]
        s.ref_sgd_free.argtypes = [C.c_void_p]
        s.ref_sgd_apply.argtypes = [C.c_void_p, C.c_char_p, _f32p, C.c_uint32, _f32p, _u32p, C.c_uint32]
        s.ref_sgd_momentum.argtypes = [C.c_void_p, C.c_char_p, _f32p, C.c_uint32]
        s.ref_sgd_smart.argtypes = [C.c_void_p, C.c_int]
        s.ref_sgd_iter.restype = C.c_uint32
        s.ref_sgd_iter.argtypes = [C.c_void_p]
        s.ref_sgd_last.argtypes = [C.c_void_p, C.c_char_p, _u32p, C.c_uint32]
        a.ref_adam_new.restype = C.c_void_p
        a.ref_adam_new.argtypes = [C.c_float] * 5 + [C.c_int, C.c_int]
        a.ref_adam_free.argtypes = [C.c_void_p]
        a.ref_adam_apply.argtypes = [C.c_void_p, C.c_char_p, _f32p, C.c_uint32, _f32p, _u32p, C.c_uint32]
        a.ref_adam_state.argtypes = [C.c_void_p, C.c_char_p, _f32p, _f32p, C.c_uint32, C.POINTER(C.c_float)]

    def sgd_new(self, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False,
                smart_momentum=False):
        h = self.s.ref_sgd_new(lr, momentum, dampening, weight_decay, int(nesterov), int(maximize))
        self.s.ref_sgd_smart(h, int(smart_momentum))
        return h

    def sgd_free(self, h):
        self.s.ref_sgd_free(h)

    def sgd_apply(self, h, name, param, g, gidx):
        self.s.ref_sgd_apply(h, name.encode(), param, param.size, np.ascontiguousarray(g, np.float32).copy(),
                             np.ascontiguousarray(gidx, np.uint32).copy(), len(g))

    def sgd_iter(self, h):
        return int(self.s.ref_sgd_iter(h))

    def sgd_momentum(self, h, name, n):
        out = np.zeros(n, np.float32)
        return None if self.s.ref_sgd_momentum(h, name.encode(), out, n) else out

    def sgd_last(self, h, name, n):
        out = np.zeros(n, np.uint32)
        return None if self.s.ref_sgd_last(h, name.encode(), out, n) else out

    def adam_new(self, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False):
        return self.a.ref_adam_new(lr, b1, b2, eps, weight_decay, int(amsgrad), int(maximize))

    def adam_free(self, h):
        self.a.ref_adam_free(h)

    def adam_apply(self, h, name, param, g, gidx):
        self.a.ref_adam_apply(h, name.encode(), param, param.size, np.ascontiguousarray(g, np.float32).copy(),
                              np.ascontiguousarray(gidx, np.uint32).copy(), len(g))

    def adam_state(self, h, name, n):
        m, v, vmax = np.zeros(n, np.float32), np.zeros(n, np.float32), C.c_float()
        tick = self.a.ref_adam_state(h, name.encode(), m, v, n, C.byref(vmax))
        return None if tick < 0 else (m, v, np.float32(vmax.value), tick)


def state_record(p, st):
    """The manifest's record of one call's result (hashes after the NaN mapping)."""
    rec = {"param": E.sha(canon_nan(p))}
    for f in ("mom", "m", "v"):
        if f in st:
            rec[f] = E.sha(canon_nan(st[f]))
    if "last" in st:
        rec["last"] = E.sha(st["last"])
    if "vmax" in st:
        rec["vmax_bits"] = int(canon_nan(np.array([st["vmax"]], np.float32))[0])
        rec["tick"] = st["tick"]
    if "iter" in st:
        rec["iter"] = st["iter"]
    return rec


def gen_optim(ref, out):
    meta = []
    for case in E.OPT_CASES:
        param0, calls, results = E.run_oracle(ref, case)
        # the reference writes nowhere but at the call's indices
        prev = param0
        for (idx, g), (p, st) in zip(calls, results):
            keep = np.ones(param0.size, bool)
            keep[idx] = False
            assert np.array_equal(prev.view(np.uint32)[keep], p.view(np.uint32)[keep])
            prev = p
        s = E.stats(case, param0, calls, results)
        E.check_stats(case, s)
        rec = {"name": case["name"], "opt": case["opt"], "cfg": case["cfg"], "kind": case["kind"],
               "plant": case["plant"], "options": E.cfg_of(case), "n": int(param0.size), "k": int(calls[0][0].size),
               "inputs": E.input_hashes(param0, calls), "calls": [state_record(p, st) for p, st in results],
               "stats": s}
        if case["name"] in E.WHOLE:
            for it, ((idx, g), (p, st)) in enumerate(zip(calls, results)):
                out[f"{case['name']}/it{it}/param"] = canon_nan(p[idx])
                for f in ("mom", "m", "v"):
                    if f in st:
                        out[f"{case['name']}/it{it}/{f}"] = canon_nan(st[f][idx])
                if "last" in st:
                    out[f"{case['name']}/it{it}/last"] = st["last"][idx]
        meta.append(rec)
        print(case["name"], "nan share %.4f" % s["nan_share"], "moved", s["moved"])
    return meta


def gen_merge(out):
    meta = []
    for case in E.MERGE_CASES:
        idx, val, plants = E.merge_case(case)
        ui, uv = torch_merge(idx, val, E.MERGE_PER_RANK, case["world"], E.MERGE_N)
        E.merge_check_stats(case, plants, ui, uv)
        if case["name"] in E.MERGE_WHOLE:
            out[f"{case['name']}/idx"] = ui
            out[f"{case['name']}/val"] = canon_nan(uv)
        meta.append({"name": case["name"], "world": case["world"], "kind": case["kind"], "n": E.MERGE_N,
                     "per_rank": E.MERGE_PER_RANK, "inputs": E.sha(idx) + ":" + E.sha(val), "plants": plants,
                     "union": int(ui.size), "nans": int(np.isnan(uv).sum()),
                     "sha256": E.sha(ui) + ":" + E.sha(canon_nan(uv))})
        print(case["name"], ui.size, "nans", int(np.isnan(uv).sum()))
    return meta


def save_npz(path, arrays):
    """np.savez_compressed with fixed timestamps: the same bytes on every run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def main():
    import torch
    torch.set_num_threads(1)
    build(ref=True)
    assert set(E.WHOLE) <= {c["name"] for c in E.OPT_CASES} and set(E.MERGE_WHOLE) <= {c["name"] for c in E.MERGE_CASES}
    ref = Ref()
    out: dict[str, np.ndarray] = {}
    gxx = subprocess.run(["g++", "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    manifest = {"producer": "reference backend/src/optim/sgd.cpp and adam.cpp compiled in place by oracle/Makefile "
                            "(libstg_ref_sgd.so, libstg_ref_adam.so); MERGE: torch CPU ops of cpu_optimize.cpp:40-72, "
                            "torch " + torch.__version__,
                "flags": REFFLAGS, "compiler": gxx, "host": platform.machine(),
                "nan_rule": "hashes and stored float arrays are uint32 bit patterns with every NaN mapped to 0x7fc00000",
                "nan_cap": E.NAN_CAP}
    manifest["optim"] = gen_optim(ref, out)
    manifest["merge"] = gen_merge(out)
    manifest["sha256"] = {k: E.sha(v) for k, v in sorted(out.items())}
    npz = os.path.join(HERE, "golden_optim_edge.npz")
    save_npz(npz, out)
    with open(os.path.join(HERE, "manifest_optim_edge.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", len(out), "arrays;", os.path.getsize(npz) >> 10, "KiB")


if __name__ == "__main__":
    main()
