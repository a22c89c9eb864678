#!/usr/bin/env python3
"""Generate tests/golden/golden_smart_sgd.npz from the REFERENCE sparse SGD itself,
with ``configure("smart_momentum", true)`` (optim/sgd.cpp:291-292).

Producer: the reference's optim/sgd.cpp compiled in place with the flags and
include paths of oracle/Makefile's _ref/libstg_ref_sgd.so rule
(-g -O3 -march=broadwell: no AVX-512, so the scalar loop sgd.cpp:221-260 runs,
asserts live).  oracle/ref_sgd_driver.cpp cannot set the option, so this script
writes a driver of its own into a temporary directory outside the repository,
builds a shared library there and loads it with ctypes.  Nothing compiled is
kept.

Every call's index set is duplicate-free: the reference asserts on a factor of
pow(m, 0) == 1 (sgd.cpp:229-232).

Stored per case (inputs included, so no random generator has to reproduce them):
    calls/name   name number of every optimize_raw call
    calls/len    its grad_len
    calls/smart  the option's value during the call
    idx, grad    the calls' indices / gradients, concatenated
    after        param[idx] after the call, concatenated (the reference writes
                 nowhere else; the generator checks that)
    <name>/param, <name>/mom, <name>/last   final parameter, buffer and
                 m_optim_state_last per name;  iter = m_iter at the end
The initial parameter of name number j is synth(n, seed_for(37, 90 + j)) * 1000.

    python tests/golden/make_golden_smart_sgd.py
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import platform
import shutil
import subprocess
import sys
import sysconfig
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.oracle import REF_SRC  # noqa: E402
from stellatrain_amd.synth import seed_for, synth  # noqa: E402

SEED_BUCKET = 37
REFFLAGS = "-std=c++17 -g -O3 -march=broadwell -fPIC -shared -D_GNU_SOURCE -w"

DRIVER = r"""
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <torch/extension.h>
#include <torch/torch.h>
#define private public
#include "optim/sgd.h"
#undef private
#define API extern "C" __attribute__((visibility("default")))
API void *sm_new(float lr, float momentum, float dampening, float weight_decay, int nesterov, int maximize) {
    auto *o = new SGD();
    std::string k;
    o->set_lr(lr);
    k = "momentum"; o->configure(k, momentum);
    k = "dampening"; o->configure(k, dampening);
    k = "weight_decay"; o->configure(k, weight_decay);
    k = "nestrov"; o->configure(k, (bool)nesterov);
    k = "maximize"; o->configure(k, (bool)maximize);
    return o;
}
API void sm_smart(void *o, int on) { std::string k = "smart_momentum"; static_cast<SGD *>(o)->configure(k, (bool)on); }
API void sm_free(void *o) { delete static_cast<SGD *>(o); }
API void sm_apply(void *o, const char *name, float *param, uint32_t param_len, float *g, uint32_t *gidx, uint32_t glen) {
    static_cast<SGD *>(o)->optimize_raw(param, param_len, name, g, gidx, glen);
}
API uint32_t sm_iter(void *o) { return static_cast<SGD *>(o)->m_iter; }
API int sm_state(void *o, const char *name, float *b, uint32_t *last, uint32_t len) {
    auto *s = static_cast<SGD *>(o);
    auto ib = s->m_optim_state_b.find(name);
    auto il = s->m_optim_state_last.find(name);
    if (ib == s->m_optim_state_b.end() || il == s->m_optim_state_last.end()) return -1;
    std::memcpy(b, ib->second.get(), sizeof(float) * len);
    std::memcpy(last, il->second.get(), sizeof(uint32_t) * len);
    return 0;
}
"""


def build_driver(tmp):
    import torch
    tdir = os.path.dirname(torch.__file__)
    src = os.path.join(tmp, "smart_sgd_driver.cpp")
    so = os.path.join(tmp, "libsmart_sgd_ref.so")
    with open(src, "w") as f:
        f.write(DRIVER)
    cmd = ["g++", *REFFLAGS.split(), f"-I{REF_SRC}", f"-I{tdir}/include", f"-I{tdir}/include/torch/csrc/api/include",
           f"-I{sysconfig.get_paths()['include']}", "-o", so, src, os.path.join(REF_SRC, "optim", "sgd.cpp"),
           f"-L{tdir}/lib", "-lc10", "-ltorch_cpu", f"-Wl,-rpath,{tdir}/lib"]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(so)
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
    lib.sm_new.restype = C.c_void_p
    lib.sm_new.argtypes = [C.c_float] * 4 + [C.c_int, C.c_int]
    lib.sm_smart.argtypes = [C.c_void_p, C.c_int]
    lib.sm_free.argtypes = [C.c_void_p]
    lib.sm_apply.argtypes = [C.c_void_p, C.c_char_p, f32p, C.c_uint32, f32p, u32p, C.c_uint32]
    lib.sm_iter.restype = C.c_uint32
    lib.sm_iter.argtypes = [C.c_void_p]
    lib.sm_state.restype = C.c_int
    lib.sm_state.argtypes = [C.c_void_p, C.c_char_p, f32p, u32p, C.c_uint32]
    return lib


def _groups(rng, n, ngroups, size):
    p = rng.permutation(n).astype(np.uint32)
    return [p[i * size:(i + 1) * size] for i in range(ngroups)]


def _mix(rng, *parts):
    a = np.concatenate(parts).astype(np.uint32)
    rng.shuffle(a)
    assert np.unique(a).size == a.size  # the reference aborts on a repeated index
    return a


# index groups of 10 per step: a group's gaps run from 1 to 4 iterations
OVERLAP6 = ["ABCD", "AEFG", "BEHA", "CFHB", "DGCA", "ABEH"]


def calls_overlap(rng, n, steps, name=0):
    g = dict(zip("ABCDEFGH", _groups(rng, n, 8, 10)))
    return [(name, _mix(rng, *[g[c] for c in s])) for s in steps]


def calls_two_names(rng, n0, n1):
    """Names 0 and 1 interleaved on one optimizer; name 1 first appears at
    m_iter = 3; call 2 has grad_len = 0."""
    g0 = dict(zip("ABCDEFGH", _groups(rng, n0, 8, 10)))
    g1 = dict(zip("ABCDEFGH", _groups(rng, n1, 8, 10)))
    plan = [(0, "ABCD"), (0, "AEFG"), (0, ""), (1, "ABCD"), (0, "BEHA"), (1, "AEFG"), (1, "BEHA"), (0, "CFHB"),
            (1, "DGCA")]
    out = []
    for nm, s in plan:
        g = g0 if nm == 0 else g1
        out.append((nm, _mix(rng, *[g[c] for c in s]) if s else np.zeros(0, np.uint32)))
    return out


def calls_long_gaps(rng, n):
    """m = 0.5: a set at iteration 0; its first half again at iteration 130
    (pow(0.5, 130) is a denormal float); all of it at iteration 152 (the second
    half's gap of 152 is past the last non-zero table entry, 149).  The calls
    between carry one gradient (of seven other indices in turn) or none."""
    p = rng.permutation(n).astype(np.uint32)
    S, other = p[:40], p[40:47]
    out = [(0, S.copy())]
    for it in range(1, 153):
        if it == 130:
            out.append((0, _mix(rng, S[:20])))
        elif it == 152:
            out.append((0, _mix(rng, S)))
        elif it % 3 == 0:
            out.append((0, np.zeros(0, np.uint32)))
        else:
            out.append((0, other[it % 7: it % 7 + 1].copy()))
    return out


def calls_wide(rng, n, k):
    p = rng.permutation(n).astype(np.uint32)
    return [(0, _mix(rng, p[:k])), (0, _mix(rng, p[k // 2: k // 2 + k])), (0, _mix(rng, p[:k]))]


def cases():
    plain = dict(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False)
    full = dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=1e-4, nesterov=True, maximize=True)
    rng = np.random.default_rng(20240)
    a = calls_overlap(rng, 4103, OVERLAP6)
    return [
        dict(name="a_overlap", opt=plain, lens=[4103], calls=a, smart_from=0),
        dict(name="b_all_options", opt=full, lens=[4103], calls=a, smart_from=0),
        dict(name="c_two_names", opt=dict(plain, nesterov=True), lens=[4103, 16411],
             calls=calls_two_names(rng, 4103, 16411), smart_from=0),
        dict(name="d_long_gaps", opt=dict(plain, momentum=0.5), lens=[4103], calls=calls_long_gaps(rng, 4103),
             smart_from=0),
        dict(name="e_wide", opt=plain, lens=[16411], calls=calls_wide(rng, 16411, 1500), smart_from=0),
        dict(name="f_enabled_mid_run", opt=plain, lens=[4103], calls=calls_overlap(rng, 4103, OVERLAP6[:4]),
             smart_from=2),
    ]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def gen(lib, out):
    meta = []
    for ci, c in enumerate(cases()):
        o = lib.sm_new(c["opt"]["lr"], c["opt"]["momentum"], c["opt"]["dampening"], c["opt"]["weight_decay"],
                       int(c["opt"]["nesterov"]), int(c["opt"]["maximize"]))
        names = [f"p{j}@weight" for j in range(len(c["lens"]))]
        params = [synth(n, seed_for(SEED_BUCKET, 90 + j)) * np.float32(1000.0) for j, n in enumerate(c["lens"])]
        after, grads, smart = [], [], []
        for s, (nm, idx) in enumerate(c["calls"]):
            on = s >= c["smart_from"]
            lib.sm_smart(o, int(on))
            g = synth(idx.size, seed_for(SEED_BUCKET, 1000 * ci + s)) * np.float32(100.0)
            before = params[nm].copy()
            lib.sm_apply(o, names[nm].encode(), params[nm], c["lens"][nm], g, np.ascontiguousarray(idx), idx.size)
            keep = np.ones(c["lens"][nm], bool)
            keep[idx] = False
            assert np.array_equal(before[keep].view(np.uint32), params[nm][keep].view(np.uint32))
            after.append(params[nm][idx])
            grads.append(g)
            smart.append(on)
        p = c["name"]
        out[f"{p}/calls/name"] = np.array([nm for nm, _ in c["calls"]], np.uint8)
        out[f"{p}/calls/len"] = np.array([i.size for _, i in c["calls"]], np.uint32)
        out[f"{p}/calls/smart"] = np.array(smart, np.uint8)
        out[f"{p}/idx"] = np.concatenate([i for _, i in c["calls"]]).astype(np.uint32)
        out[f"{p}/grad"] = np.concatenate(grads).astype(np.float32)
        out[f"{p}/after"] = np.concatenate(after).astype(np.float32)
        for j, n in enumerate(c["lens"]):
            b, last = np.zeros(n, np.float32), np.zeros(n, np.uint32)
            assert lib.sm_state(o, names[j].encode(), b, last, n) == 0
            out[f"{p}/{names[j]}/param"] = params[j]
            out[f"{p}/{names[j]}/mom"] = b
            out[f"{p}/{names[j]}/last"] = last
        it = int(lib.sm_iter(o))
        out[f"{p}/iter"] = np.array([it], np.uint32)
        meta.append({"name": p, **c["opt"], "names": names, "lens": c["lens"], "calls": len(c["calls"]),
                     "smart_from": c["smart_from"], "iter": it, "seed_bucket": SEED_BUCKET,
                     "param_init": "synth(n, seed_for(37, 90 + j)) * 1000 for name number j"})
        lib.sm_free(o)
    return meta


def main():
    tmp = tempfile.mkdtemp(prefix="smart_sgd_ref_")
    try:
        lib = build_driver(tmp)
        gxx = subprocess.run(["g++", "--version"], capture_output=True, text=True).stdout.splitlines()[0]
        manifest = {"producer": "reference backend/src/optim/sgd.cpp compiled in place with a driver that sets "
                                "smart_momentum (flags of oracle/Makefile's libstg_ref_sgd.so rule)",
                    "flags": REFFLAGS, "compiler": gxx, "host": platform.machine(),
                    "generator": "stellatrain_amd/synth.py (splitmix64 Irwin-Hall, SURVEY 8(c))"}
        out: dict[str, np.ndarray] = {}
        manifest["smart_sgd"] = gen(lib, out)
        manifest["sha256"] = {k: sha(v) for k, v in sorted(out.items())}
        np.savez_compressed(os.path.join(HERE, "golden_smart_sgd.npz"), **out)
        with open(os.path.join(HERE, "manifest_smart_sgd.json"), "w") as f:
            json.dump(manifest, f, indent=1)
        print("wrote", len(out), "arrays;", os.path.getsize(os.path.join(HERE, "golden_smart_sgd.npz")) >> 10, "KiB")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
