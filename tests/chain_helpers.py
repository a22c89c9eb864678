"""Helpers shared by the GPU parity tests that walk a key through a send /
merge / publish chain (test infrastructure; not a test module)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from parity import fbits


def u(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.itemsize == 2 else a.view(np.uint32)


def state_bits(s):
    return [fbits(v) for v in s]


def debug_words(comp, gpu):
    import torch
    from stellatrain_amd._capi import check, lib
    w = (C.c_uint32 * 64)()
    check(lib().stg_codec_debug_words(comp._h, C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream), w, 64))
    return list(w)


def oracle_send(oracle, ho, key, srcs, resid, k, flag):
    """gather_add -> tv16_compress -> error feedback -> wire_encode."""
    x = srcs[0].copy()
    for r in range(len(srcs)):
        oracle.gather_add([x] + srcs[1:], resid, r)
    co, io, vo = oracle.tv16_compress(ho, key, x, k)
    wi, wv = oracle.wire_encode(io[:co], vo[:co], flag)
    x[io[:k]] = 0
    return x, co, wi, wv


OPTS = {"sgd": dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=0.01, smart_momentum=True),
        "adam": dict(lr=0.01, weight_decay=0.01)}


class Optim:
    """A device optimizer and its oracle twin over named parameters."""

    def __init__(self, oracle, kind):
        from stellatrain_amd import SparseAdam, SparseSGD
        self.oracle, self.kind = oracle, kind
        self.dev = (SparseSGD if kind == "sgd" else SparseAdam)(**OPTS[kind])
        self.h = oracle.sgd_new(**OPTS[kind]) if kind == "sgd" else oracle.adam_new(**OPTS[kind])

    def apply_oracle(self, name, po, ev, ei):
        (self.oracle.sgd_apply if self.kind == "sgd" else self.oracle.adam_apply)(self.h, name, po, ev, ei)

    def compare(self, name, pd, po, what):
        n, o = po.size, self.oracle
        assert np.array_equal(u(pd.cpu().numpy()), u(po)), "parameter: " + what
        if self.kind == "sgd":
            assert np.array_equal(u(self.dev.momentum_buffer(name, n)), u(o.sgd_momentum(self.h, name, n))), \
                "momentum: " + what
            assert np.array_equal(self.dev.last_buffer(name, n), o.sgd_last(self.h, name, n)), "last touched: " + what
            assert self.dev.iteration == o.sgd_iter(self.h), what
        else:
            sd, so = self.dev.state(name, n), o.adam_state(self.h, name, n)
            assert np.array_equal(u(sd[0]), u(so[0])), "m: " + what
            assert np.array_equal(u(sd[1]), u(so[1])), "v: " + what
            assert sd[3] == so[3], "tick: " + what

    def check(self):
        self.dev.check() if self.kind == "sgd" else self.dev.check_device()

    def close(self):
        (self.oracle.sgd_free if self.kind == "sgd" else self.oracle.adam_free)(self.h)


def merged(out):
    oi, ov, cnt = out
    c = int(cnt.cpu().numpy().view(np.uint32)[0])
    assert c != 0xffffffff and c <= oi.numel()
    i, v = oi.cpu().numpy().view(np.uint32)[:c], ov.cpu().numpy().view(np.uint32)[:c]
    o = np.argsort(i, kind="stable")
    return i[o], v[o]
