"""CPU-only checks of the gather-add from bf16 / fp16 sources
(``stg_gather_add_typed_device``, ``stg_merge_gather_compress_typed_device``,
``stg_merge_send_batch_typed_device``): the C-ABI declarations and their
binding, ``stg_grad_src_t``'s layout, the launch plan the typed gather takes for
every pointer phase (``stg_debug_gather_plan``, host arithmetic), and the
Python argument checks that need no device."""
from __future__ import annotations

import ctypes as C
import re

import pytest

NEW = ["stg_gather_add_typed_device", "stg_merge_gather_compress_typed_device", "stg_merge_send_batch_typed_device",
       "stg_debug_gather_plan"]
F32, BF16, F16 = 0, 1, 2


def test_header_declares_the_entry_points_and_the_struct():
    from stellatrain_amd._capi import HEADER, header_symbols
    syms = header_symbols()
    for s in NEW:
        assert s in syms, s
    txt = open(HEADER).read()
    assert "typedef struct stg_grad_src" in txt and "stg_grad_src_t" in txt


def test_python_binds_the_entry_points_and_the_library_exports_them():
    from stellatrain_amd._capi import _SIGS, StgGradSrc, StgSendTask, lib
    L = lib()
    for s in NEW:
        assert s in _SIGS and hasattr(L, s), s
    assert _SIGS[NEW[0]] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(StgGradSrc), C.c_int, C.c_uint64, C.c_int,
                                       C.c_void_p])
    assert _SIGS[NEW[2]] == (C.c_int, [C.c_void_p, C.POINTER(StgSendTask), C.POINTER(C.POINTER(StgGradSrc)),
                                       C.c_size_t, C.c_void_p])


def test_struct_layout_matches_the_header():
    from stellatrain_amd._capi import HEADER, StgGradSrc as G
    txt = " ".join(open(HEADER).read().split())
    m = re.search(r"\} stg_grad_src_t; /\* (\d+) bytes on LP64: d_grad at (\d+), dtype at (\d+)", txt)
    assert m and tuple(map(int, m.groups())) == (16, 0, 8) == (C.sizeof(G), G.d_grad.offset, G.dtype.offset)
    import stellatrain_amd
    assert stellatrain_amd.StgGradSrc is G


def plan(addrs, dtypes, n):
    from stellatrain_amd._capi import lib
    a = (C.c_uint64 * len(addrs))(*addrs)
    d = (C.c_int * len(dtypes))(*dtypes)
    w, h = C.c_uint32(77), C.c_uint32(77)
    assert lib().stg_debug_gather_plan(a, d, len(addrs), n, C.byref(w), C.byref(h)) == 0
    return w.value, h.value


def _aligned(addr, dt, head, width):
    """After `head` elements: an fp32 stream on 16 bytes, a 16-bit stream on 2 * width bytes."""
    return (addr + 4 * head) % 16 == 0 if dt == F32 else (addr + 2 * head) % (2 * width) == 0


def _common_head(addrs, dtypes, width):
    for h in range(width):
        if all(_aligned(a, d, h, width) for a, d in zip(addrs, dtypes)):
            return h
    return None


@pytest.mark.parametrize("dt16", [BF16, F16])
def test_plan_every_phase_of_one_fp32_and_one_16bit_stream(dt16):
    """fp32 phase 0..3 (elements past a 16-byte boundary) x 16-bit phase 0..7,
    n = 0..40: the head aligns both streams, head <= n, 8-wide where an 8-phase
    exists, else 4-wide where a 4-phase exists, width 0 exactly when no head
    aligns both."""
    base32, base16 = 0x7f0000100000, 0x7f0000200000
    seen = set()
    for p32 in range(4):
        for p16 in range(8):
            addrs, dts = [base32 + 4 * p32, base16 + 2 * p16], [F32, dt16]
            h8, h4 = _common_head(addrs, dts, 8), _common_head(addrs, dts, 4)
            for n in range(41):
                w, h = plan(addrs, dts, n)
                what = (p32, p16, n, w, h)
                if h8 is not None:
                    assert (w, h) == (8, min(h8, n)), what
                elif h4 is not None:
                    assert (w, h) == (4, min(h4, n)), what
                else:
                    assert (w, h) == (0, 0), what
                assert h <= n, what
                if w and h < n:
                    assert all(_aligned(a, d, h, w) for a, d in zip(addrs, dts)), what
                assert (w == 0) == (h4 is None), what  # (an 8-phase is a 4-phase too)
                seen.add(w)
    # (with one 16-bit stream a 4-phase always extends to an 8-phase; 4-wide needs two, test_plan_examples)
    assert seen == {0, 8}


def test_plan_examples():
    b = 0x7f0000100000
    assert plan([b, b, b], [F32, F32, BF16], 100) == (8, 0)
    assert plan([b + 4, b + 4, b + 2], [F32, F32, F16], 100) == (8, 7)   # 7 floats to 32 bytes, 7 halves + 2 to 16
    assert plan([b, b + 8], [F32, BF16], 100) == (8, 4)
    assert plan([b, b, b + 8], [F32, BF16, F16], 100) == (4, 0)           # 16-bit streams 8 bytes apart in phase
    assert plan([b + 8, b + 4, b + 12], [F32, BF16, F16], 100) == (4, 2)
    assert plan([b, b + 2], [F32, BF16], 100) == (0, 0)                   # no head serves both
    assert plan([b + 4, b + 4], [F32, F32], 2) == (8, 2)                  # shorter than its head: all head
    assert plan([b + 2], [F32], 100) == (0, 0)                            # not even element aligned
    assert plan([b + 6, b + 6 + 1024], [BF16, F16], 9) == (8, 5)


def test_plan_refuses_bad_arguments():
    from stellatrain_amd._capi import lib
    L = lib()
    w, h = C.c_uint32(), C.c_uint32()
    a, d = (C.c_uint64 * 1)(64), (C.c_int * 1)(3)
    assert L.stg_debug_gather_plan(a, d, 1, 8, C.byref(w), C.byref(h)) == -1 and b"dtype" in L.stg_last_error()
    d[0] = 0
    assert L.stg_debug_gather_plan(a, d, 0, 8, C.byref(w), C.byref(h)) == -1
    assert L.stg_debug_gather_plan(a, d, 19, 8, C.byref(w), C.byref(h)) == -1
    assert L.stg_debug_gather_plan(None, d, 1, 8, C.byref(w), C.byref(h)) == -1
    assert L.stg_debug_gather_plan(a, d, 1, 8, None, C.byref(h)) == -1


def test_python_refusals_without_a_device():
    import torch
    from stellatrain_amd import SendTasks, gather_add
    from stellatrain_amd.compressor import typed_sources
    n = 32
    f, b, h = (torch.zeros(n, dtype=t) for t in (torch.float32, torch.bfloat16, torch.float16))
    with pytest.raises(ValueError, match="grads\\[0\\] needs a float32 bucket"):
        gather_add([b, f], None, 0)
    with pytest.raises(ValueError, match="grads\\[0\\] needs a float32 bucket"):
        gather_add([h, h], f, 1)
    with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
        gather_add([f, h, torch.zeros(n, dtype=torch.float64)], None, 0)
    with pytest.raises(ValueError, match="float32 residual and out"):
        gather_add([b, h], None, 0, out=torch.zeros(n, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="one size"):
        gather_add([f, h[:8]], None, 0)
    # the fp32 call's own message is unchanged
    with pytest.raises(ValueError, match="contiguous float32 device tensors of one size"):
        gather_add([f, f], None, 0)
    # typed_sources: None for fp32 in place, [0] null without a bucket, [0] typed with one
    assert typed_sources("t", [f, f], None) is None
    a = typed_sources("t", [f, b, h], None)
    assert [(x.d_grad, x.dtype) for x in a] == [(None, 0), (b.data_ptr(), 1), (h.data_ptr(), 2)]
    a = typed_sources("t", [h, f], f)
    assert [(x.d_grad, x.dtype) for x in a] == [(h.data_ptr(), 2), (f.data_ptr(), 0)]
    di, dv = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.float32)
    with pytest.raises(ValueError, match="item 0: a bfloat16 / float16 grads\\[0\\] needs a float32 bucket"):
        SendTasks([("k", [b, f], 4, di, dv, None, 0)], counts=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="item 0: float32 gradients and residual of one size"):
        SendTasks([("k", [f, b], 4, di, dv, h, 0)], counts=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="item 0: float32 gradients and residual of one size"):
        SendTasks([("k", [b, b], 4, di, dv, None, 0, 0, b)], counts=torch.zeros(1, dtype=torch.int32))
