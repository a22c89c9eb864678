"""CPU-only checks of the one-call MERGE send path
(``stg_merge_send_batch_device``): the C-ABI declarations and their Python
binding, the task structure's layout against the header's documented one, and
the argument checks that need no codec handle (a handle needs a HIP device;
the rest of the refusals are in tests/test_gpu_send_batch.py)."""
from __future__ import annotations

import ctypes as C
import re

import pytest

ENTRY = "stg_merge_send_batch_device"


def test_header_declares_the_entry_point_and_the_task():
    from stellatrain_amd._capi import HEADER, header_symbols
    assert ENTRY in header_symbols()
    txt = open(HEADER).read()
    assert "typedef struct stg_send_task" in txt and "stg_send_task_t" in txt


def test_python_binds_the_entry_point():
    from stellatrain_amd._capi import _SIGS, lib
    assert ENTRY in _SIGS and hasattr(lib(), ENTRY)


def test_task_layout_matches_the_header():
    """The size and offsets the header documents next to the struct are the
    ctypes structure's (and the LP64 layout of the C declaration)."""
    from stellatrain_amd._capi import HEADER, StgBucket as B, StgSendTask as T
    txt = " ".join(open(HEADER).read().split())
    m = re.search(r"\} stg_send_task_t; /\* (\d+) bytes on LP64: bucket at (\d+) \((\d+) bytes; its d_count at (\d+)\), "
                  r"d_residual at (\d+), d_grads at (\d+), num_gpus at (\d+), wire_flag at (\d+)", txt)
    assert m, "the header documents stg_send_task_t's layout"
    size, o_b, s_b, o_cnt, o_res, o_gr, o_ng, o_fl = map(int, m.groups())
    assert (size, o_b, s_b, o_cnt, o_res, o_gr, o_ng, o_fl) == (104, 0, 80, 72, 80, 88, 96, 100)
    assert C.sizeof(T) == size and C.sizeof(B) == s_b and B.d_count.offset == o_cnt
    assert (T.bucket.offset, T.d_residual.offset, T.d_grads.offset, T.num_gpus.offset, T.wire_flag.offset) == \
        (o_b, o_res, o_gr, o_ng, o_fl)


def test_null_handle_and_null_task_array_are_refused():
    from stellatrain_amd._capi import StgSendTask, lib
    L = lib()
    f = getattr(L, ENTRY)
    one = (StgSendTask * 1)()
    assert f(None, one, 1, None) == -1 and b"handle" in L.stg_last_error()
    assert f(None, None, 3, None) == -1
    assert f(None, None, 0, None) == -1  # (the handle is checked first; ntasks == 0 on a handle: the GPU tests)


def test_python_surface_exists_and_validates_without_a_device():
    import torch
    import stellatrain_amd as S
    assert callable(S.Compressor.merge_send_batch_async) and callable(S.CodecEngine.send_buckets)
    assert S.StgSendTask is not None
    assert S.SendTasks([]).count == 0
    g = torch.zeros(100)
    i16, i32, f32 = (torch.zeros(8, dtype=d) for d in (torch.int16, torch.int32, torch.float32))
    with pytest.raises(ValueError, match="item 0.*flag"):
        S.SendTasks([("a", [g], 8, i32, f32, None, 4)])
    with pytest.raises(ValueError, match="item 0.*dtypes"):
        S.SendTasks([("a", [g], 8, i32, f32, None, 1)])
    with pytest.raises(ValueError, match="item 0.*dtypes"):
        S.SendTasks([("a", [g], 8, i16, f32, None, 3)])
    with pytest.raises(ValueError, match="item 0.*one size"):
        S.SendTasks([("a", [g, torch.zeros(99)], 8, i32, f32, None, 0)])
    with pytest.raises(ValueError, match="item 0.*1..16"):
        S.SendTasks([("a", [g] * 17, 8, i32, f32, None, 0)])
    with pytest.raises(ValueError, match="item 0.*expected"):
        S.SendTasks([("a", [g], 8, i32, f32, None)])
    with pytest.raises(ValueError, match="item 0.*HIP device"):
        S.SendTasks([("a", [g], 8, i32, f32, None, 0)])  # host tensors never reach the C call
