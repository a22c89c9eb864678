"""CPU-only checks of the parameter publish (``stg_param_publish_batch_device``,
``PublishTasks`` / ``publish_params``): the C-ABI declarations and their
binding, the structs' layout, how tasks share launches
(``stg_debug_publish_launches``, host arithmetic), the all-or-nothing argument
checks, which run before any device call, and the numpy model of the 16-bit
conversions that tests/test_gpu_publish.py measures the kernel against."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import publish_cases as P

NEW = ["stg_param_publish_batch_device", "stg_debug_publish_launches"]
_WS_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stellatrain_amd", "csrc", "ws.h")
T = int(re.search(r"constexpr uint32_t PUBLISH_TILE = (\d+);", open(_WS_H).read()).group(1))
PER_CU = int(re.search(r"constexpr uint32_t PUBLISH_GRID_PER_CU = (\d+);", open(_WS_H).read()).group(1))


def test_header_declares_the_entry_points_and_the_structs():
    from stellatrain_amd._capi import HEADER, header_symbols
    syms = header_symbols()
    for s in NEW:
        assert s in syms, s
    txt = open(HEADER).read()
    assert "typedef struct stg_publish_task" in txt and "stg_publish_task_t" in txt
    assert "typedef struct stg_replica" in txt and "stg_replica_t" in txt
    for name, v in (("STG_DT_F32", 0), ("STG_DT_BF16", 1), ("STG_DT_F16", 2)):
        assert re.search(rf"#define {name}\s+{v}\b", txt), name


def test_python_binds_the_entry_points_and_the_library_exports_them():
    from stellatrain_amd._capi import _SIGS, StgPublishTask, lib
    L = lib()
    for s in NEW:
        assert s in _SIGS and hasattr(L, s), s
    assert _SIGS[NEW[0]] == (C.c_int, [C.POINTER(StgPublishTask), C.c_size_t, C.c_void_p])
    assert _SIGS[NEW[1]] == (C.c_int, [C.POINTER(C.c_uint32), C.c_size_t, C.c_int])


def test_struct_layout_matches_the_header():
    from stellatrain_amd._capi import HEADER, StgPublishTask as K, StgReplica as R
    txt = " ".join(open(HEADER).read().split())
    m = re.search(r"\} stg_replica_t; /\* (\d+) bytes on LP64: d_param at (\d+), dtype at (\d+)", txt)
    assert m and tuple(map(int, m.groups())) == (16, 0, 8) == (C.sizeof(R), R.d_param.offset, R.dtype.offset)
    m = re.search(r"\} stg_publish_task_t; /\* (\d+) bytes on LP64: d_param at (\d+), param_len at (\d+), d_idx at "
                  r"(\d+), d_count at (\d+), idx_cap at (\d+), replicas at (\d+), nreplicas at (\d+)", txt)
    assert m, "the header documents stg_publish_task_t's layout"
    assert tuple(map(int, m.groups())) == (56, 0, 8, 16, 24, 32, 40, 48)
    assert tuple(map(int, m.groups())) == (C.sizeof(K), K.d_param.offset, K.param_len.offset, K.d_idx.offset,
                                           K.d_count.offset, K.idx_cap.offset, K.replicas.offset, K.nreplicas.offset)


def _launches(caps, num_cu=256):
    from stellatrain_amd._capi import lib
    a = (C.c_uint32 * max(len(caps), 1))(*caps)
    return lib().stg_debug_publish_launches(a, len(caps), num_cu)


def test_launch_sharing():
    """Up to 16 tasks per launch; empty tasks take no slot; a launch closes
    before its grid passes PER_CU workgroups per compute unit, and a task above
    that runs alone."""
    small = 600  # one workgroup
    assert _launches([]) == 0
    assert _launches([small]) == 1
    assert _launches([small] * 16) == 1
    assert _launches([small] * 17) == 2
    assert _launches([small] * 40) == 3
    assert _launches([0] * 5) == 0
    assert _launches([small, 0] * 16) == 1          # sixteen tasks with sixteen empty ones between them
    assert _launches([0, small] * 17) == 2
    limit = 2 * PER_CU                               # workgroups per launch on a device of two compute units
    big = limit * T + 1                              # one workgroup above the limit
    assert _launches([big], 2) == 1
    assert _launches([small, small, big, small, small], 2) == 3  # the neighbours' launch is split in two
    assert _launches([small] * 4 + [big] + [small] * 4, 2) == 3
    # the limit closes a launch of small tasks too: limit one-workgroup tasks fit, one more does not
    assert limit == 16 and _launches([T] * 16, 2) == 1 and _launches([T + 1] * 9, 2) == 2
    assert _launches([limit * T], 2) == 1 and _launches([small, limit * T], 2) == 2
    # bad arguments of the diagnostic itself
    from stellatrain_amd._capi import lib
    assert lib().stg_debug_publish_launches(None, 3, 256) == 0 and _launches([small], 0) == 0


class _Env:
    """Host memory standing in for device buffers: a refused call reads none of it."""

    def __init__(self):
        from stellatrain_amd._capi import StgPublishTask, StgReplica, lib
        self.L, self.Task, self.Rep = lib(), StgPublishTask, StgReplica
        self.buf = (C.c_uint8 * 128)()
        self.p = (C.addressof(self.buf) + 15) & ~15
        self.keep = []

    def reps(self, *entries):
        a = (self.Rep * max(len(entries), 1))(*[self.Rep(p, d) for p, d in entries])
        self.keep.append(a)
        return a

    def task(self, param="p", param_len=100, idx="p", count="p", cap=8, reps="good", nrep=None):
        p = self.p
        pick = lambda v: p if v == "p" else v  # noqa: E731
        if isinstance(reps, str):
            reps = self.reps((p, 0), (p + 2, 1), (p + 6, 2))
            nrep = 3 if nrep is None else nrep
        return self.Task(pick(param), param_len, pick(idx), pick(count), cap, reps, 1 if nrep is None else nrep)

    def bad_tasks(self):
        p = self.p
        return {
            "no replicas": (self.task(nrep=0), b"nreplicas"),
            "17 replicas": (self.task(nrep=17), b"nreplicas"),
            "no replicas, empty task": (self.task(cap=0, nrep=0), b"nreplicas"),
            "unknown dtype": (self.task(reps=self.reps((p, 3))), b"dtype"),
            "negative dtype": (self.task(reps=self.reps((p, 0), (p, -1)), nrep=2), b"dtype"),
            "unknown dtype, empty task": (self.task(cap=0, reps=self.reps((p, 7))), b"dtype"),
            "null parameter": (self.task(param=None), b"null"),
            "null indices": (self.task(idx=None), b"null"),
            "null count": (self.task(count=None), b"null"),
            "null replica array": (self.task(reps=None, nrep=1), b"null"),
            "null replica": (self.task(reps=self.reps((p, 0), (None, 1)), nrep=2), b"null"),
            "empty parameter": (self.task(param_len=0), b"empty"),
            "misaligned f32 replica": (self.task(reps=self.reps((p + 2, 0))), b"aligned"),
            "misaligned bf16 replica": (self.task(reps=self.reps((p, 0), (p + 1, 1)), nrep=2), b"aligned"),
            "misaligned f16 replica": (self.task(reps=self.reps((p + 3, 2))), b"aligned"),
        }


@pytest.fixture()
def env():
    return _Env()


def test_nothing_to_do_is_ok_without_a_device(env):
    f = env.L.stg_param_publish_batch_device
    one = (env.Task * 1)(env.task())
    assert f(None, 0, None) == 0
    assert f(one, 0, None) == 0
    assert f(None, 3, None) == -1 and b"task array" in env.L.stg_last_error()
    empty = (env.Task * 3)(*[env.task(cap=0) for _ in range(3)])
    assert f(empty, 3, None) == 0  # idx_cap == 0 launches nothing, so no device is asked for
    # ... and needs none of the pointers
    bare = (env.Task * 1)(env.task(param=None, idx=None, count=None, cap=0, reps=None, nrep=1, param_len=0))
    assert f(bare, 1, None) == 0


@pytest.mark.parametrize("pos", [0, 2, 4])
def test_one_bad_task_refuses_the_call_and_names_its_index(env, pos):
    """A bad task at the start, in the middle and at the end of five: refused
    with STG_ERR_INVALID before any device call (on a host without a device
    one would come back as STG_ERR_HIP), its index in the message."""
    f = env.L.stg_param_publish_batch_device
    for what, (bad, word) in env.bad_tasks().items():
        tasks = (env.Task * 5)(*[env.task() for _ in range(5)])
        tasks[pos] = bad
        assert f(tasks, 5, None) == -1, what
        msg = env.L.stg_last_error()
        assert b"task %d:" % pos in msg and word in msg, (what, msg)


def test_python_surface_validates_without_a_device():
    import torch
    import stellatrain_amd as S
    assert callable(S.publish_params) and callable(S.PublishTasks.from_merge)
    assert S.StgPublishTask is not None and S.StgReplica is not None
    assert S.PublishTasks([]).count == 0
    assert S.publish_params([]) is None
    p = torch.zeros(100)
    oi, cnt = torch.zeros(8, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="item 0.*replica 0.*dtype"):
        S.PublishTasks([(p, oi, cnt, [torch.zeros(100, dtype=torch.float64)])])
    with pytest.raises(ValueError, match="item 0.*replica 1.*size"):
        S.PublishTasks([(p, oi, cnt, [torch.zeros(100), torch.zeros(99, dtype=torch.bfloat16)])])
    with pytest.raises(ValueError, match="item 0.*replica 0.*contiguous"):
        S.PublishTasks([(p, oi, cnt, [torch.zeros(200, dtype=torch.float16)[::2]])])
    with pytest.raises(ValueError, match="item 0.*1..16"):
        S.PublishTasks([(p, oi, cnt, [])])
    with pytest.raises(ValueError, match="item 0.*1..16"):
        S.PublishTasks([(p, oi, cnt, [torch.zeros(100)] * 17)])
    with pytest.raises(ValueError, match="item 0.*float32"):
        S.PublishTasks([(p.double(), oi, cnt, [torch.zeros(100)])])
    with pytest.raises(ValueError, match="item 0.*int32"):
        S.PublishTasks([(p, oi.long(), cnt, [torch.zeros(100)])])
    with pytest.raises(ValueError, match="item 0.*expected"):
        S.PublishTasks([(p, oi, cnt)])
    with pytest.raises(ValueError, match="item 0.*HIP device"):
        S.PublishTasks([(p, oi, cnt, [torch.zeros(100)])])  # host tensors never reach the C call


def _torch_bits(x, dtype):
    import torch
    return torch.from_numpy(x).to(dtype).view(torch.int16).numpy().view(np.uint16)


def test_numpy_rne_models_agree_with_torch_cpu():
    """The yardstick of the GPU test, pinned on the CPU over every exponent
    class: bitwise where torch's result is no NaN, a NaN where it is one."""
    import torch
    x = P.exponent_class_values()
    u = x.view(np.uint32)
    a = u & 0x7fffffff
    for dt, tdt, model in ((P.DT_BF16, torch.bfloat16, P.f32_to_bf16_bits), (P.DT_F16, torch.float16,
                                                                              P.f32_to_f16_bits)):
        got, want = model(x), _torch_bits(x, tdt)
        nan = P.is_nan_bits(want, dt)
        assert np.array_equal(nan, a > 0x7f800000)             # NaN in, NaN out; nothing else becomes one
        assert np.array_equal(P.is_nan_bits(got, dt), nan)
        assert np.array_equal(got[~nan], want[~nan]), np.flatnonzero(got != want)[:5]
    # the classes the sweep must contain, by what they become
    h, b = P.f32_to_f16_bits(x), P.f32_to_bf16_bits(x)
    fin = a < 0x7f800000
    assert ((a == 0) & (h & 0x7fff == 0)).sum() >= 2 and (u == 0x80000000).any() and (h[u == 0x80000000] == 0x8000).all()
    assert ((a != 0) & (a < 0x00800000)).any()                                     # float32 subnormals
    assert ((h & 0x7c00 == 0) & (h & 0x3ff != 0)).sum() > 100                      # fp16 subnormal results
    assert (fin & (h & 0x7fff == 0x7c00)).sum() > 100 and (fin & (b & 0x7fff == 0x7f80)).any()  # overflow to inf
    assert ((a == 0x7f800000) & (h & 0x7fff == 0x7c00) & (b & 0x7fff == 0x7f80)).sum() == (a == 0x7f800000).sum() >= 2
    up_b = fin & ((b.astype(np.uint32) << 16 & 0x7f800000) > (a & 0x7f800000))    # rounded up into the next binade
    assert up_b.sum() > 100
    e = (a >> 23).astype(np.int64) - 127
    up_h = (e >= -14) & (e < 15) & (((h >> 10) & 0x1f).astype(np.int64) - 15 > e)
    assert up_h.sum() > 20
    assert (h[(a == 0x33000000)] & 0x7fff == 0).all() and (h[a == 0x33000001] & 0x7fff == 1).all()  # 2^-25: the tie
