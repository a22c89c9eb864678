"""CPU-only checks of the batched MERGE decompress + optimizer step
(``stg_merge_optimize_{sgd,adam}_batch_device``): the C-ABI declarations and
their Python binding, the task structure's layout, and the all-or-nothing
argument checks, which run before any device call."""
from __future__ import annotations

import ctypes as C

import pytest

NEW = ["stg_merge_optimize_sgd_batch_device", "stg_merge_optimize_adam_batch_device"]


def test_header_declares_the_entry_points_and_the_task():
    from stellatrain_amd._capi import HEADER, header_symbols
    syms = header_symbols()
    for s in NEW:
        assert s in syms, s
    txt = open(HEADER).read()
    assert "typedef struct stg_merge_task" in txt and "stg_merge_task_t" in txt


def test_python_binds_the_entry_points():
    from stellatrain_amd._capi import _SIGS, lib
    L = lib()
    for s in NEW:
        assert s in _SIGS and hasattr(L, s), s


def test_task_layout_matches_the_header():
    from stellatrain_amd._capi import StgMergeTask as T
    assert C.sizeof(T) == 88
    assert (T.name.offset, T.d_param.offset, T.param_len.offset, T.ranks.offset, T.per_rank.offset) == (0, 8, 16, 24, 32)
    assert (T.world.offset, T.d_dense.offset, T.d_mark.offset) == (40, 48, 56)
    assert (T.d_out_idx.offset, T.d_out_val.offset, T.d_out_count.offset) == (64, 72, 80)


class _Env:
    """Host memory standing in for device buffers: a refused call reads none of it."""

    def __init__(self):
        from stellatrain_amd._capi import StgMergeTask, StgRankStream, lib
        self.L, self.Task, self.Rank = lib(), StgMergeTask, StgRankStream
        self.buf = (C.c_uint8 * 128)()
        self.p = (C.addressof(self.buf) + 15) & ~15
        self.keep = []

    def ranks(self, *entries):
        a = (self.Rank * len(entries))(*[self.Rank(i, v, f) for i, v, f in entries])
        self.keep.append(a)
        return a

    def task(self, name=b"w", ranks="good", per_rank=4, world=1, dense=None, mark=None, param_len=100):
        p = self.p
        if isinstance(ranks, str):
            ranks = self.ranks(*([(p, p, 1)] * max(world, 1)))
        return self.Task(name, p, param_len, ranks, per_rank, world, dense, mark, p, p, p)

    def bad_tasks(self):
        p = self.p
        return {
            "world < 1": (self.task(world=0), b"world"),
            "flag 4": (self.task(ranks=self.ranks((p, p, 4))), b"flag"),
            "null buffer": (self.task(ranks=self.ranks((None, p, 1))), b"null"),
            "misaligned u32": (self.task(ranks=self.ranks((p + 2, p, 0))), b"misaligned"),
            "world 2 without scratch": (self.task(world=2), b"scratch"),
            "null name": (self.task(name=None), b"name"),
            "null rank array": (self.task(ranks=None), b"rank"),
            "empty parameter": (self.task(param_len=0), b"empty"),
        }


@pytest.fixture()
def env():
    return _Env()


def _sgd(L):
    h = C.c_void_p()
    assert L.stg_sgd_create(0, 0.1, 0.9, 0.0, 0.0, 0, 0, C.byref(h)) == 0
    return h


def _adam(L, amsgrad=0):
    h = C.c_void_p()
    assert L.stg_adam_create(0, 1e-3, 0.9, 0.999, 1e-8, 0.0, amsgrad, 0, C.byref(h)) == 0
    return h


def _iter(L, h):
    it = C.c_uint32(9)
    assert L.stg_sgd_get_iter(h, C.byref(it)) == 0
    return it.value


def test_empty_batch_and_null_arguments(env):
    L = env.L
    h, a = _sgd(L), _adam(L)
    one = (env.Task * 1)(env.task())
    for f, o in ((L.stg_merge_optimize_sgd_batch_device, h), (L.stg_merge_optimize_adam_batch_device, a)):
        assert f(o, None, 0, None) == 0  # nothing to do
        assert f(o, one, 0, None) == 0
        assert f(o, None, 3, None) == -1 and b"task array" in L.stg_last_error()
        assert f(None, one, 1, None) == -1  # null handle
    assert _iter(L, h) == 0
    assert L.stg_sgd_destroy(h) == 0 and L.stg_adam_destroy(a) == 0


@pytest.mark.parametrize("pos", [0, 2, 4])
def test_one_bad_task_refuses_the_batch_and_names_its_index(env, pos):
    """A bad task at the start, in the middle and at the end of five: the call
    is refused before any state change, and the message carries its index."""
    L = env.L
    h, a, ams = _sgd(L), _adam(L), _adam(L, 1)
    for what, (bad, word) in env.bad_tasks().items():
        tasks = (env.Task * 5)(*[env.task(name=b"p%d" % i) for i in range(5)])
        tasks[pos] = bad
        for f, o in ((L.stg_merge_optimize_sgd_batch_device, h), (L.stg_merge_optimize_adam_batch_device, a),
                     (L.stg_merge_optimize_adam_batch_device, ams)):
            if what == "empty parameter" and o is ams:
                continue  # only the fused step has this limit, as in the per-tensor call
            assert f(o, tasks, 5, None) == (-4 if what == "empty parameter" else -1), what
            msg = L.stg_last_error()
            assert msg.startswith(b"task %d:" % pos) and word in msg, (what, msg)
        assert _iter(L, h) == 0, what  # a refused call is no iteration
    assert L.stg_sgd_destroy(h) == 0 and L.stg_adam_destroy(a) == 0 and L.stg_adam_destroy(ams) == 0


def test_param_len_that_contradicts_an_earlier_task_is_refused(env):
    """Adam pins a name's length at its first call: two tasks of one name with
    different lengths are refused together, before any state exists."""
    L = env.L
    a = _adam(L)
    tasks = (env.Task * 3)(env.task(name=b"u"), env.task(name=b"v"), env.task(name=b"u", param_len=101))
    assert L.stg_merge_optimize_adam_batch_device(a, tasks, 3, None) == -1
    msg = L.stg_last_error()
    assert msg.startswith(b"task 2:") and b"param_len" in msg, msg
    assert L.stg_adam_destroy(a) == 0


def test_python_methods_exist_and_validate_without_a_device():
    import torch
    import stellatrain_amd as S
    assert callable(S.SparseSGD.merge_optimize_batch) and callable(S.SparseAdam.merge_optimize_batch)
    assert S.StgMergeTask is not None
    o = S.SparseSGD(lr=0.1)
    assert o.merge_optimize_batch([]) == []
    p = torch.zeros(100)
    i16, i32, f32 = (torch.zeros(8, dtype=d) for d in (torch.int16, torch.int32, torch.float32))
    good = (p, "a", [(i32, f32, 0)], 8)
    with pytest.raises(ValueError, match="item 1.*flag"):
        o.merge_optimize_batch([good, (p, "b", [(i32, f32, 4)], 8)])
    with pytest.raises(ValueError, match="item 1.*dtypes"):
        o.merge_optimize_batch([good, (p, "b", [(i32, f32, 1)], 8)])
    with pytest.raises(ValueError, match="item 0.*contiguous"):
        o.merge_optimize_batch([(p, "b", [(i16[::2], f32, 1)], 4)])
    with pytest.raises(ValueError, match="item 1.*shorter"):
        o.merge_optimize_batch([good, (p, "b", [(i16, f32, 1)], 9)])
    with pytest.raises(ValueError, match="item 1.*at least one"):
        o.merge_optimize_batch([good, (p, "b", [], 8)])
    with pytest.raises(ValueError, match="item 0.*expected"):
        o.merge_optimize_batch([(p, "b", [(i32, f32, 0)])])
    assert o.iteration == 0
