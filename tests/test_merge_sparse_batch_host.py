"""CPU-only checks of the batched sparse MERGE step: how
``stg_debug_merge_sparse_batch_plan`` groups shape lists (host arithmetic),
and that ``MergeTasks(..., sparse=True)`` carries no dense / mark."""
from __future__ import annotations

import pytest

TILE, TILES, PAIRS = 4096, 1 << 16, 1 << 21
A = (60000, 600, 2)  # a tensor as a model has hundreds of


@pytest.mark.parametrize("what, shapes, want", [
    ("17 equal tasks", [A] * 17, [0] * 16 + [1]),
    ("a change of world", [A] * 3 + [(60000, 600, 4)] * 2 + [A], [0, 0, 0, 1, 1, 2]),
    ("2^16 tiles fit, one more runs alone", [(TILES * TILE, 9, 2), ((TILES + 1) * TILE - 5, 9, 2), A], [0, None, 1]),
    ("closes just before the tile cap", [(TILES // 2 * TILE, 9, 1), ((TILES // 2 - 1) * TILE, 9, 1), (TILE, 9, 1),
                                         (TILE + 1, 9, 1), (1, 9, 1)], [0, 0, 0, 1, 1]),
    ("2^21 pairs fit, one more runs alone", [(70001, PAIRS // 2, 2), (70001, PAIRS // 2 + 1, 2), A], [0, None, 1]),
    ("closes just before the pair cap", [(70001, PAIRS // 4, 2), (70001, PAIRS // 4 - 1, 2), (33, 1, 2), (33, 1, 2)],
     [0, 0, 0, 1]),
    ("per_rank 0 runs alone", [A, (60000, 0, 2), A], [0, None, 1]),
    ("world 65 runs alone", [(60000, 600, 64), (60000, 600, 65), (60000, 600, 64)], [0, None, 1]),
    ("nothing", [], []),
])
def test_plan(what, shapes, want):
    from stellatrain_amd import merge_sparse_batch_plan
    assert merge_sparse_batch_plan(shapes) == want, what


def test_sparse_merge_tasks_hold_null_dense_and_mark():
    import torch
    from stellatrain_amd import MergeTasks, SparseAdam, SparseSGD
    p = torch.zeros(100)
    i32, f32 = torch.zeros(8, dtype=torch.int32), torch.zeros(8)
    items = [(p, "a", [(i32, f32, 0)] * 3, 8), (p, "b", [(i32, f32, 0)] * 2, 8, torch.zeros(100), None)]
    t = MergeTasks(items, sparse=True)
    assert [(x.d_dense, x.d_mark) for x in t.array[:2]] == [(None, None)] * 2
    assert [o[0].numel() for o in t.outputs] == [24, 16] and t.params[0] is p
    d = MergeTasks(items)  # the default: scratch for world > 1, as before
    assert d.array[0].d_dense and d.array[0].d_mark and d.array[1].d_dense == items[1][4].data_ptr()
    assert callable(SparseSGD.merge_optimize_sparse_batch) and callable(SparseAdam.merge_optimize_sparse_batch)
    assert SparseSGD(lr=0.1).merge_optimize_sparse_batch([]) == []
