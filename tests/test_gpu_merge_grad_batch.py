"""``merge_grad_batch`` against the loop of ``merge_grad`` calls (which
tests/test_gpu_merge_grad.py holds to the numpy model): outputs bit for bit,
the grouping, and the launches a call enqueues."""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_merge_grad import DTYPES, TILE, make, prior_of, upload

pytestmark = pytest.mark.gpu

OVER = (1 << 20) + 1  # per_rank at world 2: one pair past STG_SPARSE_BATCH_PAIRS
# (n, per_rank, world): 17 of world 2 cross the 16-task boundary; a change of world; per_rank == 0 in both modes;
# a task over the pair cap; a world of two bucketing rounds
SHAPES = [((1, 33, 4095, 4096, 4097, 2 * TILE + 5, 5 * TILE)[j % 7], (1, 9, 1025)[j % 3], 2) for j in range(17)]
SHAPES += [(4097, 9, 3), (4097, 0, 3), (33, 0, 3), (4097, OVER, 2), (2 * TILE + 5, 1025, 3), (4097, 9, 8)]
GROUPS = [0] * 16 + [1, 2, None, None, None, 3, 4]


def raw(torch, t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def test_batch_is_the_loop_bit_for_bit(gpu, oracle):
    import torch
    from stellatrain_amd import GradTasks, merge_batch_launches, merge_grad, merge_grad_batch, merge_sparse_batch_plan
    from stellatrain_amd.engine import scatter_merge_check
    assert merge_sparse_batch_plan(SHAPES) == GROUPS
    items, refs = [], []
    for j, (n, per_rank, world) in enumerate(SHAPES):
        streams = upload(torch, gpu, make(oracle, n, per_rank, world, j)[0])
        acc = j % 2 == 1
        out = prior_of(torch, n, getattr(torch, DTYPES[j % 3]), j).to(gpu)
        items.append((streams, per_rank, out, acc))
        refs.append(out.clone())
    # a group: its bucketing (count and place per four ranks, one scan) and one emission; alone: 2 + 2 * ceil(world / 64)
    want = sum(2 + 2 * -(-SHAPES[GROUPS.index(g)][2] // 4) for g in range(5))
    want += sum((4 if m else j % 2 == 0) for j, ((_, m, _), g) in enumerate(zip(SHAPES, GROUPS)) if g is None)
    tasks = GradTasks(items)
    for it in range(2):
        for (streams, per_rank, _, acc), ref in zip(items, refs):
            merge_grad(streams, per_rank, ref, accumulate=acc)
        before = merge_batch_launches()
        outs = merge_grad_batch(tasks if it else items)
        assert merge_batch_launches() - before == want
        for j, (out, ref) in enumerate(zip(outs, refs)):
            assert out is items[j][2] and torch.equal(raw(torch, out), raw(torch, ref)), (it, j, SHAPES[j])
        for streams, _, _, _ in items:  # the next iteration's pairs: rank 0's indices moved one slot on
            streams[0][0].copy_(streams[0][0].roll(1))
    scatter_merge_check()
