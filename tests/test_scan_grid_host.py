"""The grid of a batched thresholdv16 scan launch (csrc/scan_grid.h), through
the C-ABI's stg_debug_tv16_scan_grid: plain host arithmetic, no device.

G = round_up_8(2 * num_cu * F / S), S = min(distinct streams, hardware queues),
kept within [8, min(2 * num_cu, 512, round_up_8(chunks))]; F = 2.5 as shipped.
"""
from __future__ import annotations

import ctypes as C

import pytest

from stellatrain_amd._capi import lib

F = 2.5  # the shipped oversubscription factor (scan_grid.h TV16_GRID_F2 / 2)


@pytest.fixture(scope="module")
def grid():
    f = lib().stg_debug_tv16_scan_grid
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32]
    return f


def test_one_stream_takes_two_per_cu(grid):
    assert grid(256, 1, 4, 2048) == 512
    assert grid(256, 1, 1, 2048) == 512
    assert grid(128, 1, 4, 2048) == 256
    assert grid(256, 0, 4, 2048) == 512  # (no launch recorded yet counts as one stream)


def test_four_streams_shipped_factor(grid):
    assert grid(256, 4, 4, 2048) == int(2 * 256 * F / 4) == 320
    assert grid(256, 2, 4, 2048) == 512  # F / S > 1: the whole chip
    assert grid(256, 3, 4, 2048) == 432  # 426.67 rounded up to a multiple of 8
    assert grid(256, 8, 8, 2048) == 160


def test_streams_capped_by_hardware_queues(grid):
    assert grid(256, 16, 4, 2048) == grid(256, 4, 4, 2048)
    assert grid(256, 4, 2, 2048) == grid(256, 2, 2, 2048) == 512
    assert grid(256, 4, 1, 2048) == 512
    assert grid(256, 16, 32, 2048) == 80


def test_fewer_chunks_than_the_share(grid):
    assert grid(256, 1, 4, 198) == 200   # the chunks, rounded up to 8
    assert grid(256, 4, 4, 198) == 200
    assert grid(256, 4, 4, 64) == 64
    assert grid(256, 4, 4, 3) == 8
    assert grid(256, 1, 4, 1) == 8
    assert grid(256, 4, 4, 400) == 320   # the share, not the chunks


def test_multiple_of_8_at_least_8_at_most_two_per_cu(grid):
    for num_cu in (1, 3, 4, 37, 104, 256, 304):
        for streams in (1, 2, 3, 4, 5, 7, 16, 64):
            for hwq in (1, 2, 4, 8, 32):
                for chunks in (1, 7, 8, 9, 100, 511, 512, 513, 4096, 1 << 20):
                    g = grid(num_cu, streams, hwq, chunks)
                    assert g % 8 == 0 and g >= 8, (num_cu, streams, hwq, chunks, g)
                    assert g <= max(8, min(2 * num_cu, 512)), (num_cu, streams, hwq, chunks, g)
                    assert g <= max(8, (chunks + 7) // 8 * 8), (num_cu, streams, hwq, chunks, g)


def test_bad_arguments(grid):
    assert grid(0, 1, 4, 100) == 0
    assert grid(256, -1, 4, 100) == 0
