"""The codec-facing surface of ``FasterDpEngine`` and its MERGE call site.

Mirrors (``/root/reference/backend/src``):

* ``FasterDpEngine::configure_compression``        engine/core.cpp:185-195
* ``FasterDpEngine::configure_compression_ratio``  engine/core.cpp:197-200
* ``FasterDpEngine::compress(name, tensor, ratio)`` engine/core.cpp:1210-1245
  (pybind ``fasterdp.compress``, python/pybind.cpp:80-82)
* ``ModuleCompress::run`` MERGE path                engine/modules/compress.cpp:36-70,139-142,172-186
* ``ModuleCpuOptimize::run`` MERGE decompress       engine/modules/cpu_optimize.cpp:40-72
* ``SGD::optimize_raw``                             optim/sgd.cpp:34-263

The rest of the engine (shm, ZMQ ring, scheduler, telemetry) is out of scope
(SURVEY.md section 2).  All compute runs on the HIP library; this module only
computes sizes, owns buffers and orders launches on torch's current stream.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import (STG_DT_BF16, STG_DT_F16, STG_DT_F32, CodecError, StgMergeTask, StgPublishTask, StgRankStream,
                    StgReplica, StgWireRx, check, lib)
from .compressor import Compressor, make_compressor, typed_sources

__all__ = ["CodecEngine", "SparseSGD", "MergeTasks", "merge_numel", "api_numel", "scatter_merge", "scatter_merge_wire",
           "wire_decode_batch", "owner_of", "merge_batch_launches", "PublishTasks", "publish_params"]


def merge_numel(n: int, ratio: float, world: int = 1) -> int:
    """Pairs per rank on the MERGE path (compress.cpp:44,52): the kept fraction is
    stored in a float, ``n * k`` is a float product, truncated to int64."""
    kf = np.float32((1.0 - float(ratio)) / float(np.float32(world)))
    return max(min(int(n), 1), int(np.float32(np.float32(n) * kf)))


def api_numel(n: int, ratio: float) -> int:
    """``numel_to_select = (1. - ratio) * numel`` with a float ratio (core.cpp:1216)."""
    return int((1.0 - float(np.float32(ratio))) * n)


def owner_of(sizes, world: int) -> list[int]:
    """Key-affine bucket placement for multi-GPU runs: greedy
    longest-first bytes balancing (largest bucket to the least-loaded rank,
    ties by rank and bucket order); deterministic, so a key always lands on the
    same rank and its AIMD state stays resident there."""
    load = [0] * world
    out = [0] * len(sizes)
    order = sorted(range(len(sizes)), key=lambda i: (-int(sizes[i]), i))
    for i in order:
        g = min(range(world), key=lambda r: (load[r], r))
        load[g] += int(sizes[i])
        out[i] = g
    return out


class CodecEngine:
    """Codec part of ``FasterDpEngine``: default method thresholdv16
    (core.cpp:23-26), ratio 0.99, ``compress(name, tensor, ratio)``."""

    def __init__(self, device: int = 0):
        self.device = device
        self.compression_ratio_ = 0.99
        self.compressor_: Compressor | None = None
        self.configure_compression("thresholdv16")

    def configure_compression(self, method: str) -> None:
        # core.cpp:185-195 accepts only these two; "topk" only via configure()
        if method not in ("thresholdv", "thresholdv16"):
            raise CodecError(-2, f"Unknown compression method {method}.")
        self.compressor_ = make_compressor(method, device=self.device)

    def configure(self, method: str) -> None:
        """The factory inside FasterDpEngine::configure (core.cpp:110-118)."""
        self.compressor_ = make_compressor(method, device=self.device)

    def configure_compression_ratio(self, ratio: float) -> None:
        assert 0 < ratio <= 1
        self.compression_ratio_ = float(ratio)

    def compression_ratio(self) -> float:
        return self.compression_ratio_

    def compressor(self) -> Compressor:
        return self.compressor_

    def compress(self, name: str, tensor, ratio: float):
        """core.cpp:1210-1245: returns (idx int32, val float32), narrowed to the count."""
        import torch
        if ratio < 0 or ratio > 1:
            raise CodecError(-1, "Ratio must be in range [0, 1].")
        k = api_numel(tensor.numel(), ratio)
        dev = tensor.device
        idx = torch.empty(k, dtype=torch.int32, device=dev)
        val = torch.empty(k, dtype=torch.float32, device=dev)
        if k == 0:
            return idx, val
        total = self.compressor_.compress(name, tensor.reshape(-1), k, idx, val)
        if total != k:
            idx, val = idx.narrow(0, 0, total), val.narrow(0, 0, total)
        return idx, val

    def compress_bucket(self, key: str, grad, world: int = 1, residual=None):
        """MERGE path of ModuleCompress::run (compress.cpp:38-70,139-186), device
        resident and asynchronous.  Returns (idx, val, count) where idx/val have
        ``numel * world`` zeroed slots (compress.cpp:60-64) and the first
        ``numel`` are this node's pairs.  With ``residual`` given, applies the
        error feedback: zero the selected entries of ``grad`` (all ``numel``
        slots, including unwritten zero indices, compress.cpp:178-179) and copy
        the bucket into ``residual`` (compress.cpp:185)."""
        import torch
        n = grad.numel()
        numel = merge_numel(n, self.compression_ratio_, world)
        idx = torch.zeros(numel * world, dtype=torch.int32, device=grad.device)
        val = torch.zeros(numel * world, dtype=torch.float32, device=grad.device)
        if not grad.is_contiguous():
            raise ValueError("grad must be contiguous")
        if residual is not None and (residual.numel() != n or residual.dtype != torch.float32
                                     or not residual.is_contiguous()):
            raise ValueError("residual must be a contiguous float32 tensor of the bucket's size")
        g = grad.reshape(-1)
        if residual is None:
            cnt = self.compressor_.compress_async(key, g, numel, idx[:numel], val[:numel], 0)
        else:
            # stg_merge_compress_batch_device: codec + error feedback, the
            # residual copy fused into thresholdv16's streaming pass
            cnt = self.compressor_.compress_batch_async([(key, g, numel, idx[:numel], val[:numel], 0)],
                                                        residuals=[residual.reshape(-1)])
        return idx, val, cnt

    def send_buckets(self, items, world: int = 1, fp16_values: bool = False):
        """The sender side of one iteration in one call
        (``Compressor.merge_send_batch_async``): for every item ``(key,
        grads[, residual])`` ModuleCpuGather::run over ``grads`` (this rank's
        slices, ``grads[0]`` the bucket), ``compress_bucket``'s MERGE compress
        with the error feedback when ``residual`` is given, and queueTx's
        packing.  Per tensor the pair count is ``merge_numel(n, ratio, world)``
        and the wire form ``wire_flag(n, fp16_values)``.  Returns ``(streams,
        counts)``: per item ``(idx, val, flag)`` with ``numel * world`` zeroed
        slots in the flag's types, the first ``numel`` this node's stream in the
        form the ring sends, and the int32 counts tensor (no host sync).  An
        item may be ``(key, grads, residual, bucket)``: ``grads`` of float32,
        bfloat16 or float16 and ``bucket`` the float32 tensor that receives the
        sum, as ``SendTasks`` describes (without ``bucket``, ``grads[1:]`` may
        still be 16-bit).  Works under ``configure_compression("thresholdv")``
        as well: the key is then the bucket's pointer, the count varies, and
        all ``W = min(numel, n)`` slots are written -- the pairs, then the wire
        form of ``(0, 0.0)`` -- with element 0 zeroed by the error feedback
        whenever the count is below ``W``; and under ``configure("topk_exact")``:
        the ``numel`` largest magnitudes in index order, the count ``numel``
        (``configure("topk")``, the shipped operator, is refused)
        (``Compressor.merge_send_batch_async``)."""
        import torch
        send, streams = [], []
        for it in items:
            key, grads = it[0], list(it[1])
            residual = it[2] if len(it) > 2 else None
            bucket = it[3] if len(it) > 3 else None
            if not all(t.is_contiguous() for t in grads + [t for t in (residual, bucket) if t is not None]):
                raise ValueError("send_buckets: gradients and residual must be contiguous")
            n = grads[0].numel()
            numel = merge_numel(n, self.compression_ratio_, world)
            flag = wire_flag(n, fp16_values)
            di, dv = _wire_dtypes(flag)
            idx = torch.zeros(numel * world, dtype=di, device=grads[0].device)
            val = torch.zeros(numel * world, dtype=dv, device=grads[0].device)
            send.append((key, [g.reshape(-1) for g in grads], numel, idx[:numel], val[:numel],
                         residual.reshape(-1) if residual is not None else None, flag) +
                        ((0, bucket.reshape(-1)) if bucket is not None else ()))
            streams.append((idx, val, flag))
        counts = self.compressor_.merge_send_batch_async(send)
        return streams, counts


def scatter_merge(idx, val, per_rank: int, world: int, n: int, dense=None, mark=None, out_idx=None, out_val=None,
                  count=None):
    """MERGE decompress on the device (cpu_optimize.cpp:40-72).  ``dense``
    (float32[n]) and ``mark`` (uint8[n]) must be zero and are left zero.  Per
    rank, the last occurrence of a duplicated index wins (index_put_ without
    accumulate); the output holds each index once (unique1d)."""
    import torch
    dev = idx.device
    dp, mp, out_idx, out_val, count = _merge_outputs(dev, n, per_rank, world, dense, mark, out_idx, out_val, count)
    check(lib().stg_scatter_merge_device(C.c_void_p(idx.data_ptr()), C.c_void_p(val.data_ptr()), per_rank, world, n,
                                         dp, mp, C.c_void_p(out_idx.data_ptr()), C.c_void_p(out_val.data_ptr()),
                                         C.c_void_p(count.data_ptr()),
                                         C.c_void_p(torch.cuda.current_stream(dev.index).cuda_stream)))
    return out_idx, out_val, count


def scatter_merge_check(device=None) -> None:
    """Raises CodecError when a MERGE decompress on the current stream of
    ``device`` hit a device failure (a look-back that gave up; the count of
    that call reads 0xffffffff).  Syncs the stream."""
    import torch
    dev = _cuda_device(device)
    with torch.cuda.device(dev):  # the C side keys the scratch on the current device
        check(lib().stg_scatter_merge_check(C.c_void_p(torch.cuda.current_stream(dev.index).cuda_stream)))


def scatter_merge_release(device=None) -> None:
    """Frees the MERGE decompress scratch kept for the current stream of
    ``device`` (call before dropping a stream that merged)."""
    import torch
    dev = _cuda_device(device)
    with torch.cuda.device(dev):
        check(lib().stg_scatter_merge_release(C.c_void_p(torch.cuda.current_stream(dev.index).cuda_stream)))


def merge_batch_launches(device=None) -> int:
    """Kernel launches the ``merge_optimize_batch`` calls have enqueued on the
    current stream of ``device`` since its MERGE scratch was created (0 before
    the first merge on it, and again after ``scatter_merge_release``): the
    shared launches and the per-tensor sequences run inside a batch, their
    step launches included.  A batched call's results are those of the loop;
    the difference of this count around a call shows what it shared."""
    import torch
    dev = _cuda_device(device)
    out = C.c_uint64()
    with torch.cuda.device(dev):
        check(lib().stg_merge_batch_launches(C.c_void_p(torch.cuda.current_stream(dev.index).cuda_stream),
                                             C.byref(out)))
    return int(out.value)


def _cuda_device(device):
    """torch.device of `device` (None or a bare "cuda": the current device)."""
    import torch
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    d = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device() if d.index is None else d.index)


def gather_slice(n: int, local_rank: int, num_gpus: int):
    """Local rank's slice [n*r/N, n*(r+1)/N) of the gather-add (cpu_gather.cpp:59-61)."""
    a, b = C.c_uint64(), C.c_uint64()
    check(lib().stg_gather_slice(n, local_rank, num_gpus, C.byref(a), C.byref(b)))
    return a.value, b.value


def gather_add(grads, residual, local_rank: int, out=None) -> None:
    """ModuleCpuGather::run on the device (cpu_gather.cpp:59-87): over this
    local rank's slice, ``grads[0] += residual + grads[1] + ... + grads[N-1]``
    left to right, in one pass.  ``grads`` are float32 device tensors of one
    size (peers' buffers where P2P is enabled); ``residual`` may be None.
    ``grads[1:]`` may also be bfloat16 or float16 (16-bit model replicas'
    gradients): they are widened, exactly, as they are loaded
    (``stg_gather_add_typed_device``).  With ``out``, a float32 tensor, the
    slice of ``out`` receives the sum and ``grads[0]``, of any of the three
    types, is only read; a 16-bit ``grads[0]`` without ``out`` is a
    ValueError."""
    import torch
    g0 = grads[0]
    n = g0.numel()
    if out is not None or any(t.dtype in (torch.bfloat16, torch.float16) for t in grads):
        f32 = [t for t in (residual, out) if t is not None]
        typed = typed_sources("gather_add", grads, out)
        if any(t.dtype != torch.float32 for t in f32):
            raise ValueError("gather_add: float32 residual and out")
        for t in list(grads) + f32:
            if t.numel() != n or not t.is_contiguous() or not t.is_cuda:
                raise ValueError("gather_add: contiguous device tensors of one size")
        d0 = g0 if out is None else out
        check(lib().stg_gather_add_typed_device(C.c_void_p(d0.data_ptr()),
                                                C.c_void_p(residual.data_ptr()) if residual is not None else None,
                                                typed, len(grads), n, local_rank,
                                                C.c_void_p(torch.cuda.current_stream(d0.device.index).cuda_stream)))
        return
    for t in list(grads) + ([residual] if residual is not None else []):
        if t.numel() != n or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("gather_add: contiguous float32 device tensors of one size")
    ptrs = (C.c_void_p * len(grads))(*[t.data_ptr() for t in grads])
    check(lib().stg_gather_add_device(C.c_void_p(g0.data_ptr()),
                                      C.c_void_p(residual.data_ptr()) if residual is not None else None,
                                      ptrs, len(grads), n, local_rank,
                                      C.c_void_p(torch.cuda.current_stream(g0.device.index).cuda_stream)))


WIRE_U16_IDX = 0x01  # COMM_FLAG_UINT16_IDX (comm_manager.h:24)
WIRE_F16_VAL = 0x02  # COMM_FLAG_FP16_VAL (comm_manager.h:25)


def wire_flag(tensor_numel: int, fp16_values: bool = False) -> int:
    """The flag byte CommManager::queueTx sends (comm_manager.cpp:573-590)."""
    return int(lib().stg_wire_flag(tensor_numel, int(fp16_values)))


def wire_encode(idx, val, flag: int, idx_out=None, val_out=None):
    """Pack a (idx, val) stream into the ring's wire layout on the device
    (comm_manager.cpp:509-548): int16-typed u16 indices when ``flag & 1``,
    fp16 bits (as int16) when ``flag & 2``; otherwise the 32-bit arrays."""
    import torch
    dev, n = idx.device, idx.numel()
    if idx_out is None:
        idx_out = torch.empty(n, dtype=torch.int16 if flag & WIRE_U16_IDX else torch.int32, device=dev)
    if val_out is None:
        val_out = torch.empty(n, dtype=torch.int16 if flag & WIRE_F16_VAL else torch.float32, device=dev)
    check(lib().stg_wire_encode_device(C.c_void_p(idx.data_ptr()), C.c_void_p(val.data_ptr()), n, flag,
                                       C.c_void_p(idx_out.data_ptr()), C.c_void_p(val_out.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream(dev.index).cuda_stream)))
    return idx_out, val_out


class StgWireStream(C.Structure):
    _fields_ = [("d_idx", C.c_void_p), ("d_val", C.c_void_p), ("numel", C.c_size_t), ("flag", C.c_int),
                ("d_idx_out", C.c_void_p), ("d_val_out", C.c_void_p)]


def wire_encode_batch(items):
    """Batched wire encode (``stg_wire_encode_batch_device``): items of
    (idx, val, flag, idx_out, val_out) device tensors; the same bytes as
    ``wire_encode`` on each, in launches of up to 16 streams."""
    import torch
    if not items:
        return
    arr = (StgWireStream * len(items))()
    for j, (idx, val, flag, io, vo) in enumerate(items):
        arr[j] = StgWireStream(idx.data_ptr(), val.data_ptr(), idx.numel(), int(flag), io.data_ptr(), vo.data_ptr())
    dev = items[0][0].device
    check(lib().stg_wire_encode_batch_device(arr, len(items),
                                             C.c_void_p(torch.cuda.current_stream(dev.index).cuda_stream)))


def wire_decode(widx, wval, flag: int, idx=None, val=None):
    """Unpack a received stream (comm_manager.cpp:877-906) into int32 indices
    and float32 values on the device."""
    import torch
    dev, n = widx.device, widx.numel()
    if idx is None:
        idx = torch.empty(n, dtype=torch.int32, device=dev)
    if val is None:
        val = torch.empty(n, dtype=torch.float32, device=dev)
    check(lib().stg_wire_decode_device(C.c_void_p(widx.data_ptr()), C.c_void_p(wval.data_ptr()), n, flag,
                                       C.c_void_p(idx.data_ptr()), C.c_void_p(val.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream(dev.index).cuda_stream)))
    return idx, val


def _wire_dtypes(flag: int):
    import torch
    if flag not in (0, 1, 2, 3):
        raise ValueError(f"wire flag {flag!r} outside 0..3")
    return (torch.int16 if flag & WIRE_U16_IDX else torch.int32,
            torch.int16 if flag & WIRE_F16_VAL else torch.float32)


def wire_decode_batch(items):
    """Batched wire decode (``stg_wire_decode_batch_device``): items of
    (widx, wval, flag, idx_out, val_out) device tensors; the same bytes as
    ``wire_decode`` on each, in launches of up to 16 streams."""
    import torch
    if not items:
        return
    arr = (StgWireRx * len(items))()
    for j, (wi, wv, flag, io, vo) in enumerate(items):
        flag = int(flag)
        di, dv = _wire_dtypes(flag)
        n = wi.numel()
        if wi.dtype != di or wv.dtype != dv or io.dtype != torch.int32 or vo.dtype != torch.float32:
            raise ValueError(f"wire_decode_batch: item {j}: dtypes do not match flag {flag}")
        if not all(t.is_contiguous() for t in (wi, wv, io, vo)):
            raise ValueError(f"wire_decode_batch: item {j}: tensors must be contiguous")
        if wv.numel() < n or io.numel() < n or vo.numel() < n:
            raise ValueError(f"wire_decode_batch: item {j}: a tensor is shorter than the stream")
        arr[j] = StgWireRx(wi.data_ptr(), wv.data_ptr(), n, flag, io.data_ptr(), vo.data_ptr())
    dev = items[0][0].device
    check(lib().stg_wire_decode_batch_device(arr, len(items),
                                             C.c_void_p(torch.cuda.current_stream(dev.index).cuda_stream)))


def _rank_streams(streams, per_rank: int):
    """The ``stg_rank_stream_t`` array of a list of (widx, wval, flag) device
    tensors, after checking dtype against flag, contiguity and length."""
    if not streams:
        raise ValueError("at least one rank stream is required")
    arr = (StgRankStream * len(streams))()
    for r, (wi, wv, flag) in enumerate(streams):
        flag = int(flag)
        di, dv = _wire_dtypes(flag)
        if wi.dtype != di or wv.dtype != dv:
            raise ValueError(f"rank {r}: dtypes {wi.dtype}/{wv.dtype} do not match wire flag {flag}")
        if not wi.is_contiguous() or not wv.is_contiguous():
            raise ValueError(f"rank {r}: stream tensors must be contiguous")
        if wi.numel() < per_rank or wv.numel() < per_rank:
            raise ValueError(f"rank {r}: stream shorter than per_rank = {per_rank}")
        if wi.device != streams[0][0].device or wv.device != wi.device:
            raise ValueError(f"rank {r}: stream tensors on different devices")
        arr[r] = StgRankStream(wi.data_ptr(), wv.data_ptr(), flag)
    return arr


def _merge_outputs(dev, n, per_rank, world, dense, mark, out_idx, out_val, count):
    import torch
    if out_idx is None:
        out_idx = torch.empty(per_rank * world, dtype=torch.int32, device=dev)
    if out_val is None:
        out_val = torch.empty(per_rank * world, dtype=torch.float32, device=dev)
    if count is None:
        count = torch.empty(1, dtype=torch.int32, device=dev)
    if world > 1:
        if dense is None:
            dense = torch.zeros(n, dtype=torch.float32, device=dev)
        if mark is None:
            mark = torch.zeros(n, dtype=torch.uint8, device=dev)
    dp = C.c_void_p(dense.data_ptr()) if dense is not None else None
    mp = C.c_void_p(mark.data_ptr()) if mark is not None else None
    return dp, mp, out_idx, out_val, count


def scatter_merge_wire(streams, per_rank: int, n: int, dense=None, mark=None, out_idx=None, out_val=None,
                       count=None):
    """MERGE decompress straight from received streams: ``streams`` is one
    (widx, wval, flag) per rank, each where it landed and in the form it
    arrived in (int16-typed tensors for the 16-bit forms, as ``wire_encode``
    returns them).  The result is bitwise that of ``wire_decode`` per rank
    into one buffer followed by ``scatter_merge``, without the decode launches
    and the buffer.  ``dense`` / ``mark`` as in ``scatter_merge``."""
    import torch
    world = len(streams)
    arr = _rank_streams(streams, per_rank)
    dev = streams[0][0].device
    dp, mp, out_idx, out_val, count = _merge_outputs(dev, n, per_rank, world, dense, mark, out_idx, out_val, count)
    check(lib().stg_scatter_merge_wire_device(arr, per_rank, world, n, dp, mp, C.c_void_p(out_idx.data_ptr()),
                                              C.c_void_p(out_val.data_ptr()), C.c_void_p(count.data_ptr()),
                                              C.c_void_p(torch.cuda.current_stream(dev.index).cuda_stream)))
    return out_idx, out_val, count


def _merge_optimize(fn, h, param, name, src, per_rank, world, dense, mark, out_idx, out_val, count):
    """ModuleCpuOptimize::run through one C call (``fn``): the MERGE decompress
    of ``world`` rank streams into the merged stream (returned), then the
    optimizer's step on it.  ``src`` is the entry's stream arguments: the
    decoded (idx, val) pointers, or the one ``_rank_streams`` array."""
    import torch
    dev, n = param.device, param.numel()
    dp, mp, out_idx, out_val, count = _merge_outputs(dev, n, per_rank, world, dense, mark, out_idx, out_val, count)
    check(fn(h, name.encode(), C.c_void_p(param.data_ptr()), n, *src, per_rank, world, dp, mp,
             C.c_void_p(out_idx.data_ptr()), C.c_void_p(out_val.data_ptr()), C.c_void_p(count.data_ptr()),
             C.c_void_p(torch.cuda.current_stream(dev.index).cuda_stream)))
    return out_idx, out_val, count


def _decoded(idx, val):
    return C.c_void_p(idx.data_ptr()), C.c_void_p(val.data_ptr())


class MergeTasks:
    """A prebuilt ``stg_merge_task_t`` array: the iteration's ModuleCpuOptimize
    tasks, marshalled and validated once and reused by every
    ``merge_optimize_batch`` call on the same tensors (a model's parameters and
    receive buffers do not move between iterations).  Each item is ``(param,
    name, streams, per_rank)`` plus, optionally, ``dense, mark, out_idx,
    out_val, count`` (positional, None to allocate); ``streams`` is a list of
    (widx, wval, flag) as in ``scatter_merge_wire``, validated as there.
    ``outputs`` holds one (out_idx, out_val, count) per item: every call on
    the array writes the same output tensors (and, at world > 1, is given the
    same dense / mark scratch, left zero by each call; items that share a group
    work on the library's scratch instead), so read an iteration's merged
    streams before the next call.  The array keeps every tensor it
    points at alive, the ones allocated here included."""

    def __init__(self, items):
        import torch
        items = list(items)
        self.count = len(items)
        self.array = (StgMergeTask * max(self.count, 1))()
        self.outputs = []
        self.device = items[0][0].device if items else None
        self._keep = []  # everything the C call reads or writes stays alive with the array
        dev = self.device
        for j, it in enumerate(items):
            if not 4 <= len(it) <= 9:
                raise ValueError(f"merge_optimize_batch: item {j}: (param, name, streams, per_rank[, dense, mark, "
                                 "out_idx, out_val, count]) expected")
            param, name, streams, per_rank = it[:4]
            dense, mark, out_idx, out_val, count = (tuple(it[4:]) + (None,) * 5)[:5]
            per_rank = int(per_rank)
            try:
                ranks = _rank_streams(streams, per_rank)
            except ValueError as e:
                raise ValueError(f"merge_optimize_batch: item {j}: {e}") from None
            if param.device != dev or streams[0][0].device != dev:
                raise ValueError(f"merge_optimize_batch: item {j}: tensors on different devices")
            if param.dtype != torch.float32 or not param.is_contiguous():
                raise ValueError(f"merge_optimize_batch: item {j}: the parameter must be contiguous float32")
            world, n = len(streams), param.numel()
            if world > 1:  # allocated here, not in _merge_outputs: it returns pointers only, and these must outlive it
                if dense is None:
                    dense = torch.zeros(n, dtype=torch.float32, device=dev)
                if mark is None:
                    mark = torch.zeros(n, dtype=torch.uint8, device=dev)
            dp, mp, out_idx, out_val, count = _merge_outputs(dev, n, per_rank, world, dense, mark, out_idx, out_val,
                                                             count)
            if out_idx.numel() < per_rank * world or out_val.numel() < per_rank * world:
                raise ValueError(f"merge_optimize_batch: item {j}: output shorter than per_rank * world")
            nm = name.encode()
            self.array[j] = StgMergeTask(nm, param.data_ptr(), n, ranks, per_rank, world, dp, mp, out_idx.data_ptr(),
                                         out_val.data_ptr(), count.data_ptr())
            self._keep.append((ranks, nm, param, streams, dense, mark))
            self.outputs.append((out_idx, out_val, count))

    @property
    def params(self):
        """The items' parameter tensors, in order."""
        return [k[2] for k in self._keep]


def _merge_optimize_batch(fn, h, items):
    """The iteration's ModuleCpuOptimize tasks through one C call (``fn``):
    ``items`` as ``MergeTasks`` takes them, or a prebuilt ``MergeTasks``."""
    import torch
    tasks = items if isinstance(items, MergeTasks) else MergeTasks(items)
    if not tasks.count:
        return []
    rc = fn(h, tasks.array, tasks.count, C.c_void_p(torch.cuda.current_stream(tasks.device.index).cuda_stream))
    if rc:
        check(rc)
    return tasks.outputs


class PublishTasks:
    """A prebuilt ``stg_publish_task_t`` array for ``publish_params``,
    marshalled and validated once (a model's parameters, merged-stream buffers
    and replicas do not move between iterations).  Each item is ``(param,
    out_idx, count, replicas)``: the float32 master parameter, the step's
    merged indices and device count (``merge_optimize_batch``'s ``out_idx`` and
    ``count``; ``idx_cap = out_idx.numel()``), and 1..16 contiguous replica
    tensors of ``param.numel()`` elements, float32, bfloat16 or float16, each
    on any HIP device the master can reach.  The array keeps every tensor it
    points at alive."""

    def __init__(self, items):
        import torch
        dts = {torch.float32: STG_DT_F32, torch.bfloat16: STG_DT_BF16, torch.float16: STG_DT_F16}
        items = list(items)
        self.count = len(items)
        self.array = (StgPublishTask * max(self.count, 1))()
        self.device = items[0][0].device if items else None
        self._keep = []
        for j, it in enumerate(items):
            if len(it) != 4:
                raise ValueError(f"publish_params: item {j}: (param, out_idx, count, replicas) expected")
            param, out_idx, count, replicas = it
            replicas = list(replicas)
            if param.dtype != torch.float32 or not param.is_contiguous():
                raise ValueError(f"publish_params: item {j}: the parameter must be contiguous float32")
            if out_idx.dtype != torch.int32 or not out_idx.is_contiguous() or count.dtype != torch.int32 \
                    or count.numel() < 1:
                raise ValueError(f"publish_params: item {j}: out_idx must be contiguous int32 and count an int32 word")
            if not 1 <= len(replicas) <= 16:
                raise ValueError(f"publish_params: item {j}: replicas outside 1..16")
            reps = (StgReplica * len(replicas))()
            for r, t in enumerate(replicas):
                if t.dtype not in dts:
                    raise ValueError(f"publish_params: item {j}: replica {r}: dtype {t.dtype} is not float32, "
                                     "bfloat16 or float16")
                if t.numel() != param.numel():
                    raise ValueError(f"publish_params: item {j}: replica {r}: size {t.numel()} is not the "
                                     f"parameter's {param.numel()}")
                if not t.is_contiguous():
                    raise ValueError(f"publish_params: item {j}: replica {r}: not contiguous")
            if not all(t.is_cuda for t in [param, out_idx, count] + replicas):
                raise ValueError(f"publish_params: item {j}: tensors must be on a HIP device")
            if param.device != self.device or out_idx.device != self.device or count.device != self.device:
                raise ValueError(f"publish_params: item {j}: parameter, out_idx and count must be on the master's "
                                 "device")
            for r, t in enumerate(replicas):
                reps[r] = StgReplica(t.data_ptr(), dts[t.dtype])
            self.array[j] = StgPublishTask(param.data_ptr(), param.numel(), out_idx.data_ptr(), count.data_ptr(),
                                           out_idx.numel(), reps, len(replicas))
            self._keep.append((reps, param, out_idx, count, replicas))

    @classmethod
    def from_merge(cls, merge_tasks: MergeTasks, replicas_per_item):
        """The publish tasks of a ``MergeTasks`` array: item j's parameter and
        its ``outputs[j]`` (merged indices and count), with
        ``replicas_per_item[j]`` as its replicas."""
        replicas_per_item = list(replicas_per_item)
        if len(replicas_per_item) != merge_tasks.count:
            raise ValueError("publish_params: one replica list per merge task expected")
        return cls([(p, o[0], o[2], reps) for p, o, reps in zip(merge_tasks.params, merge_tasks.outputs,
                                                                replicas_per_item)])


def publish_params(items) -> None:
    """ModuleH2DCopy::run (h2d_copy.cpp:31-56) for device-resident parameters,
    through ``stg_param_publish_batch_device``: every replica of every item
    receives the parameter's value at the indices the step just wrote (the
    first ``count`` of ``out_idx``; bfloat16 / float16 replicas rounded to
    nearest even) and is otherwise left alone.  Runs on the current stream of
    the master's device, after the step enqueued there; a peer's stream must
    be made to wait on it by the caller.  ``items`` as ``PublishTasks`` takes
    them, or a prebuilt ``PublishTasks`` (no per-call marshalling)."""
    import torch
    tasks = items if isinstance(items, PublishTasks) else PublishTasks(items)
    if not tasks.count:
        return
    with torch.cuda.device(tasks.device):
        rc = lib().stg_param_publish_batch_device(
            tasks.array, tasks.count, C.c_void_p(torch.cuda.current_stream(tasks.device.index).cuda_stream))
    if rc:
        check(rc)


class SparseSGD:
    """``SGD`` sparse optimizer (optim/sgd.h:10-50) on the device.  Options as
    SGD::configure (sgd.cpp:265-300); ``optimize_raw`` as sgd.cpp:34-263.

    ``smart_momentum`` (sgd.cpp:291-292): a touched element's buffer decays by
    ``momentum ** (iterations since its index was last touched)``.  The
    iteration count is the optimizer's, shared by all names."""

    def __init__(self, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False, maximize: bool = False, device: int = 0, smart_momentum: bool = False):
        h = C.c_void_p()
        check(lib().stg_sgd_create(device, lr, momentum, dampening, weight_decay, int(nesterov), int(maximize),
                                   C.byref(h)))
        self._h = h
        self.device = device
        if smart_momentum:
            self.configure("smart_momentum", True)

    def configure(self, option_name: str, option_value) -> None:
        """SGD::configure(name, bool) for the option set after construction
        (sgd.cpp:284-297); any other name raises as the reference throws."""
        if option_name != "smart_momentum" or not isinstance(option_value, (bool, np.bool_)):
            raise CodecError(-1, "NO OPTION")
        check(lib().stg_sgd_set_smart_momentum(self._h, int(option_value)))

    @property
    def iteration(self) -> int:
        """Calls made so far on this optimizer, over all names (m_iter)."""
        it = C.c_uint32()
        check(lib().stg_sgd_get_iter(self._h, C.byref(it)))
        return int(it.value)

    def check(self) -> None:
        """Raise CodecError (STG_ERR_DEVICE) if a smart-momentum element was
        ever skipped: an index repeated within one call.  Syncs the stream."""
        import torch
        check(lib().stg_sgd_check(self._h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def last_buffer(self, name: str, n: int):
        """The iteration that last touched each index of ``name`` (uint32), or
        None before the name's first call with smart momentum on."""
        import torch
        out = np.zeros(n, np.uint32)
        rc = lib().stg_sgd_get_last(self._h, name.encode(), C.c_void_p(out.ctypes.data), n,
                                    C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        return None if rc else out

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                lib().stg_sgd_destroy(h)
            except Exception:
                pass
            self._h = None

    def name(self) -> str:
        return "SGD"

    def optimize_raw(self, param, name: str, grad, gidx, grad_len: int | None = None, d_grad_len=None) -> None:
        import torch
        n = int(grad_len if grad_len is not None else grad.numel())
        check(lib().stg_sgd_optimize_raw_device(
            self._h, name.encode(), C.c_void_p(param.data_ptr()), param.numel(), C.c_void_p(grad.data_ptr()),
            C.c_void_p(gidx.data_ptr()), n, C.c_void_p(d_grad_len.data_ptr()) if d_grad_len is not None else None,
            C.c_void_p(torch.cuda.current_stream(param.device.index).cuda_stream)))

    def merge_optimize(self, param, name: str, idx, val, per_rank: int, world: int = 1, dense=None, mark=None,
                       out_idx=None, out_val=None, count=None):
        """ModuleCpuOptimize::run (cpu_optimize.cpp:26-100): the MERGE
        decompress, then optimize_raw on its output; at world 1 the step runs
        inside the decompress's emission launch."""
        return _merge_optimize(lib().stg_merge_optimize_sgd_device, self._h, param, name, _decoded(idx, val), per_rank,
                               world, dense, mark, out_idx, out_val, count)

    def merge_optimize_wire(self, param, name: str, streams, per_rank: int, dense=None, mark=None, out_idx=None,
                            out_val=None, count=None):
        """``merge_optimize`` straight from received streams, one (widx, wval,
        flag) per rank as in ``scatter_merge_wire``; bitwise the result of
        ``wire_decode`` per rank followed by ``merge_optimize``."""
        return _merge_optimize(lib().stg_merge_optimize_sgd_wire_device, self._h, param, name,
                               (_rank_streams(streams, per_rank),), per_rank, len(streams), dense, mark, out_idx,
                               out_val, count)

    def merge_optimize_batch(self, items):
        """``merge_optimize_wire`` on every item in order, in one call: items
        are ``(param, name, streams, per_rank[, dense, mark, out_idx, out_val,
        count])``; bitwise the results of the loop.  Consecutive world-1 items
        (up to 16, parameter lengths summing to at most 8 Mi, distinct names)
        share one launch pair.  Consecutive items of one world > 1 (up to 16,
        parameter lengths summing to at most 4 Mi, distinct names) share
        world + 4 launches and work on the library's scratch; their ``dense``
        / ``mark`` are still required, stay zero, and one pair may serve every
        item.  Empty items and world > 1 items above 4 Mi elements run one by
        one at their place.  ``items`` may be a prebuilt ``MergeTasks`` (no
        per-call marshalling).  Returns a list of (out_idx, out_val, count).
        ``merge_batch_launches`` counts the launches."""
        return _merge_optimize_batch(lib().stg_merge_optimize_sgd_batch_device, self._h, items)

    def momentum_buffer(self, name: str, n: int):
        import torch
        out = np.zeros(n, np.float32)
        rc = lib().stg_sgd_get_momentum(self._h, name.encode(), C.c_void_p(out.ctypes.data), n,
                                        C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        return None if rc else out


class SparseAdam:
    """``Adam`` sparse optimizer (optim/adam.h:10-55) on the device.  Options as
    Adam::configure (adam.cpp:90-122; defaults adam.h:21-23, lr
    sparse_optimizer.h:30); ``optimize_raw`` as adam.cpp:19-86."""

    def __init__(self, lr: float = 1e-3, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8,
                 weight_decay: float = 0.0, amsgrad: bool = False, maximize: bool = False, device: int = 0):
        h = C.c_void_p()
        check(lib().stg_adam_create(device, lr, b1, b2, eps, weight_decay, int(amsgrad), int(maximize), C.byref(h)))
        self._h = h
        self.device = device

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                lib().stg_adam_destroy(h)
            except Exception:
                pass
            self._h = None

    def name(self) -> str:
        return "Adam"

    def optimize_raw(self, param, name: str, grad, gidx, grad_len: int | None = None, d_grad_len=None) -> None:
        import torch
        n = int(grad_len if grad_len is not None else grad.numel())
        check(lib().stg_adam_optimize_raw_device(
            self._h, name.encode(), C.c_void_p(param.data_ptr()), param.numel(), C.c_void_p(grad.data_ptr()),
            C.c_void_p(gidx.data_ptr()), n, C.c_void_p(d_grad_len.data_ptr()) if d_grad_len is not None else None,
            C.c_void_p(torch.cuda.current_stream(param.device.index).cuda_stream)))

    def merge_optimize(self, param, name: str, idx, val, per_rank: int, world: int = 1, dense=None, mark=None,
                       out_idx=None, out_val=None, count=None):
        """ModuleCpuOptimize::run with Adam: the step inside the decompress's
        emission at world 1 without amsgrad, else the two calls."""
        return _merge_optimize(lib().stg_merge_optimize_adam_device, self._h, param, name, _decoded(idx, val), per_rank,
                               world, dense, mark, out_idx, out_val, count)

    def merge_optimize_wire(self, param, name: str, streams, per_rank: int, dense=None, mark=None, out_idx=None,
                            out_val=None, count=None):
        """``merge_optimize`` straight from received streams (see
        ``SparseSGD.merge_optimize_wire``)."""
        return _merge_optimize(lib().stg_merge_optimize_adam_wire_device, self._h, param, name,
                               (_rank_streams(streams, per_rank),), per_rank, len(streams), dense, mark, out_idx,
                               out_val, count)

    def merge_optimize_batch(self, items):
        """``merge_optimize_wire`` on every item in order, in one call (see
        ``SparseSGD.merge_optimize_batch``); with amsgrad every item runs one
        by one."""
        return _merge_optimize_batch(lib().stg_merge_optimize_adam_batch_device, self._h, items)

    def check_device(self) -> None:
        """Raise if a device-side failure was flagged (amsgrad look-back timeout)."""
        import torch
        check(lib().stg_adam_check(self._h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def state(self, name: str, n: int):
        """(m, v, vmax, tick) of a name, or None before its first call."""
        import torch
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
        vmax, tick = C.c_float(), C.c_uint32()
        rc = lib().stg_adam_get_state(self._h, name.encode(), C.c_void_p(m.ctypes.data), C.c_void_p(v.ctypes.data),
                                      n, C.byref(vmax), C.byref(tick),
                                      C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        return None if rc else (m, v, np.float32(vmax.value), int(tick.value))
