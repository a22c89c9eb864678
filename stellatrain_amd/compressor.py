"""Host-side mirror of the reference codec interface, over the HIP C-ABI.

Reference interface (``/root/reference/backend/src/compress/compressor.h:12-31``)::

    class Compressor {
        Compressor(std::unique_ptr<ThreadPool> &thread_pool, std::string name);
        const std::string &name();
        virtual size_t compress(const std::string &name, ConstSegment<float> src, uint32_t k,
                                Segment<uint32_t> dst_idx, Segment<float> dst_val,
                                int32_t idx_offset = 0) = 0;
    };

``ConstSegment``/``Segment`` (pointer, length) pairs become 1-D tensors or
arrays whose length is the segment length.  Device tensors run the
device-resident path on torch's current HIP stream; host tensors/arrays run
the host path (copy in, compress on the GPU, copy out).  ``compress`` returns
the reference's ``size_t`` (so it synchronises for device inputs);
``compress_async`` returns the count as a device tensor and never syncs.
Errors raise ``RuntimeError`` (``CodecError``), as the reference throws
``std::runtime_error`` (topk.cpp:34, core.cpp:117,193).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import (STG_DT_BF16, STG_DT_F16, STG_DT_F32, CodecError, StgBucket, StgGradSrc, StgSendTask, check,
                    lib)

__all__ = ["Compressor", "SendTasks", "ThresholdvCompressor16", "ThresholdvCompressor", "TopkCompressor", "make_compressor",
           "CodecError"]


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _stream_ptr(device: int) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def grad_dtype(t):
    """The ``STG_DT_*`` code of a gradient tensor's dtype (None: not one a gather reads)."""
    import torch
    return {torch.float32: STG_DT_F32, torch.bfloat16: STG_DT_BF16, torch.float16: STG_DT_F16}.get(t.dtype)


def typed_sources(what: str, grads, bucket):
    """The ``stg_grad_src_t`` array of a gather's ``grads`` for the
    ``*_typed_device`` entry points, or None when the fp32 entry point takes
    them: every tensor float32 and no separate ``bucket``.  ``grads[1:]`` may
    be float32, bfloat16 or float16; ``grads[0]`` too when ``bucket`` (the
    float32 tensor the sum is written to) is given -- it is then only read --
    and must be float32, the bucket itself, otherwise."""
    dts = [grad_dtype(g) for g in grads]
    if any(d is None for d in dts):
        raise ValueError(f"{what}: float32, bfloat16 or float16 gradients expected")
    if bucket is None:
        if dts[0] != STG_DT_F32:
            raise ValueError(f"{what}: a bfloat16 / float16 grads[0] needs a float32 bucket to be written to")
        if all(d == STG_DT_F32 for d in dts):
            return None
    arr = (StgGradSrc * len(grads))()
    for i, (g, d) in enumerate(zip(grads, dts)):
        if i or bucket is not None:  # ([0] stays null without a bucket: in place)
            arr[i] = StgGradSrc(g.data_ptr(), d)
    return arr


class SendTasks:
    """A prebuilt ``stg_send_task_t`` array: the iteration's sender-side tasks,
    marshalled and validated once and reused by every
    ``Compressor.merge_send_batch_async`` call on the same tensors (a model's
    gradient, residual and send buffers do not move between iterations).  Each
    item is ``(key, grads, k, dst_idx, dst_val, residual, wire_flag[,
    idx_offset[, bucket]])``: ``grads[0]`` is the bucket, ``residual`` may be
    None, the dst dtypes follow the flag (int16 / int32 indices, int16 / float32
    values).  ``grads[1:]`` may be float32, bfloat16 or float16 (16-bit model
    replicas' gradients, read as they are); with ``bucket``, a float32 tensor
    that receives the sum, ``grads[0]`` may be too and is only read.
    ``counts`` (int32, one per item) receives the pair counts of every call on
    the array.  The array keeps every tensor it points at alive, and the typed
    source arrays (``srcs``; None when every item is float32 in place)."""

    def __init__(self, items, counts=None):
        import torch
        items = list(items)
        self.count = len(items)
        self.array = (StgSendTask * max(self.count, 1))()
        self.srcs = None
        self.device = items[0][1][0].device if items and len(items[0]) > 1 and len(items[0][1]) else None
        self.counts = counts
        self._keep = []
        if not items:
            return
        dev = self.device
        if self.counts is None:
            self.counts = torch.zeros(self.count, dtype=torch.int32, device=dev)
        if self.counts.numel() < self.count or self.counts.dtype != torch.int32 or not self.counts.is_contiguous():
            raise ValueError("merge_send_batch: counts must be a contiguous int32 tensor, one element per item")
        for j, it in enumerate(items):
            if not 7 <= len(it) <= 9:
                raise ValueError(f"merge_send_batch: item {j}: (key, grads, k, dst_idx, dst_val, residual, wire_flag"
                                 "[, idx_offset]) expected")
            key, grads, k, di, dv, resid, flag = it[:7]
            off = int(it[7]) if len(it) > 7 else 0
            bucket = it[8] if len(it) > 8 else None
            flag = int(flag)
            grads = list(grads)
            if flag not in (0, 1, 2, 3):
                raise ValueError(f"merge_send_batch: item {j}: wire flag {flag!r} outside 0..3")
            if not 1 <= len(grads) <= 16:
                raise ValueError(f"merge_send_batch: item {j}: 1..16 gradient tensors expected")
            want = (torch.int16 if flag & 1 else torch.int32, torch.int16 if flag & 2 else torch.float32)
            if (di.dtype, dv.dtype) != want:
                raise ValueError(f"merge_send_batch: item {j}: dtypes {di.dtype}/{dv.dtype} do not match wire flag {flag}")
            if dv.numel() < di.numel():
                raise ValueError(f"merge_send_batch: item {j}: dst_val shorter than dst_idx")
            n = grads[0].numel()
            f32 = [t for t in (resid, bucket) if t is not None]
            srcs = grads + f32
            if any(t.numel() != n for t in srcs) or any(t.dtype != torch.float32 for t in f32) or \
                    any(grad_dtype(t) is None for t in grads):
                raise ValueError(f"merge_send_batch: item {j}: float32 gradients and residual of one size")
            typed = typed_sources(f"merge_send_batch: item {j}", grads, bucket)
            if not all(t.is_contiguous() for t in srcs + [di, dv]):
                raise ValueError(f"merge_send_batch: item {j}: tensors must be contiguous")
            if not all(t.is_cuda and t.device == dev for t in srcs + [di, dv, self.counts]):
                raise ValueError(f"merge_send_batch: item {j}: tensors must be on one HIP device")
            kb = key.encode()
            ptrs = None
            if typed is None:
                ptrs = (C.c_void_p * len(grads))(*[t.data_ptr() for t in grads])
            else:
                if self.srcs is None:
                    self.srcs = (C.POINTER(StgGradSrc) * self.count)()
                self.srcs[j] = typed
            b = StgBucket(kb, (grads[0] if bucket is None else bucket).data_ptr(), n, int(k), di.data_ptr(),
                          di.numel(), dv.data_ptr(), dv.numel(), off, self.counts.data_ptr() + 4 * j)
            self.array[j] = StgSendTask(b, resid.data_ptr() if resid is not None else None,
                                        ptrs if ptrs is not None and len(grads) > 1 else None, len(grads), flag)
            self._keep.append((kb, ptrs, typed, grads, di, dv, resid, bucket))


class Compressor:
    """Base class: one C-ABI codec handle (``stg_codec_create``)."""

    _method = ""

    def __init__(self, thread_pool=None, *, device: int = 0, method: str | None = None):
        # thread_pool: accepted for signature parity (compressor.h:26); the GPU
        # codec needs no host pool.
        self.thread_pool_ = thread_pool
        self.device = device
        self._method = method or self._method
        h = C.c_void_p()
        check(lib().stg_codec_create(self._method.encode(), device, C.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                lib().stg_codec_destroy(h)
            except Exception:
                pass
            self._h = None

    def name(self) -> str:
        """``Compressor::name()`` (compressor.h:28)."""
        return lib().stg_codec_name(self._h).decode()

    # -- compress ----------------------------------------------------------
    def compress(self, name: str, src, k: int, dst_idx, dst_val, idx_offset: int = 0) -> int:
        """``Compressor::compress`` (compressor.h:30); returns the pair count."""
        if _is_torch(src) and src.is_cuda:
            cnt = self.compress_async(name, src, k, dst_idx, dst_val, idx_offset)
            c = int(cnt.item())
            self.check_device()  # the synchronous form surfaces device-side failures as errors
            return c
        return self._compress_host(name, src, k, dst_idx, dst_val, idx_offset)

    def compress_async(self, name: str, src, k: int, dst_idx, dst_val, idx_offset: int = 0, count=None):
        """Device-resident compress on torch's current stream; returns a 1-element
        uint32-valued int32 tensor holding the count (no host sync)."""
        import torch
        assert src.is_cuda and dst_idx.is_cuda and dst_val.is_cuda, "device path needs device tensors"
        assert src.dtype == torch.float32 and dst_val.dtype == torch.float32
        assert dst_idx.dtype in (torch.int32, torch.uint32)
        assert src.is_contiguous() and dst_idx.is_contiguous() and dst_val.is_contiguous()
        if count is None:
            count = torch.empty(1, dtype=torch.int32, device=src.device)
        check(lib().stg_codec_compress_device(
            self._h, name.encode(), C.c_void_p(src.data_ptr()), src.numel(), int(k),
            C.c_void_p(dst_idx.data_ptr()), dst_idx.numel(), C.c_void_p(dst_val.data_ptr()), dst_val.numel(),
            int(idx_offset), C.c_void_p(count.data_ptr()), C.c_void_p(_stream_ptr(src.device.index))))
        return count

    def compress_raw(self, key: bytes, src_ptr: int, n: int, k: int, idx_ptr: int, cap: int, val_ptr: int,
                     count_ptr: int, stream_ptr: int, idx_offset: int = 0) -> None:
        """Lowest-overhead device call: raw device pointers, no validation
        beyond the C-ABI's own (for tight host loops such as bench.py)."""
        rc = self._fn_dev(self._h, key, src_ptr, n, k, idx_ptr, cap, val_ptr, cap, idx_offset, count_ptr, stream_ptr)
        if rc:
            check(rc)

    def compress_batch_async(self, items, stream=None, counts=None, residuals=None, wire_flags=None):
        """Batched device compress (``stg_codec_compress_batch_device``): the
        same results as ``compress_async`` on each (name, src, k, dst_idx,
        dst_val[, idx_offset]) in order, on one stream.  Returns a
        (len(items),) int32 tensor of counts (no host sync).  With
        ``residuals`` (one float32 tensor per item) it is the MERGE compress
        with error feedback (``stg_merge_compress_batch_device``,
        compress.cpp:139-186): every src is zeroed at its dst_idx slots and its
        residual receives the zeroed bucket.  With ``wire_flags`` (one STG_WIRE_*
        flag per item; thresholdv16) the emission writes each stream's wire form
        (``stg_codec_compress_wire_batch_device``, comm_manager.cpp:486-590):
        dst_idx is int16 under flag 1, dst_val float16-sized under flag 2, their
        numel the pair capacity."""
        import torch
        if not items:
            return None
        dev = items[0][1].device
        if counts is None:
            counts = torch.zeros(len(items), dtype=torch.int32, device=dev)
        arr = (StgBucket * len(items))()
        keep = []
        for j, it in enumerate(items):
            name, src, k, di, dv = it[:5]
            off = it[5] if len(it) > 5 else 0
            assert src.is_cuda and di.is_cuda and dv.is_cuda and src.dtype == torch.float32
            assert src.is_contiguous() and di.is_contiguous() and dv.is_contiguous()
            kb = name.encode()
            keep.append(kb)
            arr[j] = StgBucket(kb, src.data_ptr(), src.numel(), int(k), di.data_ptr(), di.numel(), dv.data_ptr(),
                               dv.numel(), int(off), counts.data_ptr() + 4 * j)
        sp = stream if stream is not None else _stream_ptr(dev.index)
        if wire_flags is not None:
            if residuals is not None or len(wire_flags) != len(items):
                raise ValueError("wire_flags: one flag per bucket, no residuals")
            fl = (C.c_int * len(items))(*[int(f) for f in wire_flags])
            check(lib().stg_codec_compress_wire_batch_device(self._h, arr, fl, len(items), C.c_void_p(sp)))
            return counts
        if residuals is None:
            check(lib().stg_codec_compress_batch_device(self._h, arr, len(items), C.c_void_p(sp)))
            return counts
        if len(residuals) != len(items):
            raise ValueError("one residual per bucket")
        rp = (C.c_void_p * len(items))()
        for j, (it, r) in enumerate(zip(items, residuals)):
            if r.numel() != it[1].numel() or r.dtype != torch.float32 or not r.is_contiguous() or not r.is_cuda:
                raise ValueError("residual must be a contiguous float32 device tensor of the bucket's size")
            rp[j] = r.data_ptr()
        check(lib().stg_merge_compress_batch_device(self._h, arr, rp, len(items), C.c_void_p(sp)))
        return counts

    def merge_gather_compress_async(self, name: str, grads, k: int, dst_idx, dst_val, residual=None,
                                    idx_offset: int = 0, count=None, stream=None, bucket=None):
        """One MERGE task with the intra-node gather ahead of it
        (``stg_merge_gather_compress_device``; cpu_gather.cpp:59-87, then
        compress.cpp:139-186): ``grads[0] += residual + grads[1] + ... +
        grads[N-1]`` (this rank's slices, left to right), compress grads[0]
        under ``name``, and with ``residual`` its error feedback.  thresholdv16
        sums the sources inside its streaming pass.  ``grads[1:]`` may be
        float32, bfloat16 or float16; with ``bucket`` (float32: it receives the
        sum and is what is compressed) ``grads[0]`` may be too and is only read
        (``stg_merge_gather_compress_typed_device``).  Returns the int32 count
        tensor (no host sync)."""
        import torch
        grads = list(grads)
        f32 = [t for t in (residual, bucket) if t is not None]
        g0 = grads[0] if bucket is None else bucket
        n = g0.numel()
        for t in grads + f32 + [dst_idx, dst_val]:
            if not (t.is_cuda and t.is_contiguous()):
                raise ValueError("merge_gather_compress: contiguous device tensors")
        if any(t.numel() != n for t in grads + f32) or any(t.dtype != torch.float32 for t in f32) or \
                any(grad_dtype(t) is None for t in grads):
            raise ValueError("merge_gather_compress: float32 sources of one size")
        typed = typed_sources("merge_gather_compress", grads, bucket)
        if count is None:
            count = torch.zeros(1, dtype=torch.int32, device=g0.device)
        kb = name.encode()
        b = StgBucket(kb, g0.data_ptr(), n, int(k), dst_idx.data_ptr(), dst_idx.numel(), dst_val.data_ptr(),
                      dst_val.numel(), int(idx_offset), count.data_ptr())
        sp = stream if stream is not None else _stream_ptr(g0.device.index)
        rp = C.c_void_p(residual.data_ptr()) if residual is not None else None
        if typed is not None:
            check(lib().stg_merge_gather_compress_typed_device(self._h, C.byref(b), rp, typed, len(grads),
                                                               C.c_void_p(sp)))
            return count
        ptrs = (C.c_void_p * len(grads))(*[t.data_ptr() for t in grads])
        check(lib().stg_merge_gather_compress_device(self._h, C.byref(b), rp, ptrs, len(grads), C.c_void_p(sp)))
        return count

    def merge_send_batch_async(self, items, stream=None, counts=None):
        """The sender half of a MERGE iteration in one call
        (``stg_merge_send_batch_device``): for every item ``(key, grads, k,
        dst_idx, dst_val, residual, wire_flag[, idx_offset])`` the gather-add
        ``grads[0] += residual + grads[1] + ... + grads[N-1]``, the compress of
        ``grads[0]`` under ``key`` with its error feedback (``residual`` not
        None: the selected entries zeroed by their true indices, the residual
        left equal to the bucket) and the stream written in its wire form --
        bitwise ``merge_gather_compress_async`` into u32 / f32 temporaries
        followed by ``wire_encode`` of the count = min(dst_idx.numel(), n)
        pairs.  ``dst_idx`` is int16 under flag 1 (else int32), ``dst_val``
        int16-typed fp16 bits under flag 2 (else float32); ``dst_idx.numel()``
        is the pair capacity.  Keys must be distinct within a call.
        thresholdv16, threshold-v and exact top-k (the shipped ``"topk"``:
        ``CodecError``, unsupported -- it writes ``idx[i] = i``, so there are
        no true indices to zero).
        On a ``TopkCompressor(exact=True)`` the key is ``key``, the count is
        ``dst_idx.numel()`` (topk.cpp:25; it must be at least ``k``), the
        first ``min(k, n)`` wire slots are the winners in index order (ties at
        the k-th magnitude taken in index order) and slots ``[min(k, n), W)``,
        ``W = min(dst_idx.numel(), n)``, the wire form of ``(0, 0.0)``; with
        ``residual`` element 0 is zeroed whenever ``min(k, n) <
        dst_idx.numel()``.  Batched and per-tensor calls on one key may
        interleave in any order.
        On a ``ThresholdvCompressor`` the key is the pointer of the bucket
        (``key`` is ignored) and the count varies, ``min(qualifiers,
        dst_idx.numel())``, while the engine sends all ``W =
        min(dst_idx.numel(), n)`` slots (compress.cpp:60-64): the first
        ``count`` wire slots are the pairs, slots ``[count, W)`` the wire form
        of ``(0, 0.0)``, the block / tail split of the packing at ``8 * ((W -
        1) // 8)``, nothing past ``W`` written; with ``residual``, grad and
        residual are zeroed at the true index of all ``W`` slots -- element 0
        whenever ``count < W``.  That is ``merge_gather_compress_async`` into
        zeroed temporaries, then ``wire_encode`` of their first ``W`` slots.
        ``items`` may be a prebuilt ``SendTasks``; an item
        may carry bfloat16 / float16 gradients and a trailing ``bucket`` as
        described there (``stg_merge_send_batch_typed_device``).  Returns
        the int32 counts tensor (no host sync)."""
        tasks = items if isinstance(items, SendTasks) else SendTasks(items, counts=counts)
        if not tasks.count:
            return tasks.counts
        sp = stream if stream is not None else _stream_ptr(tasks.device.index)
        if tasks.srcs is not None:
            check(lib().stg_merge_send_batch_typed_device(self._h, tasks.array, tasks.srcs, tasks.count,
                                                          C.c_void_p(sp)))
            return tasks.counts
        f = getattr(self, "_fn_send_cache", None)
        if f is None:
            f = self._fn_send_cache = lib().stg_merge_send_batch_device
        rc = f(self._h, tasks.array, tasks.count, C.c_void_p(sp))
        if rc:
            check(rc)
        return tasks.counts

    @staticmethod
    def bucket_array(rows):
        """Prebuilt ``stg_bucket_t`` array from raw tuples (key bytes, src_ptr,
        n, k, idx_ptr, cap, val_ptr, count_ptr[, idx_offset]) for tight loops."""
        arr = (StgBucket * len(rows))()
        for j, r in enumerate(rows):
            arr[j] = StgBucket(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[5], r[8] if len(r) > 8 else 0, r[7])
        return arr

    def compress_batch_raw(self, arr, nb: int, stream_ptr: int) -> None:
        """Batched call on a prebuilt ``bucket_array`` (no per-call marshalling)."""
        f = getattr(self, "_fn_batch_cache", None)
        if f is None:
            f = self._fn_batch_cache = lib().stg_codec_compress_batch_device
        rc = f(self._h, arr, nb, stream_ptr)
        if rc:
            check(rc)

    @property
    def _fn_dev(self):
        f = getattr(self, "_fn_dev_cache", None)
        if f is None:
            f = self._fn_dev_cache = lib().stg_codec_compress_device
        return f

    def _compress_host(self, name, src, k, dst_idx, dst_val, idx_offset) -> int:
        s = src.numpy() if _is_torch(src) else src
        di = dst_idx.numpy() if _is_torch(dst_idx) else dst_idx
        dv = dst_val.numpy() if _is_torch(dst_val) else dst_val
        if not (isinstance(s, np.ndarray) and s.dtype == np.float32 and s.flags.c_contiguous):
            raise TypeError("src must be a contiguous float32 array/tensor")
        if di.dtype.itemsize != 4 or dv.dtype != np.float32 or not di.flags.c_contiguous or not dv.flags.c_contiguous:
            raise TypeError("dst_idx must be contiguous (u)int32 and dst_val contiguous float32")
        out = C.c_size_t()
        check(lib().stg_codec_compress_host(
            self._h, name.encode(), C.c_void_p(s.ctypes.data), s.size, int(k), C.c_void_p(di.ctypes.data),
            di.size, C.c_void_p(dv.ctypes.data), dv.size, int(idx_offset), C.byref(out)))
        return int(out.value)

    # -- introspection (tests) ----------------------------------------------
    def state(self, name: str = "", key_ptr: int = 0, stream=None):
        """Per-key AIMD state (threshold, threshold_inc) or None if never seen."""
        t, inc = C.c_float(), C.c_float()
        sp = stream if stream is not None else 0
        rc = lib().stg_codec_get_state(self._h, name.encode(), C.c_void_p(key_ptr), C.byref(t), C.byref(inc),
                                       C.c_void_p(sp))
        if rc != 0:
            return None
        return t.value, inc.value

    def set_timing(self, enable: bool) -> None:
        check(lib().stg_codec_set_timing(self._h, int(enable)))

    def get_timing(self):
        """(scan_ms, fill_ms, call_ms) accumulated since the last read, and calls."""
        ms = (C.c_double * 3)()
        calls = C.c_uint64()
        check(lib().stg_codec_get_timing(self._h, ms, C.byref(calls)))
        return (ms[0], ms[1], ms[2]), int(calls.value)

    def check_device(self) -> None:
        check(lib().stg_codec_check(self._h))


class ThresholdvCompressor16(Compressor):
    """``ThresholdvCompressor16(std::unique_ptr<ThreadPool>&, bool multicore=true)``
    (thresholdv16.h:33-34); per-name AIMD state (thresholdv16.cpp:81-97)."""

    _method = "thresholdv16"

    def __init__(self, thread_pool=None, multicore: bool = True, *, device: int = 0):
        self.multicore_ = multicore  # never read by the reference either
        super().__init__(thread_pool, device=device)


class ThresholdvCompressor(Compressor):
    """``ThresholdvCompressor(std::unique_ptr<ThreadPool>&, bool multicore=true)``
    (thresholdv.h:24-25); AIMD state keyed by the src pointer (thresholdv.cpp:44)."""

    _method = "thresholdv"

    def __init__(self, thread_pool=None, multicore: bool = True, *, device: int = 0):
        self.multicore_ = multicore
        super().__init__(thread_pool, device=device)


class TopkCompressor(Compressor):
    """``TopkCompressor(std::unique_ptr<ThreadPool>&)`` (topk.h:28-29).  ``exact=False``
    keeps the shipped behaviour (byte-count memcpy, idx 0..k-1: topk.cpp:31,42);
    ``exact=True`` is the intended top-k by |x| with real indices."""

    _method = "topk"

    def __init__(self, thread_pool=None, *, exact: bool = False, device: int = 0):
        super().__init__(thread_pool, device=device, method="topk_exact" if exact else "topk")


def make_compressor(method: str, thread_pool=None, *, device: int = 0) -> Compressor:
    """Factory of FasterDpEngine::configure (core.cpp:110-118)."""
    if method == "thresholdv":
        return ThresholdvCompressor(thread_pool, True, device=device)
    if method == "thresholdv16":
        return ThresholdvCompressor16(thread_pool, True, device=device)
    if method == "topk":
        return TopkCompressor(thread_pool, device=device)
    if method == "topk_exact":
        return TopkCompressor(thread_pool, exact=True, device=device)
    raise CodecError(-2, f"Unknown compression method {method}.")
