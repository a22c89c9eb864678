"""stellatrain_amd -- MI355X-native gradient-sparsification codec.

A drop-in for StellaTrain's CPU compress path (backend/src/compress): the
thresholdv16 / threshold-v / Top-k codecs, the MERGE decompress and the
sparse SGD apply, as hand-written HIP kernels for gfx950 behind the C-ABI in
include/stg/codec.h.  See DESIGN.md.
"""
from ._capi import (CodecError, StgGradSrc, StgMergeTask, StgPublishTask, StgReplica, StgSendTask,  # noqa: F401
                    lib)
from .compressor import (Compressor, SendTasks, ThresholdvCompressor, ThresholdvCompressor16,  # noqa: F401
                         TopkCompressor, make_compressor)
from .engine import (CodecEngine, MergeTasks, PublishTasks, SparseAdam, SparseSGD, api_numel, merge_numel, owner_of,  # noqa: F401
                     gather_add, gather_slice, merge_batch_launches, publish_params, scatter_merge, scatter_merge_wire, wire_decode, wire_decode_batch,
                     wire_encode, wire_encode_batch, wire_flag)

__version__ = "0.1.0"
