// send_batch.hip -- the sender half of a MERGE iteration in one call (gfx950):
// the two streaming kernels of stg_merge_send_batch_device around the
// thresholdv16 scans.
//
// Per parameter tensor the reference runs ModuleCpuGather::run
// (engine/modules/cpu_gather.cpp:59-87), ModuleCompress::run with its error
// feedback (engine/modules/compress.cpp:139-186) and queueTx's packing
// (engine/comm_manager.cpp:486-590).  The per-tensor entry points spend one
// gather launch, one ef_zero launch (plus a tail copy) and a share of an encode
// launch on each tensor; here up to SEND_BATCH tensors share
//   gather_add_batch : grad[0] += residual + grad[1] + ... + grad[N-1]
//   (the thresholdv16 scans, unchanged, into u32 / f32 staging; residual copy fused)
//   ef_pack_batch    : ragged tail -> residual, zero the selected entries by
//                      their TRUE indices, write the wire form of every pair
// On a threshold-v handle the scans are tv_batch.hip's (residual copy fused
// there too) and the finish is
//   ef_pack_batch_dc : the pair count read from the device; all min(idx_cap,
//                      n) slots written, the unused ones as (0, 0.0f)
// Workgroups are dealt to the tensors by host-computed first-workgroup offsets
// (blk0), as in wire_encode_batch.  These kernels are plain streaming code:
// nothing waits on another workgroup and no LDS is used.
//
// Bounds.  gather_add_batch: HBM (xGMI for peer sources), 4 (dst) + 4
// (residual) + 4 (N - 1) + 4 (store) bytes per element, float4 lanes with
// nontemporal source loads; gather_add_batch_typed reads bf16 / fp16 sources
// as they are, 2 bytes per element each (lane groups of 8 or 4 elements), and
// the first term from a typed source when the task has one.  ef_pack_batch: k
// pairs per tensor (1 % of it), one pair per lane, so the launch is
// latency-bound like wire_encode.
#include <algorithm>

#include "ws.h"
#include "gather_dev.h"
#include "wire_dev.h"

namespace stg {

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

// (the per-element sum is gather.hip's, in its order -- dst, residual,
// grad[1], ... -- from gather_dev.h)
//
// A workgroup owns SEND_GATHER_TILE elements of its task.  Where every pointer
// of the task shares one 16-byte phase (a.vec) the tile is four float4 per lane
// counted from the first aligned element, every source's float4 loaded before
// any is added (as gather_add_vec<MAXS>; MAXS >= the launch's largest nsrc),
// and the task's first workgroup adds the scalar head (< 4 elements before the
// aligned start) and tail (< 4 after the last float4) as well.  Otherwise the
// tile is scalar.  Every element is read and written by exactly one lane.
template <uint32_t MAXS>
__global__ void __launch_bounds__(STG_WG) gather_add_batch(SendGatherBatch w) {
    const SendGather &a = w.t[batch_item(w.t, w.nt)];
    const size_t wb = blockIdx.x - a.blk0;
    if (!a.vec) {
        for (uint32_t u = 0; u < SEND_GATHER_TILE / STG_WG; ++u) {
            const size_t e = wb * SEND_GATHER_TILE + u * STG_WG + threadIdx.x;
            if (e < a.n) gather_elem<false>(a, e);
        }
        return;
    }
    const size_t v0 = a.head, nv = (a.n - v0) / 4;
    for (uint32_t u = 0; u < SEND_GATHER_TILE / 4 / STG_WG; ++u) {
        const size_t i = wb * (SEND_GATHER_TILE / 4) + u * STG_WG + threadIdx.x;
        if (i >= nv) break;
        const size_t e = v0 + 4 * i;
        f4v x[MAXS];
        f4v acc = *reinterpret_cast<const f4v *>(a.dst + e);
        const f4v r = a.resid ? __builtin_nontemporal_load(reinterpret_cast<const f4v *>(a.resid + e)) : f4v{0, 0, 0, 0};
#pragma unroll
        for (uint32_t s = 1; s < MAXS; ++s)
            if (s < a.nsrc)
                x[s] = __builtin_nontemporal_load(reinterpret_cast<const f4v *>(static_cast<const float *>(a.src[s]) + e));
        if (a.resid) acc += r;
#pragma unroll
        for (uint32_t s = 1; s < MAXS; ++s)
            if (s < a.nsrc) acc += x[s];
        *reinterpret_cast<f4v *>(a.dst + e) = acc;
    }
    if (wb == 0) {
        const size_t vt = v0 + 4 * nv, ns = v0 + (a.n - vt);  // head + tail elements: at most 6
        if (threadIdx.x < ns) gather_elem<false>(a, threadIdx.x < v0 ? threadIdx.x : vt + (threadIdx.x - v0));
    }
}

// The same for tables with a 16-bit source or a typed first term (a.dtypes,
// a.src[0]; gather_dev.h): a.vec is the task's lane-group width W (ws.h
// GatherPlan) -- the tile is SEND_GATHER_TILE / W groups counted from a.head,
// head (< W) and tail (< W) scalar in the task's first workgroup -- or 0 for a
// scalar tile.  The width is uniform over the workgroup.
template <uint32_t MAXS, uint32_t W>
__device__ __forceinline__ void gather_typed_tile(const SendGather &a, size_t wb) {
    const size_t v0 = a.head, nv = (a.n - v0) / W;
    for (uint32_t u = 0; u < SEND_GATHER_TILE / W / STG_WG; ++u) {
        const size_t i = wb * (SEND_GATHER_TILE / W) + u * STG_WG + threadIdx.x;
        if (i >= nv) break;
        gather_lane<MAXS, W>(a, v0 + W * i);
    }
    if (wb == 0) {
        const size_t vt = v0 + W * nv, ns = v0 + (a.n - vt);  // head + tail elements: at most 2 (W - 1)
        if (threadIdx.x < ns) gather_elem<true>(a, threadIdx.x < v0 ? threadIdx.x : vt + (threadIdx.x - v0));
    }
}

template <uint32_t MAXS>
__global__ void __launch_bounds__(STG_WG) gather_add_batch_typed(SendGatherBatch w) {
    const SendGather &a = w.t[batch_item(w.t, w.nt)];
    const size_t wb = blockIdx.x - a.blk0;
    if (a.vec == 8) {
        gather_typed_tile<MAXS, 8>(a, wb);
    } else if (a.vec == 4) {
        gather_typed_tile<MAXS, 4>(a, wb);
    } else {
        for (uint32_t u = 0; u < SEND_GATHER_TILE / STG_WG; ++u) {
            const size_t e = wb * SEND_GATHER_TILE + u * STG_WG + threadIdx.x;
            if (e < a.n) gather_elem<true>(a, e);
        }
    }
}

// The finish of a task after its scan: pair j of the staged u32 / f32 stream
// belongs to lane j of the task's workgroups, which writes its wire form
// (wire_idx16 / wire_val16 by position against simd_end = 8 * ((count - 1) /
// 8), the split wire.hip makes) and, under error feedback (resid != null),
// zeroes grad and residual at the pair's true index.
//
// The ragged tail grad[n / 16 * 16 .. n) is not streamed to the residual by
// the fused scan, so it is copied here -- a read of elements this launch may
// also zero.  Scheme: ALL accesses to tail elements belong to the task's first
// workgroup.  It copies the tail, passes a __syncthreads() (the copy's loads
// and stores are complete and ordered before what follows in the workgroup),
// and then alone walks the task's count indices and zeroes those at or past
// n / 16 * 16; every workgroup skips such indices in the general pass.  No
// other workgroup reads or writes a tail element, so there is no race and no
// wait between workgroups.  Only ragged tasks pay the extra walk.  Elements
// below the tail are only ever written (zeros, possibly by several lanes) in
// this launch, and the staged stream is only read.
//
// The reference's unused slots hold index 0 (compress.cpp:60-64,178-179): when
// idx_cap > count (d.zero0) element 0 is zeroed too, by the first workgroup
// after the barrier (element 0 is a tail element when n < 16).
__global__ void __launch_bounds__(STG_WG) ef_pack_batch(SendFinishBatch w) {
    const SendFinish &d = w.t[batch_item(w.t, w.nt)];
    const uint32_t wb = blockIdx.x - d.blk0;
    const size_t full = d.n / 16 * 16;
    const bool ef = d.resid != nullptr;
    const size_t j = (size_t)wb * STG_WG + threadIdx.x;
    if (j < d.count) {
        const size_t wend = 8 * ((size_t)(d.count - 1) / 8);
        const uint32_t ix = d.idx[j];
        const float v = d.val[j];
        if (d.flag & 1u) static_cast<uint16_t *>(d.idx_out)[j] = (uint16_t)wire_idx16(ix, j, wend);
        else static_cast<uint32_t *>(d.idx_out)[j] = ix;
        if (d.flag & 2u) static_cast<uint16_t *>(d.val_out)[j] = (uint16_t)wire_val16(v, j, wend);
        else static_cast<float *>(d.val_out)[j] = v;
        if (ef && ix < full) {
            d.grad[ix] = 0.f;
            d.resid[ix] = 0.f;
        }
    }
    if (wb != 0 || !ef) return;
    if (full + threadIdx.x < d.n) d.resid[full + threadIdx.x] = d.grad[full + threadIdx.x];  // (n - full < 16)
    __syncthreads();
    if (full < d.n) {
        for (uint32_t q = threadIdx.x; q < d.count; q += STG_WG) {
            const uint32_t ix = d.idx[q];
            if (ix >= full && ix < d.n) {
                d.grad[ix] = 0.f;
                d.resid[ix] = 0.f;
            }
        }
    }
    if (d.zero0 && threadIdx.x == 0) {
        d.grad[0] = 0.f;
        d.resid[0] = 0.f;
    }
}

// The finish of a threshold-v task (tv_batch.hip's scan, or tv_pass for a task
// that ran alone): the pair count is the task's device word.  The engine sends
// all W = min(idx_cap, n) slots, the unused ones holding (index 0, value 0.0)
// (compress.cpp:60-64): lane j < W writes the wire form of staged pair j when
// j < count and of (0, 0.0f) otherwise, by position against wend = 8 * ((W -
// 1) / 8); under error feedback it zeroes grad and residual at the pair's true
// index, and at element 0 for an unused slot (compress.cpp:178-179).  A
// poisoned count writes nothing and zeroes nothing.  The scan copied the whole
// bucket to the residual, so every element is only ever written (zeros) here:
// no ragged-tail case, no order between workgroups.
__global__ void __launch_bounds__(STG_WG) ef_pack_batch_dc(SendFinishDcBatch w) {
    const SendFinishDc &d = w.t[batch_item(w.t, w.nt)];
    const uint32_t wb = blockIdx.x - d.blk0;
    const size_t j = (size_t)wb * STG_WG + threadIdx.x;
    const uint32_t count = *d.count;
    if (count == POISON_COUNT || j >= d.slots) return;
    const size_t wend = 8 * ((size_t)(d.slots - 1) / 8);
    const bool pair = j < count;
    const uint32_t ix = pair ? d.idx[j] : 0u;
    const float v = pair ? d.val[j] : 0.f;
    if (d.flag & 1u) static_cast<uint16_t *>(d.idx_out)[j] = (uint16_t)wire_idx16(ix, j, wend);
    else static_cast<uint32_t *>(d.idx_out)[j] = ix;
    if (d.flag & 2u) static_cast<uint16_t *>(d.val_out)[j] = (uint16_t)wire_val16(v, j, wend);
    else static_cast<float *>(d.val_out)[j] = v;
    if (d.resid && ix < d.n && (pair || j == count)) {  // (one lane of the unused slots zeroes element 0)
        d.grad[ix] = 0.f;
        d.resid[ix] = 0.f;
    }
}

}  // namespace

hipError_t launch_ef_pack_batch_dc(const SendFinishDcBatch &w, uint32_t blocks, hipStream_t s) {
    if (!w.nt || !blocks) return hipSuccess;
    ef_pack_batch_dc<<<blocks, STG_WG, 0, s>>>(w);
    return hipGetLastError();
}

hipError_t launch_gather_add_batch(const SendGatherBatch &w, uint32_t blocks, hipStream_t s) {
    if (!w.nt || !blocks) return hipSuccess;
    uint32_t maxs = 1;
    for (uint32_t i = 0; i < w.nt; ++i) maxs = std::max(maxs, w.t[i].nsrc);
    if (maxs <= 4) gather_add_batch<4><<<blocks, STG_WG, 0, s>>>(w);
    else if (maxs <= 8) gather_add_batch<8><<<blocks, STG_WG, 0, s>>>(w);
    else gather_add_batch<GATHER_MAX><<<blocks, STG_WG, 0, s>>>(w);
    return hipGetLastError();
}

hipError_t launch_gather_add_batch_typed(const SendGatherBatch &w, uint32_t blocks, hipStream_t s) {
    if (!w.nt || !blocks) return hipSuccess;
    uint32_t maxs = 1;
    for (uint32_t i = 0; i < w.nt; ++i) maxs = std::max(maxs, w.t[i].nsrc);
    if (maxs <= 4) gather_add_batch_typed<4><<<blocks, STG_WG, 0, s>>>(w);
    else if (maxs <= 8) gather_add_batch_typed<8><<<blocks, STG_WG, 0, s>>>(w);
    else gather_add_batch_typed<GATHER_MAX><<<blocks, STG_WG, 0, s>>>(w);
    return hipGetLastError();
}

hipError_t launch_ef_pack_batch(const SendFinishBatch &w, uint32_t blocks, hipStream_t s) {
    if (!w.nt || !blocks) return hipSuccess;
    ef_pack_batch<<<blocks, STG_WG, 0, s>>>(w);
    return hipGetLastError();
}

}  // namespace stg
