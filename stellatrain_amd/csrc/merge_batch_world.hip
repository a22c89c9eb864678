// merge_batch_world.hip -- the world > 1 MERGE decompress (apply.hip:
// scatter_mark[_w], mark_count, mark_scan, mark_emit_tile) with the optimizer
// step fused into its emission, for up to MERGE_BATCH parameter tensors per
// launch (gfx950).
//
// A lone world > 1 task is world + 1 scatter launches, three launches of the
// mark emission and the step: world + 5 launches for, typically, a few KB of
// traffic.  Here the tensors of a group (the same world, all with pairs) share
// world + 4:
//   * launches r = 0 .. world: every tensor scatters rank r - 1 and elects rank
//     r, on the parity halves of its own winner words.  The launch's table
//     (MergeScatterArgs) carries only the two ranks it reads.  One launch per
//     rank, stream-ordered, so dense[j] = (((0 + v0) + v1) + ...) in rank order
//     exactly as the per-tensor launches leave it;
//   * the per-tile mark counts of every tensor;
//   * their scan, one workgroup per tensor, which also writes the tensor's count;
//   * the emission: per tile of MERGE_TILE marks the marked indices in order at
//     the tile's prefix, value dense / world, and sgd_step / adam_step on each
//     emitted pair.  The union holds each index once, so the updates commute
//     with the separate step over the merged stream, and a plain load of the
//     last-touched word reads what sgd_apply<true>'s exchange would.
// A workgroup learns its tensor from blockIdx (blk0, host-computed) and works on
// that tensor's slices of the library's scratch: 2 n winner words, n dense
// floats, n mark bytes, each slice on a 16-byte boundary (MergeWorldTensor::off
// is a multiple of 16 elements), all zero between calls: the winners re-zero
// their words as they scatter, the emission re-zeroes dense and marks.
//
// No workgroup waits for another: launch boundaries are the only ordering, and
// every barrier is reached by the whole workgroup.
//
// The per-element code is wire_dev.h (the loaders, which take flag 0 as well)
// and merge_dev.h (load_marks, nz_bytes, Step, sgd_step, adam_step), the text
// the per-tensor kernels compile, so parameters, state and merged streams agree
// with them bitwise.
#include "ws.h"
#include "wire_dev.h"
#include "merge_dev.h"

namespace stg {

namespace {

// Launch r of the group: threads [0, m) of a tensor scatter its rank r - 1 (the
// winners only; sidx null at r = 0), threads [m, 2m) elect its rank r (midx
// null at r = world).  One thread per pair, STG_WG per workgroup.
__global__ void __launch_bounds__(STG_WG) merge_world_scatter(MergeScatterArgs w) {
    const uint32_t t = batch_item(w.t, w.nt);
    const MergeScatterTensor &d = w.t[t];
    const size_t m = d.m, n = d.n;
    const size_t wend = 8 * ((m - 1) / 8);  // m >= 1
    const size_t p = (size_t)(blockIdx.x - d.blk0) * STG_WG + threadIdx.x;
    uint32_t *__restrict__ win = w.win + 2 * (size_t)d.off;
    if (p < m) {
        if (!d.sidx) return;
        uint32_t *__restrict__ swin = win + (size_t)((w.rank - 1u) & 1u) * n;
        const uint32_t j = wire_get_idx(d.sidx, d.sflag, wend, p);
        if (j >= n || swin[j] != (uint32_t)p + 1u) return;  // dropped, or a later occurrence wins
        swin[j] = 0;
        w.dense[(size_t)d.off + j] += wire_get_val(d.sval, d.sflag, wend, p);
        w.mark[(size_t)d.off + j] = 1;
    } else if (p < 2 * m) {
        if (!d.midx) return;
        uint32_t *__restrict__ mwin = win + (size_t)(w.rank & 1u) * n;
        const size_t i = p - m;
        const uint32_t j = wire_get_idx(d.midx, d.mflag, wend, i);
        if (j < n) atomicMax(&mwin[j], (uint32_t)i + 1u);
    }
}

// A tensor's tile counts and, behind them, their exclusive prefixes: 2 ntiles
// words at 2 blk0 (blk0 = the tiles of the tensors before it).
__device__ __forceinline__ uint32_t *tile_slice(const MergeWorldArgs &w, const MergeWorldTensor &d) {
    return w.tiles + 2 * (size_t)d.blk0;
}
__device__ __forceinline__ uint32_t tiles_of(const MergeWorldTensor &d) {
    return (uint32_t)(((size_t)d.n + MERGE_TILE - 1) / MERGE_TILE);
}

// mark_count per tensor: one workgroup per MERGE_TILE marks.
__global__ void __launch_bounds__(STG_WG) merge_world_count(MergeWorldArgs w) {
    __shared__ uint32_t s[STG_WAVES];
    const uint32_t t = batch_item(w.t, w.nt);
    const MergeWorldTensor &d = w.t[t];
    const uint32_t tile = blockIdx.x - d.blk0;
    const size_t e = (size_t)tile * MERGE_TILE + 16 * threadIdx.x;
    const uint4 v = load_marks(w.mark + d.off, d.n, e);
    uint32_t c = nz_bytes(v.x) + nz_bytes(v.y) + nz_bytes(v.z) + nz_bytes(v.w);
    c = wave_sum(c);
    if (__lane_id() == 0) s[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t q = 0; q < STG_WAVES; ++q) sum += s[q];
        tile_slice(w, d)[tile] = sum;
    }
}

// mark_scan per tensor: workgroup t scans tensor t's tile counts (1,024
// threads, 4 tiles per thread per round) and writes its count.
__global__ void __launch_bounds__(1024) merge_world_scan(MergeWorldArgs w) {
    __shared__ uint32_t sh[16 + 1];
    const MergeWorldTensor &d = w.t[blockIdx.x];
    uint32_t *__restrict__ tile_cnt = tile_slice(w, d);
    const uint32_t ntiles = tiles_of(d);
    uint32_t run = 0;
    for (uint32_t t0 = 0; t0 < ntiles; t0 += 4 * 1024) {  // uniform trip count
        const uint32_t tb = t0 + 4 * threadIdx.x;
        uint32_t c[4], sum = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) { c[q] = tb + q < ntiles ? tile_cnt[tb + q] : 0u; sum += c[q]; }
        uint32_t tot;
        uint32_t p = run + blk_excl_scan<16>(sum, sh, &tot);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
            if (tb + q < ntiles) { tile_cnt[ntiles + tb + q] = p; p += c[q]; }
        run += tot;
    }
    if (threadIdx.x == 0) *d.out_count = run;
}

// mark_emit_tile per tensor with the step on every emitted pair; dense and
// marks zeroed behind it.  A lane's 16 marks and 16 dense values are one uint4
// and four float4 loads (the slices start 16-byte aligned).
template <int OPT>
__global__ void __launch_bounds__(STG_WG) merge_world_emit(MergeWorldArgs w) {
    __shared__ uint32_t sh[STG_WAVES + 1];
    const uint32_t tid = threadIdx.x;
    const uint32_t t = batch_item(w.t, w.nt);
    const MergeWorldTensor &d = w.t[t];
    const uint32_t tile = blockIdx.x - d.blk0;
    const size_t n = d.n;
    const uint32_t *__restrict__ tile_cnt = tile_slice(w, d);
    const bool any = tile_cnt[tile] != 0;  // uniform: anything marked in this tile
    const uint64_t P = tile_cnt[tiles_of(d) + tile];
    uint8_t *__restrict__ mark = w.mark + d.off;
    float *__restrict__ dense = w.dense + d.off;
    const size_t e = (size_t)tile * MERGE_TILE + 16 * tid;
    const uint4 v = any ? load_marks(mark, n, e) : make_uint4(0u, 0u, 0u, 0u);
    const uint32_t words[4] = {v.x, v.y, v.z, v.w};
    const uint32_t c = nz_bytes(v.x) + nz_bytes(v.y) + nz_bytes(v.z) + nz_bytes(v.w);
    const bool full = e + 16 <= n;
    float dv[16];
    if (c && full) {
        const float4 *p = reinterpret_cast<const float4 *>(dense + e);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const float4 x = p[q];
            dv[4 * q] = x.x; dv[4 * q + 1] = x.y; dv[4 * q + 2] = x.z; dv[4 * q + 3] = x.w;
        }
    }
    uint32_t tc;
    uint32_t r = wg_excl_scan(c, sh, &tc);  // every lane of the workgroup arrives
    if (!c) return;
    const Step<OPT> opt(w, d);
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b) {
        if ((words[b >> 2] >> (8 * (b & 3))) & 0xffu) {
            const size_t j = e + b;
            const float g = (full ? dv[b] : dense[j]) / w.world;  // merged_grad[j] (cpu_optimize.cpp:49-55)
            d.out_idx[P + r] = (uint32_t)j;
            d.out_val[P + r] = g;
            float x, m0, f;
            uint32_t l;
            opt.load((uint32_t)j, x, m0, f, l);
            opt.factors(f, l);
            opt.step((uint32_t)j, g, x, m0, f, l);  // the union holds j once: updates commute
            if (!full) { dense[j] = 0.f; mark[j] = 0; }
            ++r;
        }
    }
    if (full) {  // leave the scratch zeroed for the next call
        float4 *p = reinterpret_cast<float4 *>(dense + e);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) p[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<uint4 *>(mark + e) = make_uint4(0u, 0u, 0u, 0u);
    }
}

}  // namespace

hipError_t launch_merge_world_scatter(const MergeScatterArgs &w, uint32_t blocks, hipStream_t s, uint64_t *launches) {
    if (!w.nt || !blocks) return hipSuccess;
    merge_world_scatter<<<blocks, STG_WG, 0, s>>>(w);
    count_launch(launches);
    return hipGetLastError();
}

hipError_t launch_merge_world_emit(const MergeWorldArgs &w, uint32_t blocks, int opt, hipStream_t s,
                                   uint64_t *launches) {
    if (!w.nt || !blocks) return hipSuccess;
    merge_world_count<<<blocks, STG_WG, 0, s>>>(w);
    count_launch(launches);
    merge_world_scan<<<w.nt, 1024, 0, s>>>(w);
    count_launch(launches);
    if (opt == 2) merge_world_emit<2><<<blocks, STG_WG, 0, s>>>(w);
    else if (opt == 1) merge_world_emit<1><<<blocks, STG_WG, 0, s>>>(w);
    else merge_world_emit<0><<<blocks, STG_WG, 0, s>>>(w);
    count_launch(launches);
    return hipGetLastError();
}

}  // namespace stg
