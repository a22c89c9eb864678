// merge_grad.hip -- MERGE decompress of `world` rank streams into the dense
// averaged gradient a torch.optim class reads: float32, bfloat16 or float16,
// overwritten over all of [0, n) or accumulated at the union (gfx950).
//
// The pairs are bucketed by merge_sparse.hip's three launches (count, scan,
// place; the batched ones for a group), so scratch and bucketing work follow
// the pairs.  One emission launch replaces the union count, its scan and the
// union emission:
//
//   tb_dense<DT, ACC>  one workgroup per tile of TB_TILE indices, occupied or
//                      not.  The tile's last counter word is its records' end
//                      after the placement and zero when no pair fell into it,
//                      so one scalar load tells an empty tile: it stores zeros
//                      (ACC: returns) and touches neither LDS nor a record.
//                      An occupied tile finds its first record in the scan's
//                      ascending tile list -- each wave probes 64 entries at
//                      once, two rounds for 4,096 listed tiles -- merges as
//                      tb_tile does (per rank an LDS atomicMax election on
//                      position + 1, then the winners add into the LDS sum in
//                      rank order), stores, and zeroes its counters.
//   tbb_dense          the same over a group's virtual tile space: a tile's
//                      tensor among <= 16 tile0 entries (scalar loads), its
//                      pointer, type, mode and n from the table.
//
// Stores.  The output needs only its element's alignment, so a lane does not
// store the 16 elements [16 tid, 16 tid + 16) but those shifted down by the
// tile's phase ph (elements of the tile's first address past a 16-byte
// boundary): [16 tid - ph, 16 tid - ph + 16) is four (fp32) or two (16-bit)
// aligned 16-byte words, read from the LDS sums and converted in registers.
// A word that is not wholly inside the tile (the first of lane 0, the ragged
// end of the last tile) goes element by element, as do the tile's last ph
// elements (lanes < ph, one each).  Every element of [0, n) is stored once and
// nothing else is.  ACC stores the union only: a read, an add and a store per
// marked element.
//
// No workgroup waits for another.  Every barrier is reached by the whole
// workgroup (the occupied test is uniform).  What is loaded from the scratch
// is clamped before it indexes anything; a disagreement sets FAIL_MERGE_SPARSE.
#include "merge_tile_dev.h"

namespace stg {

namespace {

typedef uint32_t u4v __attribute__((ext_vector_type(4)));

// Every element of the tile once: sum / world (ZERO: +0.0, no LDS read).
template <uint32_t DT, bool ZERO>
__device__ __forceinline__ void tile_store(const TileLds &L, const TileJob &k) {
    using E = elem_t<DT>;
    constexpr int32_t V = 16 / sizeof(E);  // elements of a 16-byte word
    E *p = static_cast<E *>(k.grad) + k.j0;
    const int32_t ph = (int32_t)((reinterpret_cast<uintptr_t>(p) / sizeof(E)) & (uintptr_t)(V - 1));
    const int32_t len = (int32_t)k.len, tid = (int32_t)threadIdx.x;
    const auto bits = [&](int32_t l) -> uint32_t { return ZERO ? 0u : to_bits<DT>(L.sum[l] / k.fworld); };
#pragma unroll
    for (int32_t q = 0; q < 16 / V; ++q) {
        const int32_t b = 16 * tid - ph + V * q;  // p + b: on a 16-byte boundary
        uint32_t x[V];
#pragma unroll
        for (int32_t u = 0; u < V; ++u) x[u] = b + u >= 0 && b + u < len ? bits(b + u) : 0u;
        if (b >= 0 && b + V <= len) {
            u4v w;
            if constexpr (V == 4) w = u4v{x[0], x[1], x[2], x[3]};
            else w = u4v{x[0] | x[1] << 16, x[2] | x[3] << 16, x[4] | x[5] << 16, x[6] | x[7] << 16};
            *reinterpret_cast<u4v *>(p + b) = w;
        } else {
#pragma unroll
            for (int32_t u = 0; u < V; ++u)
                if (b + u >= 0 && b + u < len) p[b + u] = (E)x[u];
        }
    }
    const int32_t l = (int32_t)TB_TILE - ph + tid;  // the shift left the tile's last ph elements over
    if (tid < ph && l < len) p[l] = (E)bits(l);
}

// grad += sum / world at the tile's union; nothing else is read or stored.
template <uint32_t DT>
__device__ __forceinline__ void tile_accumulate(const TileLds &L, const TileJob &k) {
    using E = elem_t<DT>;
    E *p = static_cast<E *>(k.grad) + k.j0;
    const uint32_t tid = threadIdx.x;
    const uint4 mv = reinterpret_cast<const uint4 *>(L.mark)[tid];
    const uint32_t words[4] = {mv.x, mv.y, mv.z, mv.w};
    if (!(mv.x | mv.y | mv.z | mv.w)) return;
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b) {
        const uint32_t l = 16 * tid + b;
        if (((words[b >> 2] >> (8 * (b & 3))) & 0xffu) && l < k.len)
            p[l] = (E)to_bits<DT>(from_bits<DT>(p[l]) + L.sum[l] / k.fworld);
    }
}

template <uint32_t DT, bool ACC>
__device__ __forceinline__ void tile_emit(const TileLds &L, const TileJob &k, bool occupied) {
    if (!occupied) {
        if (!ACC) tile_store<DT, true>(L, k);
        return;
    }
    if (ACC) tile_accumulate<DT>(L, k);
    else tile_store<DT, false>(L, k);
    for (uint32_t r = threadIdx.x; r < k.world; r += STG_WG) k.cw[r] = 0;  // the counters, zero for the next call
}

template <uint32_t DT, bool ACC>
__global__ void __launch_bounds__(STG_WG) tb_dense(GradArgs a) {
    __shared__ __attribute__((aligned(16))) TileLds L;
    const uint32_t tile = blockIdx.x;
    const uint64_t j0 = (uint64_t)tile << TB_TILE_SHIFT;
    if (j0 >= a.n) return;
    const TileJob k{a.sc, a.sc.cnt ? a.sc.cnt + (size_t)tile * a.world : nullptr, tile, a.world, a.cap, a.lcap,
                    a.fworld, a.grad, j0, (uint32_t)min((uint64_t)TB_TILE, a.n - j0)};
    tile_emit<DT, ACC>(L, k, tile_merge(L, k));
}

__global__ void __launch_bounds__(STG_WG) tbb_dense(GradBatchArgs a) {
    __shared__ __attribute__((aligned(16))) TileLds L;
    const uint32_t tile = blockIdx.x;
    // the tile's tensor: uniform, so the table is read with scalar loads
    uint32_t qt = 0;
    while (qt + 1 < a.nt && qt + 1 < MERGE_BATCH && tile >= a.t[qt + 1].blk0) ++qt;
    const GradBatchTensor &d = a.t[qt];
    const uint64_t j0 = (uint64_t)(tile - d.blk0) << TB_TILE_SHIFT;
    if (tile < d.blk0 || j0 >= d.n) return;
    const TileJob k{a.sc, a.sc.cnt + (size_t)tile * a.world, tile, a.world, a.cap, a.lcap,
                    a.fworld, d.grad, j0, (uint32_t)min((uint64_t)TB_TILE, d.n - j0)};
    const bool occ = tile_merge(L, k);
    switch (2 * d.dtype + (d.accumulate ? 1u : 0u)) {  // uniform
    case 2 * GRAD_F32: tile_emit<GRAD_F32, false>(L, k, occ); break;
    case 2 * GRAD_F32 + 1: tile_emit<GRAD_F32, true>(L, k, occ); break;
    case 2 * GRAD_BF16: tile_emit<GRAD_BF16, false>(L, k, occ); break;
    case 2 * GRAD_BF16 + 1: tile_emit<GRAD_BF16, true>(L, k, occ); break;
    case 2 * GRAD_F16: tile_emit<GRAD_F16, false>(L, k, occ); break;
    case 2 * GRAD_F16 + 1: tile_emit<GRAD_F16, true>(L, k, occ); break;
    default: break;  // (the entry refuses other types)
    }
}

template <uint32_t DT>
void launch_dense(const GradArgs &a, bool acc, hipStream_t s) {
    if (acc) tb_dense<DT, true><<<a.ntiles, STG_WG, 0, s>>>(a);
    else tb_dense<DT, false><<<a.ntiles, STG_WG, 0, s>>>(a);
}

}  // namespace

hipError_t launch_grad_dense(const GradArgs &a, int dtype, bool accumulate, hipStream_t s) {
    if (!a.ntiles || !a.world) return hipErrorInvalidValue;
    if (dtype == (int)GRAD_F32) launch_dense<GRAD_F32>(a, accumulate, s);
    else if (dtype == (int)GRAD_BF16) launch_dense<GRAD_BF16>(a, accumulate, s);
    else if (dtype == (int)GRAD_F16) launch_dense<GRAD_F16>(a, accumulate, s);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_grad_dense_batch(const GradBatchArgs &a, hipStream_t s) {
    if (!a.nt || !a.ntiles || !a.world || !a.sc.cnt) return hipErrorInvalidValue;
    tbb_dense<<<a.ntiles, STG_WG, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace stg
