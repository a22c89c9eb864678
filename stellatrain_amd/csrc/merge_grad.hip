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
#include "merge_grad.h"
#include "wire_dev.h"
#include "merge_dev.h"

#include <type_traits>

namespace stg {

namespace {

typedef uint32_t u4v __attribute__((ext_vector_type(4)));

struct TileLds {
    float sum[TB_TILE];
    uint32_t win[TB_TILE];
    uint8_t mark[TB_TILE];
    uint32_t end[TB_RANKS];
};

template <uint32_t DT>
using elem_t = typename std::conditional<DT == GRAD_F32, uint32_t, uint16_t>::type;

// float -> the output's bits: bf16 and fp16 round to nearest even, a NaN stays a NaN
template <uint32_t DT>
__device__ __forceinline__ uint32_t to_bits(float f) {
    const uint32_t u = f2u(f);
    if (DT == GRAD_F32) return u;
    if (DT == GRAD_F16) return f32_to_f16_rne(u);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
template <uint32_t DT>
__device__ __forceinline__ float from_bits(uint32_t x) {
    if (DT == GRAD_F32) return u2f(x);
    if (DT == GRAD_F16) return u2f(f16_to_f32(x));
    return u2f(x << 16);
}

// The first record slot of `tile` from the scan's list (ascending by tile, ntl
// entries): a 64-way search per wave, every lane of the wave active.  All
// waves read the same words and agree.
__device__ __forceinline__ bool list_find(const uint2 *list, uint32_t ntl, uint32_t tile, uint32_t *start) {
    const uint32_t lane = lane_id();
    uint32_t lo = 0, hi = ntl;
    while (hi - lo > 64) {  // uniform
        const uint32_t step = (hi - lo + 63) / 64;
        const uint32_t i = lo + lane * step;
        const uint32_t c = (uint32_t)__popcll(__ballot(i < hi && list[i].x <= tile));
        if (!c) return false;
        lo += (c - 1) * step;  // (c counts probes below hi: lo stays one of them)
        hi = min(hi, lo + step);
    }
    const uint32_t i = lo + lane;
    const uint2 e = i < hi ? list[i] : make_uint2(~0u, 0u);
    const uint64_t hit = __ballot(i < hi && e.x == tile);
    if (!hit) return false;
    *start = (uint32_t)__shfl((int)e.y, __ffsll((long long)hit) - 1, 64);
    return true;
}

// One tile's work: its counters, where its elements go, the call's bounds.
struct TileJob {
    SparseScratch sc;
    uint32_t *cw;      // the tile's `world` counter words (null: nothing bucketed, the tile is empty)
    uint32_t tile;     // its number in the list
    uint32_t world, cap, lcap;
    float fworld;
    void *grad;        // the tensor's first element
    uint64_t j0;       // the tile's first index in it
    uint32_t len;      // its elements: min(TB_TILE, n - j0) >= 1
};

// False for an empty tile.  Else the tile merged into L by tb_tile's rules:
// L.sum the winners' sum in rank order from +0.0f, L.mark the union; ends on a
// barrier.
__device__ __forceinline__ bool tile_merge(TileLds &L, const TileJob &k) {
    const uint32_t tid = threadIdx.x, world = k.world;
    const uint32_t tend0 = k.cw ? k.cw[world - 1] : 0u;
    if (!tend0) return false;  // uniform: one word, the same for every lane
    const uint32_t tend = min(tend0, k.cap);
    uint32_t start0 = tend;
    const bool found = list_find(k.sc.list, min(k.sc.ctl->ntl, k.lcap), k.tile, &start0);
    const uint32_t start = min(start0, tend);
    if (tid == 0 && (!found || tend0 > k.cap || start0 > tend)) g_or(k.sc.fail, FAIL_MERGE_SPARSE);
    const bool cached = world <= TB_RANKS;  // the segments' ends fit L.end: records can be held with their ranks
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        reinterpret_cast<uint4 *>(L.sum)[4 * tid + q] = make_uint4(0u, 0u, 0u, 0u);
        reinterpret_cast<uint4 *>(L.win)[4 * tid + q] = make_uint4(0u, 0u, 0u, 0u);
    }
    reinterpret_cast<uint4 *>(L.mark)[tid] = make_uint4(0u, 0u, 0u, 0u);
    if (cached && tid < world) L.end[tid] = k.cw[tid];
    __syncthreads();
    // the first records of the tile, whatever their rank, in one round trip
    uint2 rc[TB_CACHE];
    float rv[TB_CACHE];
    uint32_t rr[TB_CACHE];
    const uint32_t ncache = cached ? min(tend - start, TB_CACHE * STG_WG) : 0u;
#pragma unroll
    for (uint32_t q = 0; q < TB_CACHE; ++q) {
        const uint32_t g = start + q * STG_WG + tid;
        rr[q] = ~0u;
        rc[q] = make_uint2(0u, 0u);
        rv[q] = 0.f;
        if (q * STG_WG + tid < ncache) {
            rc[q] = k.sc.rec[g];
            rv[q] = k.sc.rval[g];
            uint32_t r = 0;
            while (r + 1 < world && g >= L.end[r]) ++r;
            rr[q] = r;
        }
    }
    const uint32_t sfirst = start + ncache;  // streamed from here on
    uint32_t sb = start;
    for (uint32_t r = 0; r < world; ++r) {
        const uint32_t se0 = cached ? L.end[r] : k.cw[r];
        const uint32_t se = min(max(se0, sb), tend);  // ends ascend inside [start, tend]
        if (tid == 0 && se != se0) g_or(k.sc.fail, FAIL_MERGE_SPARSE);
#pragma unroll
        for (uint32_t q = 0; q < TB_CACHE; ++q)
            if (rr[q] == r) atomicMax(&L.win[rc[q].y & (TB_TILE - 1)], rc[q].x + 1u);
        for (uint32_t g = max(sb, sfirst) + tid; g < se; g += STG_WG) {
            const uint2 x = k.sc.rec[g];
            atomicMax(&L.win[x.y & (TB_TILE - 1)], x.x + 1u);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t q = 0; q < TB_CACHE; ++q) {
            const uint32_t l = rc[q].y & (TB_TILE - 1);
            if (rr[q] == r && L.win[l] == rc[q].x + 1u) {
                L.win[l] = 0;
                L.mark[l] = 1;
                L.sum[l] += rv[q];
            }
        }
        for (uint32_t g = max(sb, sfirst) + tid; g < se; g += STG_WG) {
            const uint2 x = k.sc.rec[g];
            const uint32_t l = x.y & (TB_TILE - 1);
            if (L.win[l] == x.x + 1u) {
                L.win[l] = 0;
                L.mark[l] = 1;
                L.sum[l] += k.sc.rval[g];
            }
        }
        __syncthreads();
        sb = se;
    }
    return true;
}

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
