// merge_tile_dev.h -- one tile of a tile-bucketed MERGE decompress merged in a
// workgroup's LDS, and the typed-output casts: shared by the dense gradient
// (merge_grad.hip) and the fused dense AdamW step (merge_adamw.hip) -- one
// text, so their merged sums agree bitwise.  gfx950 only.
#pragma once

#include <type_traits>

#include "merge_grad.h"
#include "wire_dev.h"
#include "merge_dev.h"

namespace stg {

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

}  // namespace stg
