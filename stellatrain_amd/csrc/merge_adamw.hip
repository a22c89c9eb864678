// merge_adamw.hip -- the dense Adam / AdamW step of torch.optim fed straight
// from `world` rank streams: every element's moments decay and every parameter
// moves, whether or not an index arrived for it, and the dense averaged
// gradient never exists in memory (gfx950).
//
// The pairs are bucketed by merge_sparse.hip's three launches (the batched ones
// for a group), as merge_grad.hip's are.  One launch then merges and steps:
//
//   tb_adamw<PT, MASTER>  one workgroup per tile of TB_TILE indices, occupied
//                         or not.  An occupied tile runs tile_merge (the text
//                         merge_grad.hip runs, merge_tile_dev.h) and steps with
//                         g = sum / world, +0.0 where no rank wrote: the mark
//                         array is not read.  It zeroes its counters for the
//                         next call.  An empty tile, told by the one scalar load
//                         of its last counter word, touches neither LDS nor a
//                         record and steps with g = +0.0f through the same
//                         function, so an unmarked element of an occupied tile
//                         and an element of an empty one get identical bits.
//   tbb_adamw             the same over a group's virtual tile space; the
//                         tensor's type and master come from the table and are
//                         uniform.
//
// Data movement.  The step is a pure stream over m, v and the fp32 parameter or
// master (and the 16-bit parameter), so it is laid out for coalescing: lane tid
// takes the 16-byte words q * 256 + tid, q = 0..3, of the tile shifted down by
// the fp32 arrays' common phase ph (elements of the tile's first address past a
// 16-byte boundary; the entry refuses arrays that are not congruent mod 16).
// A wave instruction then covers 1 KiB of whole contiguous lines per array.
// The tile's sums are read from LDS as the aligned float4 of the same word (and
// the one before it where ph != 0, picked apart by the uniform ph).  Per word a
// lane loads three 16-byte words, steps four elements in registers and stores
// three; the loop over q is not unrolled, so one word's loads are live at a
// time.  A word that is not wholly inside the tile (the first, the ragged end
// of the last tile) goes element by element, as do the tile's last ph elements
// (lanes < ph, one each).  Every element of [0, n) of each array is loaded once
// and stored once, and nothing outside is touched.  A 16-bit parameter needs
// only its element's alignment: a word's four elements move in the widest
// naturally aligned accesses their address allows (8; 4 + 4; 2 + 4 + 2 bytes),
// uniform over the tile.
//
// No workgroup waits for another.  Every barrier is reached by the whole
// workgroup (the occupied test is uniform).
#include "merge_adamw.h"
#include "merge_tile_dev.h"

namespace stg {

namespace {

// One element of torch.optim.Adam (decoupled: AdamW), no amsgrad, no maximize:
// every operation a separate fp32 rounding, in this order (-ffp-contract=off).
__device__ __forceinline__ void adamw_elem(const AdamwHyper &h, float g, float &x, float &m, float &v) {
    if (h.decoupled) x = x * h.decay;
    else g = g + h.wd * x;
    m = h.beta1 * m + h.omb1 * g;
    v = h.beta2 * v + h.omb2 * (g * g);
    const float den = sqrtf(v) / h.bc2s + h.eps;
    x = x - h.ss * (m / den);
}

// Four 16-bit elements at p, whose address in elements is `mis` mod 4 (uniform
// over a tile): one 8-byte access, two of 4 bytes, or 2 + 4 + 2.
__device__ __forceinline__ void load4_h(const uint16_t *p, uint32_t mis, uint32_t (&x)[4]) {
    uint32_t lo, hi;
    if (mis == 0) {
        const uint2 w = *reinterpret_cast<const uint2 *>(p);
        lo = w.x;
        hi = w.y;
    } else if (mis == 2) {
        lo = *reinterpret_cast<const uint32_t *>(p);
        hi = *reinterpret_cast<const uint32_t *>(p + 2);
    } else {
        const uint32_t mid = *reinterpret_cast<const uint32_t *>(p + 1);
        lo = (uint32_t)p[0] | mid << 16;
        hi = mid >> 16 | (uint32_t)p[3] << 16;
    }
    x[0] = lo & 0xffffu;
    x[1] = lo >> 16;
    x[2] = hi & 0xffffu;
    x[3] = hi >> 16;
}
__device__ __forceinline__ void store4_h(uint16_t *p, uint32_t mis, const uint32_t (&x)[4]) {
    const uint32_t lo = x[0] | x[1] << 16, hi = x[2] | x[3] << 16;
    if (mis == 0) {
        *reinterpret_cast<uint2 *>(p) = make_uint2(lo, hi);
    } else if (mis == 2) {
        *reinterpret_cast<uint32_t *>(p) = lo;
        *reinterpret_cast<uint32_t *>(p + 2) = hi;
    } else {
        p[0] = (uint16_t)x[0];
        *reinterpret_cast<uint32_t *>(p + 1) = x[1] | x[2] << 16;
        p[3] = (uint16_t)x[3];
    }
}

// Every element of the tile once: the step with g = sum / world (ZERO: +0.0f,
// no LDS read).  PT: the parameter's type; MASTER: x is the fp32 master and the
// 16-bit parameter is only written.
template <uint32_t PT, bool MASTER, bool ZERO>
__device__ __forceinline__ void tile_step(const TileLds &L, const TileJob &k, const AdamwTensor &t,
                                          const AdamwHyper &h) {
    static_assert(!(MASTER && PT == GRAD_F32), "a master goes with a 16-bit parameter");
    constexpr bool XF = MASTER || PT == GRAD_F32;  // x lives in an fp32 array
    constexpr bool PH = PT != GRAD_F32;            // there is a 16-bit parameter
    float *const m = t.m + k.j0, *const v = t.v + k.j0;
    float *const xf = XF ? (MASTER ? t.master : static_cast<float *>(t.param)) + k.j0 : nullptr;
    uint16_t *const p16 = PH ? static_cast<uint16_t *>(t.param) + k.j0 : nullptr;
    const int32_t ph = (int32_t)((reinterpret_cast<uintptr_t>(m) / sizeof(float)) & 3u);
    // a word's 16-bit elements start at p16 + 4 w - ph: the same residue for every word of the tile
    const uint32_t mis = PH ? (uint32_t)((reinterpret_cast<uintptr_t>(p16) / sizeof(uint16_t) - (uintptr_t)ph) & 3u) : 0u;
    const int32_t len = (int32_t)k.len, tid = (int32_t)threadIdx.x;
    const auto one = [&](int32_t l) {
        float x = XF ? xf[l] : from_bits<PT>(p16[l]);
        float mm = m[l], vv = v[l];
        adamw_elem(h, ZERO ? 0.f : L.sum[l] / k.fworld, x, mm, vv);
        m[l] = mm;
        v[l] = vv;
        if (XF) xf[l] = x;
        if (PH) p16[l] = (uint16_t)to_bits<PT>(x);
    };
#pragma nounroll
    for (int32_t q = 0; q < 4; ++q) {
        const int32_t w = q * (int32_t)STG_WG + tid;
        const int32_t b = 4 * w - ph;  // m + b: on a 16-byte boundary
        if (b >= 0 && b + 4 <= len) {
            const float4 m4 = *reinterpret_cast<const float4 *>(m + b);
            const float4 v4 = *reinterpret_cast<const float4 *>(v + b);
            float x[4], mm[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
            if (XF) {
                const float4 x4 = *reinterpret_cast<const float4 *>(xf + b);
                x[0] = x4.x; x[1] = x4.y; x[2] = x4.z; x[3] = x4.w;
            } else {
                uint32_t xb[4];
                load4_h(p16 + b, mis, xb);
#pragma unroll
                for (int32_t u = 0; u < 4; ++u) x[u] = from_bits<PT>(xb[u]);
            }
            float g[4] = {0.f, 0.f, 0.f, 0.f};
            if (!ZERO) {
                const float4 hi = reinterpret_cast<const float4 *>(L.sum)[w];
                float s[4] = {hi.x, hi.y, hi.z, hi.w};
                if (ph) {  // uniform; b >= 0 makes w >= 1
                    const float4 lo = reinterpret_cast<const float4 *>(L.sum)[w - 1];
                    if (ph == 1) { s[3] = hi.z; s[2] = hi.y; s[1] = hi.x; s[0] = lo.w; }
                    else if (ph == 2) { s[3] = hi.y; s[2] = hi.x; s[1] = lo.w; s[0] = lo.z; }
                    else { s[3] = hi.x; s[2] = lo.w; s[1] = lo.z; s[0] = lo.y; }
                }
#pragma unroll
                for (int32_t u = 0; u < 4; ++u) g[u] = s[u] / k.fworld;
            }
#pragma unroll
            for (int32_t u = 0; u < 4; ++u) adamw_elem(h, g[u], x[u], mm[u], vv[u]);
            *reinterpret_cast<float4 *>(m + b) = make_float4(mm[0], mm[1], mm[2], mm[3]);
            *reinterpret_cast<float4 *>(v + b) = make_float4(vv[0], vv[1], vv[2], vv[3]);
            if (XF) *reinterpret_cast<float4 *>(xf + b) = make_float4(x[0], x[1], x[2], x[3]);
            if (PH) {
                uint32_t xb[4];
#pragma unroll
                for (int32_t u = 0; u < 4; ++u) xb[u] = to_bits<PT>(x[u]);
                store4_h(p16 + b, mis, xb);
            }
        } else {
            for (int32_t u = 0; u < 4; ++u)
                if (b + u >= 0 && b + u < len) one(b + u);
        }
    }
    const int32_t l = (int32_t)TB_TILE - ph + tid;  // the shift left the tile's last ph elements over
    if (tid < ph && l < len) one(l);
}

template <uint32_t PT, bool MASTER>
__device__ __forceinline__ void tile_adamw(const TileLds &L, const TileJob &k, const AdamwTensor &t,
                                           const AdamwHyper &h, bool occupied) {
    if (!occupied) {
        tile_step<PT, MASTER, true>(L, k, t, h);
        return;
    }
    tile_step<PT, MASTER, false>(L, k, t, h);
    for (uint32_t r = threadIdx.x; r < k.world; r += STG_WG) k.cw[r] = 0;  // the counters, zero for the next call
}

template <uint32_t PT, bool MASTER>
__global__ void __launch_bounds__(STG_WG) tb_adamw(AdamwArgs a) {
    __shared__ __attribute__((aligned(16))) TileLds L;
    const uint32_t tile = blockIdx.x;
    const uint64_t j0 = (uint64_t)tile << TB_TILE_SHIFT;
    if (j0 >= a.n) return;
    const TileJob k{a.sc, a.sc.cnt ? a.sc.cnt + (size_t)tile * a.world : nullptr, tile, a.world, a.cap, a.lcap,
                    a.fworld, nullptr, j0, (uint32_t)min((uint64_t)TB_TILE, a.n - j0)};
    tile_adamw<PT, MASTER>(L, k, a.t, a.h, tile_merge(L, k));
}

__global__ void __launch_bounds__(STG_WG) tbb_adamw(AdamwBatchArgs a) {
    __shared__ __attribute__((aligned(16))) TileLds L;
    const uint32_t tile = blockIdx.x;
    // the tile's tensor: uniform, so the table is read with scalar loads
    uint32_t qt = 0;
    while (qt + 1 < a.nt && qt + 1 < MERGE_BATCH && tile >= a.t[qt + 1].blk0) ++qt;
    const AdamwBatchTensor &d = a.t[qt];
    const uint64_t j0 = (uint64_t)(tile - d.blk0) << TB_TILE_SHIFT;
    if (tile < d.blk0 || j0 >= d.n) return;
    const TileJob k{a.sc, a.sc.cnt + (size_t)tile * a.world, tile, a.world, a.cap, a.lcap,
                    a.fworld, nullptr, j0, (uint32_t)min((uint64_t)TB_TILE, d.n - j0)};
    const bool occ = tile_merge(L, k);
    switch (2 * d.dtype + (d.t.master ? 1u : 0u)) {  // uniform
    case 2 * GRAD_F32: tile_adamw<GRAD_F32, false>(L, k, d.t, a.h, occ); break;
    case 2 * GRAD_BF16: tile_adamw<GRAD_BF16, false>(L, k, d.t, a.h, occ); break;
    case 2 * GRAD_BF16 + 1: tile_adamw<GRAD_BF16, true>(L, k, d.t, a.h, occ); break;
    case 2 * GRAD_F16: tile_adamw<GRAD_F16, false>(L, k, d.t, a.h, occ); break;
    case 2 * GRAD_F16 + 1: tile_adamw<GRAD_F16, true>(L, k, d.t, a.h, occ); break;
    default: break;  // (the entry refuses other types, and a master beside an fp32 parameter)
    }
}

}  // namespace

hipError_t launch_adamw_dense(const AdamwArgs &a, int dtype, hipStream_t s) {
    if (!a.ntiles || !a.world || !a.t.param || !a.t.m || !a.t.v) return hipErrorInvalidValue;
    const bool master = a.t.master != nullptr;
    if (dtype == (int)GRAD_F32 && !master) tb_adamw<GRAD_F32, false><<<a.ntiles, STG_WG, 0, s>>>(a);
    else if (dtype == (int)GRAD_BF16 && !master) tb_adamw<GRAD_BF16, false><<<a.ntiles, STG_WG, 0, s>>>(a);
    else if (dtype == (int)GRAD_BF16) tb_adamw<GRAD_BF16, true><<<a.ntiles, STG_WG, 0, s>>>(a);
    else if (dtype == (int)GRAD_F16 && !master) tb_adamw<GRAD_F16, false><<<a.ntiles, STG_WG, 0, s>>>(a);
    else if (dtype == (int)GRAD_F16) tb_adamw<GRAD_F16, true><<<a.ntiles, STG_WG, 0, s>>>(a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_adamw_dense_batch(const AdamwBatchArgs &a, hipStream_t s) {
    if (!a.nt || !a.ntiles || !a.world || !a.sc.cnt) return hipErrorInvalidValue;
    tbb_adamw<<<a.ntiles, STG_WG, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace stg
