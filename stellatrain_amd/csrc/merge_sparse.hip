// merge_sparse.hip -- MERGE decompress of `world` rank streams without any
// array as long as the parameter: the pairs are bucketed by index tile and
// each occupied tile is merged in LDS (gfx950).
//
// The results are those of apply.hip's world > 1 path bit for bit -- per rank
// the last position of an index wins, the winners are summed in rank order
// from +0.0f, divided by (float)world and emitted in ascending index order --
// but the work and the scratch follow the world * per_rank pairs and the
// ceil(n / TB_TILE) tiles, not n:
//
//   tb_bucket<false>  every pair once: pairs per (tile, rank), integer atomics
//                     on cnt[tile * world + rank].  A lane reads four
//                     consecutive pairs of one rank and adds a run of them that
//                     share a tile in one atomic (codec streams ascend, so runs
//                     are the rule; the (0, 0.0) filler slots all hit tile 0).
//   tb_scan           one workgroup: the counters of every non-empty tile
//                     become the first record slot of each (tile, rank)
//                     segment -- a tile's segments back to back in rank order
//                     -- and the tile joins the list with its first slot.
//   tb_bucket<true>   every pair again: a slot from the segment's word (which
//                     so ends at the segment's end), the record {position,
//                     index within the tile} and the value.  Order inside a
//                     segment is whatever the atomics give; nothing reads it.
//   tb_tile<0>        per listed tile (grid-stride over the device's list
//                     count): for rank 0 .. world - 1 in turn the rank's
//                     segment elects with an LDS atomicMax on position + 1, and
//                     after a barrier the records that hold the elected
//                     position add their value to the LDS sum, set the mark and
//                     clear the election word: one winner per index and rank,
//                     so no two lanes touch a word.  Then the tile's marks are
//                     counted.
//   tb_tscan          one workgroup: the union counts' exclusive prefixes and
//                     *out_count.
//   tb_tile<1>        the merge of the tile again (cheaper than staging 36 KiB
//                     per tile), then its marked indices in order at the tile's
//                     prefix with sum / world, the optimizer step on each where
//                     fused, and the tile's counters back to zero.
//
// A tile's records are one contiguous range, so a lane loads up to TB_CACHE
// of them (1,024 per workgroup: every tile of a codec's stream at its usual
// density) with their ranks in one round trip before the rank loop; what lies
// past the cached range is streamed from memory inside each rank's two phases.
// A tile may hold every pair of the call.
//
// No workgroup waits for another: launch boundaries are the only ordering.
// Every barrier is reached by the whole workgroup: the rank loop runs `world`
// (a kernel argument) times with two barriers each, and loaded values only
// bound loops that hold no barrier.  What is loaded from the scratch is clamped
// before it indexes anything, and a disagreement sets FAIL_MERGE_SPARSE in the
// scratch's fail word.
#include "merge_sparse.h"
#include "wire_dev.h"
#include "merge_dev.h"

namespace stg {

namespace {

struct BucketArgs {
    SparseScratch sc;
    uint64_t n;
    uint32_t world, per_rank;
    uint32_t bpr;      // workgroups per rank
    uint32_t cap;
};

template <bool PLACE>
__global__ void __launch_bounds__(STG_WG) tb_bucket(SparseRanks rk, BucketArgs a) {
    const uint32_t lr = blockIdx.x / a.bpr;
    const RankStream &k = rk.r[lr];
    const size_t m = a.per_rank;
    const size_t wend = 8 * ((m - 1) / 8);  // m >= 1
    const size_t e = (size_t)(blockIdx.x - lr * a.bpr) * TB_PAIRS + 4 * threadIdx.x;
    if (e >= m) return;
    uint32_t j[4];
    float v[4];
    wire_get_idx4(k.idx, k.flag, wend, m, e, j);
    if (PLACE) wire_get_val4(k.val, k.flag, wend, m, e, v);
    // a run: consecutive kept pairs of the lane in one tile; len at its head
    bool ok[4];
    uint32_t len[4];
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) ok[b] = e + b < m && j[b] < a.n;
#pragma unroll
    for (int b = 3; b >= 0; --b) {
        const bool joins = b < 3 && ok[b + 1] && (j[b + 1] >> TB_TILE_SHIFT) == (j[b] >> TB_TILE_SHIFT);
        len[b] = ok[b] ? 1u + (joins ? len[b + 1] : 0u) : 0u;
    }
    uint32_t slot = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) {
        if (!ok[b]) continue;
        const bool head = b == 0 || !ok[b - 1] || (j[b - 1] >> TB_TILE_SHIFT) != (j[b] >> TB_TILE_SHIFT);
        if (head) {
            uint32_t *w = a.sc.cnt + (size_t)(j[b] >> TB_TILE_SHIFT) * a.world + (rk.r0 + lr);
            if (PLACE) slot = g_add(w, len[b]);
            else (void)g_add(w, len[b]);
        }
        if (PLACE) {
            if (slot < a.cap) {
                a.sc.rec[slot] = make_uint2((uint32_t)(e + b), j[b] & (TB_TILE - 1));
                a.sc.rval[slot] = v[b];
            } else {
                g_or(a.sc.fail, FAIL_MERGE_SPARSE);  // an offset past the record buffer
            }
            ++slot;
        }
    }
}

// One workgroup of 1,024 threads, four tiles per thread per round: a non-empty
// tile's counters become its segments' first slots; the list of those tiles.
__global__ void __launch_bounds__(1024) tb_scan(SparseArgs a) {
    __shared__ uint32_t sh[16 + 1];
    const uint32_t world = a.world;
    uint32_t run = 0, nl = 0;
    for (uint32_t t0 = 0; t0 < a.ntiles; t0 += 4 * 1024) {  // uniform trip count
        const uint32_t tb = t0 + 4 * threadIdx.x;
        uint32_t c[4], sum = 0, ne = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            c[q] = 0;
            if (tb + q < a.ntiles) {
                const uint32_t *w = a.sc.cnt + (size_t)(tb + q) * world;
                for (uint32_t r = 0; r < world; ++r) c[q] += w[r];
            }
            sum += c[q];
            ne += c[q] != 0;
        }
        uint32_t tot, ltot;
        uint32_t p = run + blk_excl_scan<16>(sum, sh, &tot);
        uint32_t lp = nl + blk_excl_scan<16>(ne, sh, &ltot);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            if (tb + q < a.ntiles && c[q]) {
                if (lp < a.lcap) a.sc.list[lp] = make_uint2(tb + q, p);
                ++lp;
                uint32_t *w = a.sc.cnt + (size_t)(tb + q) * world;
                uint32_t o = p;
                for (uint32_t r = 0; r < world; ++r) { const uint32_t x = w[r]; w[r] = o; o += x; }
                p += c[q];
            }
        }
        run += tot;
        nl += ltot;
    }
    if (threadIdx.x == 0) {
        const bool bad = nl > a.lcap || run > a.cap;  // more tiles or pairs than the call can hold
        if (bad) g_or(a.sc.fail, FAIL_MERGE_SPARSE);
        a.sc.ctl->ntl = bad ? 0u : nl;
        a.sc.ctl->kept = run;
    }
}

// One workgroup, as tb_scan: the listed tiles' union counts to exclusive
// prefixes, and the call's count.
__global__ void __launch_bounds__(1024) tb_tscan(SparseArgs a) {
    __shared__ uint32_t sh[16 + 1];
    const uint32_t ntl = min(a.sc.ctl->ntl, a.lcap);
    uint32_t run = 0;
    for (uint32_t t0 = 0; t0 < ntl; t0 += 4 * 1024) {  // uniform: every lane read the same count
        const uint32_t tb = t0 + 4 * threadIdx.x;
        uint32_t c[4], sum = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) { c[q] = tb + q < ntl ? a.sc.ucnt[tb + q] : 0u; sum += c[q]; }
        uint32_t tot;
        uint32_t p = run + blk_excl_scan<16>(sum, sh, &tot);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
            if (tb + q < ntl) { a.sc.ucnt[tb + q] = p; p += c[q]; }
        run += tot;
    }
    if (threadIdx.x == 0) {
        const bool bad = run > a.cap || run > a.sc.ctl->kept;  // a union larger than its pairs
        if (bad) g_or(a.sc.fail, FAIL_MERGE_SPARSE);
        *a.t.out_count = bad ? POISON_COUNT : run;
    }
}

// EMIT 0: the tile's union size into ucnt.  EMIT 1: the union in order at the
// tile's prefix, with the step (OPT -1: none; else Step<OPT>).
template <int EMIT, int OPT>
__global__ void __launch_bounds__(STG_WG) tb_tile(SparseArgs a) {
    __shared__ __attribute__((aligned(16))) float s_sum[TB_TILE];
    __shared__ __attribute__((aligned(16))) uint32_t s_win[TB_TILE];
    __shared__ __attribute__((aligned(16))) uint8_t s_mark[TB_TILE];
    __shared__ uint32_t s_end[TB_RANKS];
    __shared__ uint32_t sh[STG_WAVES + 1];
    const uint32_t tid = threadIdx.x, world = a.world;
    const uint32_t ntl = min(a.sc.ctl->ntl, a.lcap);
    const bool cached = world <= TB_RANKS;  // the segments' ends fit s_end: records can be held with their ranks
    for (uint32_t li = blockIdx.x; li < ntl; li += gridDim.x) {  // uniform: every lane read the same count
        // a lane zeroes the 16 indices it emits (nobody else reads them after the rank loop)
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            reinterpret_cast<uint4 *>(s_sum)[4 * tid + q] = make_uint4(0u, 0u, 0u, 0u);
            reinterpret_cast<uint4 *>(s_win)[4 * tid + q] = make_uint4(0u, 0u, 0u, 0u);
        }
        reinterpret_cast<uint4 *>(s_mark)[tid] = make_uint4(0u, 0u, 0u, 0u);
        const uint2 le = a.sc.list[li];
        const uint32_t tile = min(le.x, a.ntiles - 1);  // (ntl > 0 implies ntiles > 0)
        uint32_t *cw = a.sc.cnt + (size_t)tile * world;
        if (cached && tid < world) s_end[tid] = cw[tid];
        const uint32_t tend = min(cw[world - 1], a.cap);
        const uint32_t start = min(le.y, tend);
        if (tid == 0 && (le.x >= a.ntiles || cw[world - 1] > a.cap || le.y > tend)) g_or(a.sc.fail, FAIL_MERGE_SPARSE);
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
                rc[q] = a.sc.rec[g];
                if (EMIT) rv[q] = a.sc.rval[g];
                uint32_t r = 0;
                while (r + 1 < world && g >= s_end[r]) ++r;
                rr[q] = r;
            }
        }
        const uint32_t sfirst = start + ncache;  // streamed from here on
        uint32_t sb = start;
        for (uint32_t r = 0; r < world; ++r) {
            const uint32_t se0 = cached ? s_end[r] : cw[r];
            const uint32_t se = min(max(se0, sb), tend);  // ends ascend inside [start, tend]
            if (tid == 0 && se != se0) g_or(a.sc.fail, FAIL_MERGE_SPARSE);
#pragma unroll
            for (uint32_t q = 0; q < TB_CACHE; ++q)
                if (rr[q] == r) atomicMax(&s_win[rc[q].y & (TB_TILE - 1)], rc[q].x + 1u);
            for (uint32_t g = max(sb, sfirst) + tid; g < se; g += STG_WG) {
                const uint2 x = a.sc.rec[g];
                atomicMax(&s_win[x.y & (TB_TILE - 1)], x.x + 1u);
            }
            __syncthreads();
#pragma unroll
            for (uint32_t q = 0; q < TB_CACHE; ++q) {
                const uint32_t l = rc[q].y & (TB_TILE - 1);
                if (rr[q] == r && s_win[l] == rc[q].x + 1u) {
                    s_win[l] = 0;
                    s_mark[l] = 1;
                    if (EMIT) s_sum[l] += rv[q];
                }
            }
            for (uint32_t g = max(sb, sfirst) + tid; g < se; g += STG_WG) {
                const uint2 x = a.sc.rec[g];
                const uint32_t l = x.y & (TB_TILE - 1);
                if (s_win[l] == x.x + 1u) {
                    s_win[l] = 0;
                    s_mark[l] = 1;
                    if (EMIT) s_sum[l] += a.sc.rval[g];
                }
            }
            __syncthreads();
            sb = se;
        }
        const uint4 mv = reinterpret_cast<const uint4 *>(s_mark)[tid];
        const uint32_t words[4] = {mv.x, mv.y, mv.z, mv.w};
        const uint32_t c = nz_bytes(mv.x) + nz_bytes(mv.y) + nz_bytes(mv.z) + nz_bytes(mv.w);
        uint32_t tc;
        uint32_t o = wg_excl_scan(c, sh, &tc);  // (ends on a barrier: the next tile may zero)
        if (!EMIT) {
            if (tid == 0) a.sc.ucnt[li] = tc;
            continue;
        }
        o += a.sc.ucnt[li];
        if (tid == 0 && (o > a.cap || tc > a.cap - o)) g_or(a.sc.fail, FAIL_MERGE_SPARSE);
        if (c) {
#pragma unroll
            for (uint32_t b = 0; b < 16; ++b) {
                if ((words[b >> 2] >> (8 * (b & 3))) & 0xffu) {
                    const uint32_t l = 16 * tid + b;
                    const uint32_t j = (tile << TB_TILE_SHIFT) + l;
                    const float g = s_sum[l] / a.fworld;  // merged_grad[j] (cpu_optimize.cpp:49-55)
                    if (o < a.cap) {
                        a.t.out_idx[o] = j;
                        a.t.out_val[o] = g;
                        if constexpr (OPT >= 0) {
                            const Step<OPT> opt(a, a.t);
                            float x, m0, f;
                            uint32_t last;
                            opt.load(j, x, m0, f, last);
                            opt.factors(f, last);
                            opt.step(j, g, x, m0, f, last);  // the union holds j once: updates commute
                        }
                    }
                    ++o;
                }
            }
        }
        for (uint32_t r = tid; r < world; r += STG_WG) cw[r] = 0;  // the counters, zero for the next call
    }
}

hipError_t launch_emit(const SparseArgs &a, int opt, uint32_t grid, hipStream_t s) {
    if (opt < 0) tb_tile<1, -1><<<grid, STG_WG, 0, s>>>(a);
    else if (opt == 2) tb_tile<1, 2><<<grid, STG_WG, 0, s>>>(a);
    else if (opt == 1) tb_tile<1, 1><<<grid, STG_WG, 0, s>>>(a);
    else tb_tile<1, 0><<<grid, STG_WG, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sparse_bucketing(const RankStream *ranks, const SparseArgs &a, hipStream_t s) {
    BucketArgs b{a.sc, a.n, a.world, a.per_rank, (uint32_t)(((uint64_t)a.per_rank + TB_PAIRS - 1) / TB_PAIRS), a.cap};
    const auto bucket = [&](bool place) -> hipError_t {
        for (uint32_t r0 = 0; r0 < a.world; r0 += TB_RANKS) {
            SparseRanks rk{};
            rk.nr = std::min<uint32_t>(TB_RANKS, a.world - r0);
            rk.r0 = r0;
            for (uint32_t r = 0; r < rk.nr; ++r) rk.r[r] = ranks[r0 + r];
            if (place) tb_bucket<true><<<b.bpr * rk.nr, STG_WG, 0, s>>>(rk, b);
            else tb_bucket<false><<<b.bpr * rk.nr, STG_WG, 0, s>>>(rk, b);
        }
        return hipGetLastError();
    };
    hipError_t e;
    if ((e = bucket(false)) != hipSuccess) return e;
    tb_scan<<<1, 1024, 0, s>>>(a);
    return bucket(true);
}

hipError_t launch_merge_sparse(const RankStream *ranks, const SparseArgs &a, int opt, int num_cu, hipStream_t s) {
    if (const hipError_t e = launch_sparse_bucketing(ranks, a, s); e != hipSuccess) return e;
    // four workgroups of 36 KiB per CU; never more than the list can hold
    const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>(a.lcap, (uint32_t)std::max(num_cu, 1) * 4));
    tb_tile<0, -1><<<grid, STG_WG, 0, s>>>(a);
    tb_tscan<<<1, 1024, 0, s>>>(a);
    return launch_emit(a, opt, grid, s);
}

}  // namespace stg
