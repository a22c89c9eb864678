// merge_sparse_batch.hip -- the sparse MERGE decompress (merge_sparse.hip) with
// the optimizer step in its emission, for up to MERGE_BATCH parameter tensors
// of one world in shared launches (gfx950).
//
// The group is one virtual tile space: tensor q owns the tiles [tile0_q,
// tile0_q + ceil(n_q / TB_TILE)).  The counter array, the tile list, the
// records and the union counts are those of one large sparse call over that
// space, and the kernels are merge_sparse.hip's with three things per tensor:
// where a pair's tile lands, where a tile's output goes, and where the output
// prefix restarts.
//
//   sb_bucket<false>  every pair of every tensor once, SB_RANKS ranks per
//                     launch (the streams travel by value): a workgroup finds
//                     (tensor, rank, block) through blk0; a pair j < n_q counts
//                     in virtual tile tile0_q + (j >> 12), a run per atomic.
//                     The atomics only count, so the launches' order is free.
//   sb_scan           one workgroup over the group's tiles: segments' first
//                     record slots (global to the group) and the list of
//                     non-empty virtual tiles, ascending.
//   sb_bucket<true>   every pair again: its record and value at its slot.
//   sb_tile<0>        grid-stride over the listed tiles: the merge of a tile
//                     in LDS (the rank loop of tb_tile, two whole-workgroup
//                     barriers per rank), its union count.
//   sb_tscan          one workgroup: the union counts' exclusive prefixes over
//                     the group, then per tensor the prefix at its first
//                     listed tile (a tensor with none: count 0); a tile's
//                     offset becomes its prefix minus its tensor's base, and
//                     every tensor's count is written.
//   sb_tile<1>        the merge again, the tile's marked indices in order at
//                     its offset in its tensor's output -- j = (local tile <<
//                     12) + l, sum / world -- Step<OPT> of that tensor on each,
//                     and the tile's counters back to zero.
//
// The bucketing lane, the scan and the tile merge restate merge_sparse.hip's
// text line for line.  They are not one shared header: with the bodies moved
// into templated device functions the per-tensor kernels compile to the same
// instructions on other register numbers, and that file's assembly is kept as
// it is.
//
// No workgroup waits for another: launch boundaries are the only ordering.
// Every barrier is reached by the whole workgroup; loaded values only bound
// loops that hold no barrier.  What is loaded from the scratch is clamped
// before it indexes anything; a disagreement sets FAIL_MERGE_SPARSE and
// poisons the counts of the group's tensors.  A tile's tensor is searched
// among the <= 16 tile0 entries on a value made uniform (readfirstlane), so
// the table is read with scalar loads and never copied to scratch memory.
#include "merge_sparse_batch.h"
#include "wire_dev.h"
#include "merge_dev.h"

namespace stg {

namespace {

template <bool PLACE>
__global__ void __launch_bounds__(STG_WG) sb_bucket(SparseBucketArgs w) {
    const uint32_t t = batch_item(w.t, w.nt);
    const SparseBucketTensor &d = w.t[t];
    const uint32_t blk = blockIdx.x - d.blk0;
    const uint32_t lr = min(blk / d.bpr, SB_RANKS - 1);
    const RankStream &k = d.r[lr];
    const size_t m = d.per_rank;
    const size_t wend = 8 * ((m - 1) / 8);  // m >= 1
    const size_t e = (size_t)(blk - lr * d.bpr) * TB_PAIRS + 4 * threadIdx.x;
    if (e >= m) return;
    uint32_t j[4];
    float v[4];
    wire_get_idx4(k.idx, k.flag, wend, m, e, j);
    if (PLACE) wire_get_val4(k.val, k.flag, wend, m, e, v);
    // a run: consecutive kept pairs of the lane in one tile; len at its head
    bool ok[4];
    uint32_t len[4];
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) ok[b] = e + b < m && j[b] < d.n;
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
            // (j < n_q: the tile is one of the tensor's own)
            uint32_t *c = w.sc.cnt + (size_t)(d.tile0 + (j[b] >> TB_TILE_SHIFT)) * w.world + (w.r0 + lr);
            if (PLACE) slot = g_add(c, len[b]);
            else (void)g_add(c, len[b]);
        }
        if (PLACE) {
            if (slot < w.cap) {
                w.sc.rec[slot] = make_uint2((uint32_t)(e + b), j[b] & (TB_TILE - 1));
                w.sc.rval[slot] = v[b];
            } else {
                g_or(w.sc.fail, FAIL_MERGE_SPARSE);  // an offset past the record buffer
            }
            ++slot;
        }
    }
}

// tb_scan over the group's tile space: one workgroup of 1,024 threads, four
// tiles per thread per round (at most 16 rounds: SB_TILE_CAP).
__global__ void __launch_bounds__(1024) sb_scan(SparseBatchArgs a) {
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
        const bool bad = nl > a.lcap || run > a.cap;  // more tiles or pairs than the group can hold
        if (bad) g_or(a.sc.fail, FAIL_MERGE_SPARSE);
        a.sc.ctl->ntl = bad ? 0u : nl;
        a.sc.ctl->kept = run;
    }
}

// The tensor that owns virtual tile `tile`, among nt <= MERGE_BATCH ascending tile0 entries.
__device__ __forceinline__ uint32_t tile_owner(const uint32_t *tile0, uint32_t nt, uint32_t tile) {
    uint32_t q = 0;
    while (q + 1 < nt && tile >= tile0[q + 1]) ++q;
    return q;
}

// One workgroup, as sb_scan.  Round one: the listed tiles' union counts to
// exclusive prefixes over the group; a tensor's listed tiles are consecutive
// in the list (it ascends), so the entry whose predecessor has another owner
// holds the tensor's base and the one whose successor has another owner its
// end.  Round two (each thread on the entries it wrote): prefix minus base.
__global__ void __launch_bounds__(1024) sb_tscan(SparseBatchArgs a) {
    __shared__ uint32_t sh[16 + 1];
    __shared__ uint32_t s_t0[MERGE_BATCH], s_base[MERGE_BATCH], s_end[MERGE_BATCH];
    const uint32_t tid = threadIdx.x, nt = min(a.nt, MERGE_BATCH);
    const uint32_t ntl = min(a.sc.ctl->ntl, a.lcap);
    if (tid == 0) {
#pragma unroll
        for (uint32_t q = 0; q < MERGE_BATCH; ++q) {  // (constant subscripts: scalar loads of the table)
            s_t0[q] = a.t[q].blk0;
            s_base[q] = 0;
            s_end[q] = 0;
        }
    }
    __syncthreads();
    const uint32_t tmax = a.ntiles - 1;  // (ntl > 0 implies ntiles > 0)
    uint32_t run = 0;
    for (uint32_t t0 = 0; t0 < ntl; t0 += 4 * 1024) {  // uniform: every lane read the same count
        const uint32_t tb = t0 + 4 * tid;
        uint32_t c[4], sum = 0;
        uint32_t ow[6];  // the owners of entries tb - 1 .. tb + 4; none: ~0
#pragma unroll
        for (uint32_t q = 0; q < 6; ++q) {
            const uint32_t i = tb + q - 1u;  // (tb == 0, q == 0: wraps past ntl)
            ow[q] = i < ntl ? tile_owner(s_t0, nt, min(a.sc.list[i].x, tmax)) : ~0u;
        }
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) { c[q] = tb + q < ntl ? a.sc.ucnt[tb + q] : 0u; sum += c[q]; }
        uint32_t tot;
        uint32_t p = run + blk_excl_scan<16>(sum, sh, &tot);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            if (tb + q < ntl) {
                if (ow[q] != ow[q + 1]) s_base[ow[q + 1]] = p;
                a.sc.ucnt[tb + q] = p;
                p += c[q];
                if (ow[q + 2] != ow[q + 1]) s_end[ow[q + 1]] = p;
            }
        }
        run += tot;
    }
    __syncthreads();
    for (uint32_t t0 = 0; t0 < ntl; t0 += 4 * 1024) {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t i = t0 + 4 * tid + q;
            if (i < ntl) a.sc.ucnt[i] -= s_base[tile_owner(s_t0, nt, min(a.sc.list[i].x, tmax))];
        }
    }
    if (tid == 0) {
        bool bad = run > a.cap || run > a.sc.ctl->kept;  // a union larger than its pairs
#pragma unroll
        for (uint32_t q = 0; q < MERGE_BATCH; ++q)
            if (q < nt) bad = bad || s_end[q] < s_base[q] || s_end[q] - s_base[q] > a.t[q].ocap;
        if (bad) g_or(a.sc.fail, FAIL_MERGE_SPARSE);
#pragma unroll
        for (uint32_t q = 0; q < MERGE_BATCH; ++q)
            if (q < nt) *a.t[q].out_count = bad ? POISON_COUNT : s_end[q] - s_base[q];
    }
}

// EMIT 0: the tile's union size into ucnt.  EMIT 1: the union in order at the
// tile's offset in its tensor's output, with Step<OPT> of that tensor.
template <int EMIT, int OPT>
__global__ void __launch_bounds__(STG_WG) sb_tile(SparseBatchArgs a) {
    __shared__ __attribute__((aligned(16))) float s_sum[TB_TILE];
    __shared__ __attribute__((aligned(16))) uint32_t s_win[TB_TILE];
    __shared__ __attribute__((aligned(16))) uint8_t s_mark[TB_TILE];
    __shared__ uint32_t s_end[TB_RANKS];
    __shared__ uint32_t sh[STG_WAVES + 1];
    const uint32_t tid = threadIdx.x, world = a.world;  // world <= TB_RANKS: the segments' ends fit s_end
    const uint32_t ntl = min(a.sc.ctl->ntl, a.lcap);
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
        if (tid < world) s_end[tid] = cw[tid];
        const uint32_t tend = min(cw[world - 1], a.cap);
        const uint32_t start = min(le.y, tend);
        if (tid == 0 && (le.x >= a.ntiles || cw[world - 1] > a.cap || le.y > tend)) g_or(a.sc.fail, FAIL_MERGE_SPARSE);
        __syncthreads();
        // the first records of the tile, whatever their rank, in one round trip
        uint2 rc[TB_CACHE];
        float rv[TB_CACHE];
        uint32_t rr[TB_CACHE];
        const uint32_t ncache = min(tend - start, TB_CACHE * STG_WG);
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
            const uint32_t se0 = s_end[r];
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
        // the tile's tensor: uniform, so the table is read with scalar loads
        const uint32_t ut = __builtin_amdgcn_readfirstlane(tile);
        uint32_t qt = 0;
        while (qt + 1 < a.nt && qt + 1 < MERGE_BATCH && ut >= a.t[qt + 1].blk0) ++qt;
        const SparseBatchTensor &d = a.t[qt];
        const uint32_t ltile = ut - d.blk0;
        if (tid == 0 && (o > d.ocap || tc > d.ocap - o)) g_or(a.sc.fail, FAIL_MERGE_SPARSE);
        if (c) {
#pragma unroll
            for (uint32_t b = 0; b < 16; ++b) {
                if ((words[b >> 2] >> (8 * (b & 3))) & 0xffu) {
                    const uint32_t l = 16 * tid + b;
                    const uint32_t j = (ltile << TB_TILE_SHIFT) + l;
                    const float g = s_sum[l] / a.fworld;  // merged_grad[j] (cpu_optimize.cpp:49-55)
                    if (o < d.ocap && j < d.n) {
                        d.out_idx[o] = j;
                        d.out_val[o] = g;
                        if constexpr (OPT >= 0) {
                            const Step<OPT> opt(a, d);
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

hipError_t launch_emit(const SparseBatchArgs &a, int opt, uint32_t grid, hipStream_t s) {
    if (opt == 2) sb_tile<1, 2><<<grid, STG_WG, 0, s>>>(a);
    else if (opt == 1) sb_tile<1, 1><<<grid, STG_WG, 0, s>>>(a);
    else sb_tile<1, 0><<<grid, STG_WG, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sparse_batch_bucketing(const SparseBatchArgs &w, const RankStream *const *ranks, hipStream_t s,
                                         uint64_t *launches) {
    if (!w.nt || !w.world || w.world > TB_RANKS) return hipErrorInvalidValue;
    SparseBucketArgs b{};
    b.sc = w.sc;
    b.nt = w.nt;
    b.world = w.world;
    b.cap = w.cap;
    for (uint32_t q = 0; q < w.nt; ++q) {
        SparseBucketTensor &d = b.t[q];
        d.n = w.t[q].n;
        d.per_rank = w.t[q].ocap / w.world;
        d.tile0 = w.t[q].blk0;
        d.bpr = (uint32_t)(((uint64_t)d.per_rank + TB_PAIRS - 1) / TB_PAIRS);
        if (!d.per_rank) return hipErrorInvalidValue;
    }
    const auto bucket = [&](bool place) -> hipError_t {
        for (uint32_t r0 = 0; r0 < w.world; r0 += SB_RANKS) {
            const uint32_t nr = std::min<uint32_t>(SB_RANKS, w.world - r0);
            uint32_t blocks = 0;
            b.r0 = r0;
            for (uint32_t q = 0; q < w.nt; ++q) {
                SparseBucketTensor &d = b.t[q];
                for (uint32_t r = 0; r < nr; ++r) d.r[r] = ranks[q][r0 + r];
                d.blk0 = blocks;
                blocks += d.bpr * nr;  // (at most SB_PAIR_CAP / TB_PAIRS + MERGE_BATCH * SB_RANKS in all)
            }
            if (place) sb_bucket<true><<<blocks, STG_WG, 0, s>>>(b);
            else sb_bucket<false><<<blocks, STG_WG, 0, s>>>(b);
            count_launch(launches);
        }
        return hipGetLastError();
    };
    hipError_t e;
    if ((e = bucket(false)) != hipSuccess) return e;
    sb_scan<<<1, 1024, 0, s>>>(w);
    count_launch(launches);
    return bucket(true);
}

hipError_t launch_merge_sparse_batch(const SparseBatchArgs &w, const RankStream *const *ranks, int opt, int num_cu,
                                     hipStream_t s, uint64_t *launches) {
    if (const hipError_t e = launch_sparse_batch_bucketing(w, ranks, s, launches); e != hipSuccess) return e;
    // four workgroups of 36 KiB per CU; never more than the list can hold
    const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>(w.lcap, (uint32_t)std::max(num_cu, 1) * 4));
    sb_tile<0, -1><<<grid, STG_WG, 0, s>>>(w);
    sb_tscan<<<1, 1024, 0, s>>>(w);
    count_launch(launches, 3);
    return launch_emit(w, opt, grid, s);
}

}  // namespace stg
