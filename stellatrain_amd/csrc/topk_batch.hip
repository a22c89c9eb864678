// topk_batch.hip -- exact top-k by |x| for up to SEND_BATCH buckets per group
// of launches (gfx950): the select and ordered emission of
// stg_merge_send_batch_device on a "topk_exact" handle.
//
// Semantics are topk.hip's intended operator (TopkCompressor::impl_nth_element,
// compress/topk.cpp:28-46, without its two defects): the min(k, n) largest
// |x| of the bucket, ties at the k-th magnitude T taken in index order, emitted
// in index order with index + idx_offset; the count is the capacity
// (topk.cpp:25).  Keys are bits & 0x7fffffff, so a NaN ranks above infinity.
//
// The per-tensor route (topk1.hip, topk.hip) spends two to five dependent
// launches on every bucket.  Here a group of tasks -- a by-value table of up to
// SEND_BATCH, one 256-thread workgroup per TV_TILE floats, workgroups dealt by
// host-computed first-tile offsets (blk0) -- shares FIVE launches, whatever the
// number of slots in use:
//   tkb_level<0>  bits 30..20 of T: every tile's keys into the task's level-1
//                 bins; the residual receives what the pass loads (the gathered
//                 bucket is final by then);
//   tkb_level<1>  bits 19..9, over the keys in the level-1 bin;
//   tkb_level<2>  bits 8..0, over the keys in the level-2 bin: T, the number of
//                 keys above it, and the key's state (t = T, init = 1);
//   tkb_count     per tile: keys > T and == T;
//   tkb_emit      every tile sums the counts of its task's earlier tiles (at
//                 most the group's tile cap of them), writes its winners at
//                 their offsets, a share of the (0, 0.0f) slots [min(k, n), W)
//                 and, in the task's first tile, the count.
// The splits (11 / 11 / 9 bits) are select.h's.  Each level's pick is run by
// the task's last-arriving workgroup (a per-task counter, as last_workgroup in
// select.h: the flag is read back from LDS after a barrier, so the branch is
// uniform), which then zeroes the bins and the counter for the next group.
// NO workgroup waits on another: ordering comes from the stream order of the
// five launches and from that counter.  Histograms are integer atomics only,
// so the result does not depend on the order of arrival.
//
// Bounds.  A group holds at most topk_batch_tile_cap(num_cu) tiles, 32 KiB
// each, read once from HBM and four more times from the cache; the passes are
// latency-bound (one wave of workgroups each), which is what the batching is
// for: 256 buckets of 60,000 floats take 16 x 5 launches instead of 256 x 2..5.
#include <algorithm>

#include "tile.h"

namespace stg {

namespace {

__device__ __forceinline__ uint32_t magb(uint32_t bits) { return bits & 0x7fffffffu; }

template <int LEVEL> struct Lv;
template <> struct Lv<0> { static constexpr uint32_t SHIFT = 20, NB = 2048, OFF = 0; };
template <> struct Lv<1> { static constexpr uint32_t SHIFT = 9, NB = 2048, OFF = 2048; };
template <> struct Lv<2> { static constexpr uint32_t SHIFT = 0, NB = 512, OFF = 4096; };

__device__ __forceinline__ void load_task_tile(const TopkBatchTask &a, size_t base, float4 (&v)[TILE_U]) {
    if ((reinterpret_cast<uintptr_t>(a.src) & 15u) == 0) load_tile<true>(a.src, a.n, base, 0xffffffffu, v);
    else load_tile<false>(a.src, a.n, base, 0xffffffffu, v);
}

// The tile as loaded to the residual: 16-byte stores for a whole tile when
// source and residual are both on 16 bytes (the phase the tile's loads
// vectorise at), dword stores otherwise.
__device__ __forceinline__ void store_resid(const TopkBatchTask &a, size_t base, const float4 (&v)[TILE_U]) {
    const bool vec = ((reinterpret_cast<uintptr_t>(a.src) | reinterpret_cast<uintptr_t>(a.resid)) & 15u) == 0;
    if (vec && base + TV_TILE <= a.n) {
        float4 *p = reinterpret_cast<float4 *>(a.resid + base) + threadIdx.x;
#pragma unroll
        for (uint32_t u = 0; u < TILE_U; ++u) p[u * STG_WG] = v[u];
        return;
    }
#pragma unroll
    for (uint32_t u = 0; u < TILE_U; ++u) {
        const size_t e = base + 4 * ((size_t)u * STG_WG + threadIdx.x);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e + j < a.n) a.resid[e + j] = comp(v[u], j);
    }
}

// The bin holding descending rank `rank` among the level's NB bins, by the
// task's last workgroup (the other tiles' bin atomics are device-visible: they
// drained before counting themselves done); the bins are zeroed behind it.
template <int LEVEL>
__device__ __forceinline__ void pick(const TopkBatchTask &a, uint32_t prefix, uint32_t *sh) {
    using L = Lv<LEVEL>;
    constexpr uint32_t PER = L::NB / STG_WG;
    __shared__ uint32_t s_bin, s_before;
    TopkBatchSel *const S = a.sel;
    const uint32_t t = threadIdx.x;
    const uint32_t rank = LEVEL == 0 ? a.kk - 1u : S->rank;  // (written by the previous launch)
    uint32_t c[PER], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < PER; ++j) {  // top-down: thread t holds bins NB - 1 - (PER t + j)
        c[j] = ld_sc1(&S->hist[L::OFF + L::NB - 1u - (PER * t + j)]);
        sum += c[j];
    }
    if (t == 0) { s_bin = 0xffffffffu; s_before = 0; }
    uint32_t tot;
    const uint32_t before = wg_excl_scan(sum, sh, &tot);  // (its barriers order the s_bin reset)
    if (sum && rank >= before && rank - before < sum) {
        uint32_t acc = before;
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) {
            if (rank - acc < c[j]) { s_bin = L::NB - 1u - (PER * t + j); s_before = acc; break; }
            acc += c[j];
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < PER; ++j)
        if (c[j]) st_sc1(&S->hist[L::OFF + L::NB - 1u - (PER * t + j)], 0u);
    __syncthreads();
    if (t == 0) {
        const bool hit = s_bin != 0xffffffffu;  // (a rank out of range cannot happen: kk <= n keys were counted)
        const uint32_t b = hit ? s_bin : 0u, bb = hit ? s_before : 0u;
        const uint32_t T = prefix | (b << L::SHIFT);
        S->prefix = T;
        S->rank = rank - bb;
        S->cnt_gt = (LEVEL == 0 ? 0u : S->cnt_gt) + bb;
        st_sc1(&S->done[LEVEL], 0u);
        if (LEVEL == 2) {  // the key's hint for the per-tensor route: this call's T
            a.state->t = u2f(T);
            if (!a.state->init) a.state->inc = TOPK_HINT_SEED;
            a.state->init = 1;
        }
    }
}

template <int LEVEL>
__global__ void __launch_bounds__(STG_WG) tkb_level(TopkBatch w) {
    using L = Lv<LEVEL>;
    __shared__ uint32_t h[L::NB];
    __shared__ uint32_t sh[STG_WAVES + 1];
    __shared__ uint32_t s_last;
    const TopkBatchTask &a = w.t[batch_item(w.t, w.nt)];
    const uint32_t tile = blockIdx.x - a.blk0;
    const size_t base = (size_t)tile * TV_TILE;
    for (uint32_t i = threadIdx.x; i < L::NB; i += STG_WG) h[i] = 0;
    const uint32_t prefix = LEVEL == 0 ? 0u : a.sel->prefix;  // (the previous launch's pick)
    float4 v[TILE_U];
    load_task_tile(a, base, v);
    if (LEVEL == 0 && a.resid) store_resid(a, base, v);
    __syncthreads();
    if (a.kk) {
#pragma unroll
        for (uint32_t u = 0; u < TILE_U; ++u) {
            const size_t e = base + 4 * ((size_t)u * STG_WG + threadIdx.x);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t key = magb(f2u(comp(v[u], j)));
                // the bits above this level's equal the prefix's (level 1: every key)
                const bool in = LEVEL == 0 || (key >> (L::SHIFT + (LEVEL == 1 ? 11 : 9))) ==
                                                  (prefix >> (L::SHIFT + (LEVEL == 1 ? 11 : 9)));
                if (e + j < a.n && in) atomicAdd(&h[(key >> L::SHIFT) & (L::NB - 1u)], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t *const gh = a.sel->hist + L::OFF;
    for (uint32_t i = threadIdx.x; i < L::NB; i += STG_WG)
        if (h[i]) g_add(&gh[i], h[i]);
    // the task's last workgroup picks
    __builtin_amdgcn_s_waitcnt(0);  // this thread's memory operations are done
    __syncthreads();
    if (threadIdx.x == 0) s_last = g_add(&a.sel->done[LEVEL], 1u) == a.tiles - 1u ? 1u : 0u;
    __syncthreads();
    if (s_last && a.kk) pick<LEVEL>(a, prefix, sh);
    else if (s_last && threadIdx.x == 0) st_sc1(&a.sel->done[LEVEL], 0u);
}

__global__ void __launch_bounds__(STG_WG) tkb_count(TopkBatch w) {
    __shared__ uint32_t s_c[2 * STG_WAVES];
    const TopkBatchTask &a = w.t[batch_item(w.t, w.nt)];
    const uint32_t tile = blockIdx.x - a.blk0;
    const size_t base = (size_t)tile * TV_TILE;
    const uint32_t T = a.sel->prefix;
    float4 v[TILE_U];
    load_task_tile(a, base, v);
    uint32_t gt = 0, eq = 0;
#pragma unroll
    for (uint32_t u = 0; u < TILE_U; ++u) {
        const size_t e = base + 4 * ((size_t)u * STG_WG + threadIdx.x);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t key = magb(f2u(comp(v[u], j)));
            const bool in = e + j < a.n && a.kk;
            gt += in && key > T;
            eq += in && key == T;
        }
    }
    gt = wave_sum(gt);
    eq = wave_sum(eq);
    if (__lane_id() == 0) { s_c[threadIdx.x >> 6] = gt; s_c[STG_WAVES + (threadIdx.x >> 6)] = eq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t g = 0, q = 0;
        for (uint32_t i = 0; i < STG_WAVES; ++i) { g += s_c[i]; q += s_c[STG_WAVES + i]; }
        w.tile_gt[blockIdx.x] = g;
        w.tile_eq[blockIdx.x] = q;
    }
}

// A winner ranked past kk: the select's counts and the tiles disagree (never
// with a consistent select).  As topk.hip: the write is dropped, the failure
// word gets FAIL_SELECT and the count is poisoned.
__device__ __forceinline__ void select_broken(const TopkBatch &w, const TopkBatchTask &a) {
    g_or(w.fail, FAIL_SELECT);
    __hip_atomic_fetch_max(gp(a.count_out), POISON_COUNT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(STG_WG) tkb_emit(TopkBatch w) {
    __shared__ uint32_t s_wt[TILE_U * STG_WAVES + 1];
    __shared__ uint32_t s_p[2 * STG_WAVES];
    const TopkBatchTask &a = w.t[batch_item(w.t, w.nt)];
    const uint32_t tile = blockIdx.x - a.blk0, tid = threadIdx.x;
    const size_t base = (size_t)tile * TV_TILE;
    const uint32_t T = a.sel->prefix;
    const uint32_t need_eq = a.kk - std::min(a.kk, a.sel->cnt_gt);  // ties to take, in index order
    // the task's earlier tiles' counts (tkb_count's, the previous launch)
    uint32_t pg = 0, pe = 0;
    for (uint32_t i = a.blk0 + tid; i < blockIdx.x; i += STG_WG) { pg += w.tile_gt[i]; pe += w.tile_eq[i]; }
    pg = wave_sum(pg);
    pe = wave_sum(pe);
    if (__lane_id() == 0) { s_p[tid >> 6] = pg; s_p[STG_WAVES + (tid >> 6)] = pe; }
    __syncthreads();
    uint32_t gt_before = 0, eq_before = 0;
    for (uint32_t i = 0; i < STG_WAVES; ++i) { gt_before += s_p[i]; eq_before += s_p[STG_WAVES + i]; }
    const uint32_t cg = w.tile_gt[blockIdx.x], ce = w.tile_eq[blockIdx.x];
    if (cg || (ce && eq_before < need_eq)) {  // uniform per workgroup
        float4 v[TILE_U];
        load_task_tile(a, base, v);
        uint32_t qg = 0, qe = 0;
#pragma unroll
        for (uint32_t u = 0; u < TILE_U; ++u) {
            const size_t e = base + 4 * ((size_t)u * STG_WG + tid);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t key = magb(f2u(comp(v[u], j)));
                if (e + j < a.n) {
                    if (key > T) qg |= 1u << (u * 4 + j);
                    else if (key == T) qe |= 1u << (u * 4 + j);
                }
            }
        }
        uint32_t sr[TILE_U * 4], tot;
        tile_ranks(qe, sr, s_wt, &tot);
        uint32_t qw = qg;
#pragma unroll
        for (uint32_t b = 0; b < TILE_U * 4; ++b)
            if (((qe >> b) & 1u) && eq_before + sr[b] < need_eq) qw |= 1u << b;
        tile_ranks(qw, sr, s_wt, &tot);
        const uint32_t win_before = gt_before + std::min(eq_before, need_eq);
#pragma unroll
        for (uint32_t u = 0; u < TILE_U; ++u) {
            const size_t e = base + 4 * ((size_t)u * STG_WG + tid);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t b = u * 4 + j;
                if ((qw >> b) & 1u) {
                    const uint32_t slot = win_before + sr[b];
                    if (slot >= a.kk) { select_broken(w, a); continue; }  // an inconsistent select: surfaced
                    a.idx[slot] = (uint32_t)(e + j) + (uint32_t)a.idx_offset;
                    a.val[slot] = comp(v[u], j);
                }
            }
        }
    }
    // the unused slots the engine still sends (compress.cpp:60-64): the staging
    // is not zeroed between calls, so every tile writes its share of them
    for (uint64_t s = (uint64_t)a.kk + (uint64_t)tile * STG_WG + tid; s < a.slots; s += (uint64_t)a.tiles * STG_WG) {
        a.idx[s] = 0u;
        a.val[s] = 0.f;
    }
    // the count, then the failure word again (topk.hip's order: a tile whose
    // select_broken came before that second read is seen there and poisoned
    // here; one that came after it stores its poison after ours)
    if (tile == 0 && tid == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        if (!(ld_sc1(w.fail) & FAIL_SELECT)) {
            st_sc1(a.count_out, a.cap);
            __builtin_amdgcn_s_waitcnt(0);
            if (ld_sc1(w.fail) & FAIL_SELECT)
                __hip_atomic_fetch_max(gp(a.count_out), POISON_COUNT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

hipError_t launch_topk_batch(const TopkBatch &w, uint32_t tiles, hipStream_t s) {
    if (!w.nt || !tiles) return hipSuccess;
    tkb_level<0><<<tiles, STG_WG, 0, s>>>(w);
    tkb_level<1><<<tiles, STG_WG, 0, s>>>(w);
    tkb_level<2><<<tiles, STG_WG, 0, s>>>(w);
    tkb_count<<<tiles, STG_WG, 0, s>>>(w);
    tkb_emit<<<tiles, STG_WG, 0, s>>>(w);
    return hipGetLastError();
}

}  // namespace stg
