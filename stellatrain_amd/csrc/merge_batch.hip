// merge_batch.hip -- the world-1 MERGE decompress with the optimizer step fused
// into its emission (apply.hip: win_mark[_w], win_emit1t<4, SMART, WIRE>) for up
// to MERGE_BATCH parameter tensors per launch pair (gfx950).
//
// ModuleCpuOptimize::run (engine/modules/cpu_optimize.cpp:26-106) is one task
// per parameter tensor per iteration; a model has hundreds of them, most small,
// and a per-tensor call is launch-bound (two launches for ~10 KB of traffic).
// Here the tensors of a group share the two launches.  A workgroup learns its
// tensor from blockIdx (MergeTensor::blk0, host-computed, as the batched wire
// kernels do) and from then on works on that tensor's own slices and words:
//   * win0:  its winner words (zero between calls, re-zeroed by the emission);
//   * desc0: its tagged tile counts;
//   * ctl[slot]: its tile ticket, duplicate flag and failed-launch tag, each on
//     a 128-byte line of its own.
// Ordering: in the ticketed path a workgroup takes its tile from its tensor's
// ticket and waits only on lower tiles of the same tensor, which workgroups
// already running hold -- the per-tensor kernel's argument, unchanged: no
// co-residency is needed, and every wait is bounded by spin_expired.  A tensor
// without a repeated or out-of-range index copies its stream through (no
// ticket, no look-back) whatever its neighbours in the launch do.
//
// Every stream is read through the wire loaders (wire_dev.h), which take flag
// 0 (u32 / f32) as well; the per-element code is merge_dev.h, the text the
// per-tensor kernels compile, so parameters, state and merged streams agree
// with them bitwise.
#include <algorithm>

#include "ws.h"
#include "wire_dev.h"
#include "merge_dev.h"

namespace stg {

namespace {

// The election of every tensor of the group: win[j] = 1 + the last position of
// index j in the tensor's stream; any repeat or index >= n sets the slot's
// duplicate flag.  One workgroup per MERGE_BATCH_TILE pairs, the emission's
// partition, so both launches share blk0.
__global__ void __launch_bounds__(STG_WG) merge_mark_batch(MergeBatchArgs w) {
    const uint32_t t = batch_item(w.t, w.nt);
    const MergeTensor &d = w.t[t];
    MergeSlotCtl *c = w.ctl + t;
    const uint32_t tile = blockIdx.x - d.blk0;
    if (tile == 0 && threadIdx.x == 0) st_sc1(&c->ticket, 0ull);
    uint32_t *__restrict__ win = w.win + d.win0;
    const size_t m = d.m, n = d.n;
    const size_t wend = 8 * ((m - 1) / 8);  // m >= 1
#pragma unroll
    for (uint32_t q = 0; q < MERGE_BATCH_WP; ++q) {
        const size_t i = (size_t)tile * MERGE_BATCH_TILE + (size_t)q * STG_WG + threadIdx.x;
        if (i < m) {
            const uint32_t j = wire_get_idx(d.idx, d.flag, wend, i);
            if (j >= n || atomicMax(&win[j], (uint32_t)i + 1u) != 0u) g_or(&c->dup, 1u);
        }
    }
}

// (One winner's optimizer step, Step<OPT>: merge_dev.h, shared with
// merge_batch_world.hip.)

// win_emit1t<4, SMART, true> per tensor of the group (apply.hip): tiles in the
// tensor's own ticket order, tagged tile counts in its own desc slice, the
// look-back over its own lower tiles only.
template <int OPT>
__global__ void __launch_bounds__(STG_WG) merge_emit_batch(MergeBatchArgs w) {
    constexpr uint32_t WP = MERGE_BATCH_WP;
    __shared__ uint32_t sh[STG_WAVES + 1];
    __shared__ uint32_t s_tile, s_bad;
    __shared__ uint64_t s_P, s_psum[STG_WAVES];
    __shared__ uint32_t s_dup;
    const uint32_t tid = threadIdx.x, lane = __lane_id();
    const uint32_t t = batch_item(w.t, w.nt);
    const MergeTensor &d = w.t[t];
    MergeSlotCtl *c = w.ctl + t;
    const size_t m = d.m, n = d.n;
    const size_t wend = 8 * ((m - 1) / 8);  // m >= 1
    const uint32_t flag = d.flag;
    const uint32_t ntiles = (uint32_t)((m + MERGE_BATCH_TILE - 1) / MERGE_BATCH_TILE);
    uint32_t *__restrict__ win = w.win + d.win0;
    uint64_t *desc = w.desc + d.desc0;
    const Step<OPT> opt(w, d);
    if (tid == 0) s_dup = ld_sc1(&c->dup);
    __syncthreads();
    if (!s_dup) {
        // no index of this tensor repeats: the output is its stream (tile = the
        // tensor's block), whatever path its neighbours take
        const uint32_t tile = blockIdx.x - d.blk0;
        const size_t e = (size_t)tile * MERGE_BATCH_TILE + (size_t)WP * tid;
        uint32_t j[WP];
        float v[WP];
        if (e < m) {
            wire_idx_wp<WP>(d.idx, flag, wend, m, e, j);
            wire_val_wp<WP>(d.val, flag, wend, m, e, v);
        }
        float xp[WP], mp[WP], vp[WP];
        uint32_t lp[WP];
#pragma unroll
        for (uint32_t b = 0; b < WP; ++b) opt.load(e + b < m ? j[b] : 0u, xp[b], mp[b], vp[b], lp[b]);
#pragma unroll
        for (uint32_t b = 0; b < WP; ++b) opt.factors(vp[b], lp[b]);
#pragma unroll
        for (uint32_t b = 0; b < WP; ++b) {
            if (e + b < m) {
                const float g = (0.0f + v[b]) / 1.0f;  // merged_grad[j] (cpu_optimize.cpp:49-55), world 1
                d.out_idx[e + b] = j[b];
                d.out_val[e + b] = g;
                opt.step(j[b], g, xp[b], mp[b], vp[b], lp[b]);  // indices unique: updates commute
                win[j[b]] = 0;  // scratch back to zero for the next call
            }
        }
        if (tid == 0 && tile == ntiles - 1) {
            __builtin_amdgcn_s_waitcnt(0);
            *d.out_count = (uint32_t)m;  // no look-back for this tensor: nothing of it can have failed
        }
        return;
    }
    if (tid == 0) { s_tile = (uint32_t)g_add(&c->ticket, 1ull); s_bad = 0; }
    __syncthreads();
    const uint32_t tile = s_tile;
    const size_t e = (size_t)tile * MERGE_BATCH_TILE + (size_t)WP * tid;
    uint32_t j[WP];
    const uint32_t keep = e < m ? win_keep_t<WP, true>(static_cast<const uint32_t *>(d.idx), m, n, win, e, j, flag, wend)
                                : 0u;
    float v[WP];
    if (e < m) wire_val_wp<WP>(d.val, flag, wend, m, e, v);
    float xp[WP], mp[WP], vp[WP];
    uint32_t lp[WP];
    // the winners' parameter and state words, loaded under the look-back
#pragma unroll
    for (uint32_t b = 0; b < WP; ++b) opt.load((keep >> b & 1u) ? j[b] : 0u, xp[b], mp[b], vp[b], lp[b]);
#pragma unroll
    for (uint32_t b = 0; b < WP; ++b) opt.factors(vp[b], lp[b]);
    uint32_t tc;
    uint32_t r = wg_excl_scan((uint32_t)__popc(keep), sh, &tc);
    if (tid == 0) st_sc1(&desc[tile], ((uint64_t)w.tag << 32) | tc);
    {   // look-back over this tensor's tiles 0 .. tile-1, STG_WG per round trip
        uint64_t Pl = 0;
        bool gave = false;
        for (uint32_t i0 = 0; i0 < tile; i0 += STG_WG) {
            const uint32_t i = i0 + tid;
            uint64_t x = i < tile ? ld_sc1(&desc[i]) : 0ull;
            uint64_t st = 0;
            for (uint32_t spins = 0; i < tile && (uint32_t)(x >> 32) != w.tag; ++spins) {
                __builtin_amdgcn_s_sleep(4);
                x = ld_sc1(&desc[i]);
                if (spin_expired(spins, st)) { gave = true; break; }  // 200 ms: give up, poison the count
            }
            Pl += (uint32_t)x;
        }
        if (gave) s_bad = 1;
        Pl = wave_sum64(Pl);
        if (lane == 0) s_psum[tid >> 6] = Pl;
        __syncthreads();
        if (tid == 0) {
            uint64_t t2 = 0;
            for (uint32_t q = 0; q < STG_WAVES; ++q) t2 += s_psum[q];
            s_P = t2;
        }
    }
    __syncthreads();
    const uint64_t P = s_P;
    const bool bad = s_bad != 0;
    // a tile that gave up writes nothing, marks the scratch's sticky failure
    // word (stg_scatter_merge_check) and tags its own slot: this tensor's count
    // is poisoned, its neighbours' are not
    if (bad && tid == 0) {
        g_or(w.fail, FAIL_SPIN_TIMEOUT);
        st_sc1(&c->fail_tag, w.tag);
    }
#pragma unroll
    for (uint32_t b = 0; b < WP; ++b) {
        if (keep >> b & 1u) {
            const float g = (0.0f + v[b]) / 1.0f;
            if (!bad) {
                d.out_idx[P + r] = j[b];
                d.out_val[P + r] = g;
            }
            opt.step(j[b], g, xp[b], mp[b], vp[b], lp[b]);  // each index elected once: updates commute
            win[j[b]] = 0;  // scratch back to zero for the next call
            ++r;
        }
    }
    if (tid == 0 && tile == ntiles - 1) {
        __builtin_amdgcn_s_waitcnt(0);
        *d.out_count = (bad || ld_sc1(&c->fail_tag) == w.tag) ? POISON_COUNT : (uint32_t)(P + tc);
        // every tile of the tensor read the flag before publishing its count
        // (the look-back above saw them all): clear it for the slot's next tensor
        if (!bad) st_sc1(&c->dup, 0u);
    }
}

}  // namespace

hipError_t launch_merge_batch(const MergeBatchArgs &w, uint32_t blocks, int opt, hipStream_t s, uint64_t *launches) {
    if (!w.nt || !blocks) return hipSuccess;
    count_launch(launches, 2);  // the election and the emission
    merge_mark_batch<<<blocks, STG_WG, 0, s>>>(w);
    if (opt == 2) merge_emit_batch<2><<<blocks, STG_WG, 0, s>>>(w);
    else if (opt == 1) merge_emit_batch<1><<<blocks, STG_WG, 0, s>>>(w);
    else merge_emit_batch<0><<<blocks, STG_WG, 0, s>>>(w);
    return hipGetLastError();
}

}  // namespace stg
