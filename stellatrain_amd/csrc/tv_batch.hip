// tv_batch.hip -- threshold-v over a table of buckets in one launch (gfx950):
// the scan of the one-call send path (stg_merge_send_batch_device) for a
// threshold-v handle.
//
// Semantics: tv.hip's, per task (ThresholdvCompressor::impl_naive,
// thresholdv.cpp:40-83): |x| >= t emitted in index order while fewer than cap
// were found, every qualifier counted, gmax by the reference's NaN-restart
// rule, the AIMD update in double, *count_out = min(cnt, cap).  The emission is
// in position order and the fold sees every range's count and maximum, so the
// result does not depend on how many ranges a task is cut into: a task here
// gives tv_pass's bits although the two pick different range counts.
//
// Structure: tv_pass's range body -- 1024-thread workgroups, 16 waves, a
// rolling pipeline of SCAN_D nontemporal float4 buffer loads per lane, the
// qualifiers listed in LDS (LCAP entries), an in-order re-scan of a range whose
// list overflowed -- over up to SEND_BATCH tasks whose table travels by value
// in the kernel arguments.  One ticket counter per launch (the workspace's, so
// per-tensor and batched launches on one workspace interleave): ticket r maps to
// (task, range) through the host-computed first ranges (blk0), as batch_item
// deals workgroups.  The look-back of a range reads only its own task's earlier
// ranges: they drew earlier tickets, so running or finished workgroups hold
// them (no co-residency needed).  Every wait is bounded by spin_expired; on
// expiry the sticky failure word is set and the task's count poisoned.
//
// Error feedback: with a residual the streaming waves also store every float4
// they load to the residual (the gathered grad[0] is final when the scan
// starts), and the lane that folds the n % 4 tail stores that: the separate
// 8 n-byte copy pass of the per-tensor sequence is gone.  Nothing is zeroed
// here (ef_pack_batch_dc, send_batch.hip).
//
// Bound: HBM, 4 bytes read (+ 4 written under error feedback) per element; at
// the 60,000-float tensors the path is for, launch latency: four ranges per
// task, 16 tasks per launch.
#include <algorithm>

#include "ws.h"

namespace stg {

namespace {

typedef unsigned int u4v __attribute__((ext_vector_type(4)));
typedef float f4v __attribute__((ext_vector_type(4)));

constexpr uint32_t TWG = 1024;        // threads per workgroup (16 waves), as tv_pass
constexpr uint32_t TNW = TWG / 64;
constexpr uint32_t SCAN_D = 6;        // float4 loads in flight per lane, as tv_pass
constexpr uint32_t LCAP = TV_SCAP;    // qualifiers listed in LDS per range
static_assert(TV_BATCH_RANGE * 16 < (1u << 28), "a range fits one buffer descriptor");

__global__ void tvb_init_state(KeyState *st, const RSel *rs) {
    st->t = u2f(rs->prefix);
    st->inc = 0.f;
    st->init = 1;
}

// Range w of a task's G in float4 units; the ragged n % 4 tail belongs to the
// last range (tv.hip's split).
struct TvbRange {
    uint64_t lo, len;
};
__device__ __forceinline__ TvbRange tvb_range(uint64_t n4, uint32_t G, uint32_t w) {
    const uint64_t per = n4 / G, rem = n4 % G;
    TvbRange r;
    r.lo = w * per + std::min<uint64_t>(w, rem);
    r.len = per + (w < rem ? 1u : 0u);
    return r;
}

struct TvbCtl {
    uint64_t *desc;      // per ticket of the launch: {tag:32 | qualifier count:32}
    uint64_t *rmax;      // per ticket: {tag:32 | max |x| bits:32}
    uint64_t *ticket;    // ranges taken: monotonic over the workspace's launches
    uint32_t *fail;      // the workspace's sticky failure word
    uint32_t total;      // ranges of this launch
};

__global__ void __launch_bounds__(TWG, 8) tv_pass_batch(TvBatch tb, TvbCtl ctl) {
    __shared__ uint32_t s_pos[LCAP];
    __shared__ float s_val[LCAP];
    __shared__ uint32_t s_n, s_r, s_cnt[TNW], s_max[TNW];
    __shared__ uint64_t s_P, s_psum[TNW];
    __shared__ uint32_t sh[TNW + 1];
    const uint32_t tid = threadIdx.x;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    if (tid == 0) {
        s_n = 0;
        s_r = (uint32_t)(g_add(ctl.ticket, 1ull) - tb.base);
    }
    __syncthreads();
    const uint32_t rg = (uint32_t)__builtin_amdgcn_readfirstlane(s_r);  // ranges in ticket order
    if (rg >= ctl.total) {  // (never: the launch has `total` workgroups and the host keeps base)
        if (tid == 0) g_or(ctl.fail, FAIL_SPIN_TIMEOUT);
        return;
    }
    uint32_t b = 0;
    while (b + 1 < tb.nt && rg >= tb.t[b + 1].blk0) ++b;
    const TvBatchTask &a = tb.t[b];
    const uint32_t G = a.ranges, r = rg - a.blk0;
    uint64_t *desc = ctl.desc + a.blk0, *rmax = ctl.rmax + a.blk0;
    // read before this range's count is published: the task's last range
    // rewrites the state only after every range's count is in
    const float t = a.state->t;
    const uint64_t n = a.n, n4 = n / 4;
    const TvbRange R = tvb_range(n4, G, r);
    const float *src = a.src;
    float *resid = a.resid;
    // the residual takes float4 stores where it and the bucket are both on 16
    // bytes (a range starts a multiple of 16 bytes into either), else scalar ones
    const bool rvec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(resid)) & 15u) == 0;
    // the range as a bounded buffer: lanes past it read zeros
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(src + R.lo * 4), 0, (uint32_t)(R.len * 16), 0x00020000);
    const uint32_t steps = (uint32_t)((R.len + 63) / 64);  // 64 float4 per wave step
    const uint32_t mine = steps > wave ? (steps - wave + TNW - 1) / TNW : 0u;
    auto load = [&](uint32_t m) -> float4 {
        uint32_t voff = (wave * 64 + lane) * 16u;
        asm volatile("" : "+v"(voff));
        const u4v q = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff + m * (TNW * 1024u), 0, 2 /* nt */);
        return make_float4(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w));
    };
    uint32_t cnt = 0, mx = 0;
    float4 v[SCAN_D];
#pragma unroll
    for (uint32_t u = 0; u < SCAN_D; ++u) v[u] = load(u);
    for (uint32_t m0 = 0; m0 < mine; m0 += SCAN_D) {
#pragma unroll
        for (uint32_t u = 0; u < SCAN_D; ++u) {
            // consume the slot before loading into it (as tv_pass)
            const float4 x = v[u];
            const uint32_t f = ((m0 + u) * TNW + wave) * 64 + lane;  // float4 within the range
            const bool in = f < R.len;
            const float a0 = fabsf(x.x), a1 = fabsf(x.y), a2 = fabsf(x.z), a3 = fabsf(x.w);
            if (in) mx = max(mx, max(max(f2u(a0), f2u(a1)), max(f2u(a2), f2u(a3))));
            if (in && resid) {  // f < R.len: elements (R.lo + f) * 4 .. + 3 < n4 * 4 <= n
                float *o = resid + (R.lo + f) * 4;
                if (rvec) {
                    __builtin_nontemporal_store(f4v{x.x, x.y, x.z, x.w}, reinterpret_cast<f4v *>(o));
                } else {
                    o[0] = x.x; o[1] = x.y; o[2] = x.z; o[3] = x.w;
                }
            }
            const uint32_t q = in ? ((uint32_t)(a0 >= t) | ((uint32_t)(a1 >= t) << 1) | ((uint32_t)(a2 >= t) << 2) |
                                     ((uint32_t)(a3 >= t) << 3))
                                  : 0u;
            if (__ballot(q != 0) && q) {  // rare: list this lane's qualifiers
                const uint32_t c = (uint32_t)__popc(q);
                cnt += c;
                uint32_t o = atomicAdd(&s_n, c);
                const uint32_t p0 = (uint32_t)((R.lo + f) * 4);
                const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    if ((q >> j) & 1u) {
                        if (o < LCAP) { s_pos[o] = p0 + j; s_val[o] = xs[j]; }
                        ++o;
                    }
                }
            }
            v[u] = load(m0 + u + SCAN_D);
        }
    }
    // the ragged tail (n % 4 elements) closes the task's last range
    if (r == G - 1 && tid == 0) {
        for (uint64_t e = n4 * 4; e < n; ++e) {
            const float x = src[e], ax = fabsf(x);
            if (resid) resid[e] = x;
            mx = max(mx, f2u(ax));
            if (ax >= t) {
                const uint32_t o = atomicAdd(&s_n, 1u);
                ++cnt;
                if (o < LCAP) { s_pos[o] = (uint32_t)e; s_val[o] = x; }
            }
        }
    }
    cnt = wave_sum(cnt);
    mx = wave_max(mx);
    if (lane == 0) { s_cnt[wave] = cnt; s_max[wave] = mx; }
    __syncthreads();
    const uint32_t listed = s_n;
    uint32_t c = 0;
    for (uint32_t i = 0; i < TNW; ++i) c += s_cnt[i];
    if (tid == 0) {  // publish: the tagged maximum and the tagged count (no order between them)
        uint32_t m = 0;
        for (uint32_t i = 0; i < TNW; ++i) m = max(m, s_max[i]);
        st_sc1(&rmax[r], ((uint64_t)tb.tag << 32) | m);
        st_sc1(&desc[r], ((uint64_t)tb.tag << 32) | c);
    }
    // look-back: the counts of the task's ranges 0 .. r-1, one per thread in
    // one round trip; stale ones are polled by their lane with s_sleep
    uint64_t Pl = 0;
    bool gave_up = false;
    constexpr uint32_t LB = (TV_MAXG + TWG - 1) / TWG;  // earlier ranges per thread, all loaded at once
    uint64_t dl[LB];
#pragma unroll
    for (uint32_t q = 0; q < LB; ++q) {
        const uint32_t i = tid + q * TWG;
        dl[q] = i < r ? ld_sc1(&desc[i]) : (uint64_t)tb.tag << 32;
    }
#pragma unroll
    for (uint32_t q = 0; q < LB; ++q) {
        const uint32_t i = tid + q * TWG;
        uint64_t d = dl[q], st = 0;
        for (uint32_t spins = 0; (uint32_t)(d >> 32) != tb.tag; ++spins) {
            __builtin_amdgcn_s_sleep(8);
            d = ld_sc1(&desc[i]);
            if (spin_expired(spins, st)) { gave_up = true; break; }  // 200 ms: the count is poisoned below
        }
        Pl += (uint32_t)d;
    }
    if (gave_up) g_or(ctl.fail, FAIL_SPIN_TIMEOUT);
    Pl = wave_sum64(Pl);
    if (lane == 0) s_psum[wave] = Pl;
    __syncthreads();
    if (tid == 0) {
        uint64_t t2 = 0;
        for (uint32_t i = 0; i < TNW; ++i) t2 += s_psum[i];
        s_P = t2;
    }
    __syncthreads();
    const uint64_t P = s_P;
    const uint32_t cap_e = a.cap;
    if (P < cap_e && c) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(c, cap_e - P);
        if (listed <= LCAP) {
            // position order: rank = listed entries with a smaller position
            for (uint32_t e = tid; e < listed; e += TWG) {
                const uint32_t p = s_pos[e];
                uint32_t rk = 0;
                for (uint32_t x = 0; x < listed; ++x) rk += s_pos[x] < p;
                if (rk < m) {
                    a.idx[P + rk] = p;
                    a.val[P + rk] = s_val[e];
                }
            }
        } else {
            // the range's list overflowed: its qualifiers again, in order
            const uint64_t units = R.len + (r == G - 1 && n % 4 ? 1u : 0u);  // + the ragged tail
            uint64_t base = 0;
            for (uint64_t f0 = 0; f0 < units && base < m; f0 += TWG) {
                const uint64_t f = f0 + tid;
                uint32_t q = 0;
                float xs[4] = {0.f, 0.f, 0.f, 0.f};
                if (f < units) {
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) {
                        const uint64_t e = (R.lo + f) * 4 + j;
                        if (e < n) {
                            xs[j] = src[e];
                            q |= (uint32_t)(fabsf(xs[j]) >= t) << j;
                        }
                    }
                }
                uint32_t total;
                const uint32_t ex = blk_excl_scan<TNW>((uint32_t)__popc(q), sh, &total);
                uint64_t o = base + ex;
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    if ((q >> j) & 1u) {
                        if (o < m) {
                            a.idx[P + o] = (uint32_t)((R.lo + f) * 4 + j);
                            a.val[P + o] = xs[j];
                        }
                        ++o;
                    }
                }
                base += total;
            }
        }
    }
    // the task's last range has seen every earlier count (the look-back), and
    // each range stored its maximum before its count: fold them
    if (r != G - 1) return;
    // gmax by the reference's NaN-restart rule (tv.hip): the maximum of the
    // elements after the bucket's last NaN, or that NaN when it is the last
    // element.  A range's maximum of magnitude bits is above inf's exactly
    // when the range holds a NaN; only the last such range is read again.
    constexpr uint32_t INF_BITS = 0x7f800000u;
    uint32_t gm = 0, hn = 0;  // hn: 1 + the last range with a NaN
    for (uint32_t i = tid; i < G; i += TWG) {  // every range's tagged maximum
        uint64_t x = ld_sc1(&rmax[i]);
        uint64_t st = 0;
        for (uint32_t spins = 0; (uint32_t)(x >> 32) != tb.tag; ++spins) {
            __builtin_amdgcn_s_sleep(8);
            x = ld_sc1(&rmax[i]);
            if (spin_expired(spins, st)) { g_or(ctl.fail, FAIL_SPIN_TIMEOUT); break; }
        }
        gm = max(gm, (uint32_t)x);
        if ((uint32_t)x > INF_BITS) hn = max(hn, i + 1u);
    }
    const uint64_t cntall = P + c;
    gm = wave_max(gm);
    hn = wave_max(hn);
    if (lane == 0) { s_max[wave] = gm; s_cnt[wave] = hn; }
    __syncthreads();
    uint32_t hn_all = 0;
    for (uint32_t i = 0; i < TNW; ++i) hn_all = max(hn_all, s_cnt[i]);
    __syncthreads();
    if (hn_all) {  // rare and uniform: a NaN somewhere in the bucket
        const uint32_t rn = hn_all - 1u;
        const TvbRange Rn = tvb_range(n4, G, rn);
        const uint64_t e0 = Rn.lo * 4, e1 = rn == G - 1 ? n : (Rn.lo + Rn.len) * 4;  // (the last range has the ragged tail)
        uint32_t pl = 0;  // 1 + the range's last NaN element
        for (uint64_t e = e0 + tid; e < e1; e += TWG)
            if (f2u(fabsf(src[e])) > INF_BITS) pl = (uint32_t)(e - e0) + 1u;
        pl = wave_max(pl);
        if (lane == 0) s_cnt[wave] = pl;
        __syncthreads();
        uint32_t pl_all = 0;
        for (uint32_t i = 0; i < TNW; ++i) pl_all = max(pl_all, s_cnt[i]);
        const uint64_t pn = e0 + pl_all - 1u;  // the bucket's last NaN (pl_all >= 1: the range's maximum said so)
        gm = 0;
        for (uint64_t e = pn + 1 + tid; e < e1; e += TWG) gm = max(gm, f2u(fabsf(src[e])));
        for (uint32_t i = rn + 1 + tid; i < G; i += TWG) gm = max(gm, (uint32_t)ld_sc1(&rmax[i]));
        if (pl_all && pn + 1 == n) gm = f2u(fabsf(src[pn]));  // ends in a NaN: that NaN
        gm = wave_max(gm);
        if (lane == 0) s_max[wave] = gm;
        __syncthreads();
    }
    if (tid == 0) {
        uint32_t g = 0;
        for (uint32_t i = 0; i < TNW; ++i) g = max(g, s_max[i]);
        const float gmax = n ? u2f(g) : -1.f;
        float nt = t;
        if ((uint64_t)a.k > cntall) nt = (float)((double)t * 0.99);
        else if ((uint64_t)a.k < cntall) nt = (float)fma(0.01 * (double)cntall / (double)a.k, (double)gmax, (double)t);
        a.state->t = nt;
        a.state->init = 1;
        *a.count_out = (uint32_t)std::min<uint64_t>(cntall, a.cap);
        if (ld_sc1(ctl.fail)) *a.count_out = POISON_COUNT;  // a bounded wait gave up: untrusted output
    }
}

}  // namespace

hipError_t launch_tv_batch(const TvBatch &w, uint32_t ranges, const DevWS &ws, hipStream_t s) {
    if (!w.nt || !ranges) return hipSuccess;
    if (ranges > TV_MAXG) return hipErrorInvalidValue;  // the range words hold TV_MAXG pairs
    TvbCtl c;
    c.desc = reinterpret_cast<uint64_t *>(ws.tile_cnt);
    c.rmax = reinterpret_cast<uint64_t *>(ws.tile_aux);
    c.ticket = ws.tv_ticket;
    c.fail = ws.fail;
    c.total = ranges;
    tv_pass_batch<<<ranges, TWG, 0, s>>>(w, c);
    return hipGetLastError();
}

hipError_t launch_tv_first(const float *src, size_t n, uint32_t k, KeyState *state, const DevWS &ws, int num_cu,
                           hipStream_t s) {
    const uint32_t rank = (uint32_t)std::min<uint64_t>(k, n - 1);
    const hipError_t e = launch_radix_select(src, n, 0xffffffffu, 0, rank, ws, num_cu, s);
    if (e != hipSuccess) return e;
    tvb_init_state<<<1, 1, 0, s>>>(state, ws.rsel);
    return hipGetLastError();
}

}  // namespace stg
