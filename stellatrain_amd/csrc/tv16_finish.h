// tv16_finish.h -- what the three finishes of a thresholdv16 call repeat, once:
// tv16.hip finish_chunk (the batched scan's last chunk), tv16lfin.h (the fill
// launch's finish of a one-bucket call) and tv16lf2.h (the one-bucket scan
// launch's own finish), with the readers of their decision in tv16fill.hip and
// tv16wide.h.  Their results must agree bit for bit, so the rule each follows
// is written here and every site calls it.
//
// Reference: ThresholdvCompressor16::impl_simd_v2 after the streaming
// (thresholdv16.cpp:138-259) and the arithmetic around the regime-B heap fill
// (:261-293).
//
// Scalar arithmetic only: no memory access, no LDS, and no intrinsic but the
// count of leading zeros (clz32: __clz on the device, __builtin_clz on the
// host).  A host compiler takes the header as it is (tests/cpp/finish_units.cpp).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TV16_FN __host__ __device__ __forceinline__
#else
#define TV16_FN inline
#endif

#include "tv16_const.h"

namespace stg {
namespace tv16 {

constexpr uint32_t NO_RANK = 0xffffffffu;      // the ragged tail is not among the ranked entries
constexpr uint32_t POS_LIM = (1u << 20) - 1;   // right-first ranking: N <= POS_LIM (rf_key's 20-bit paths)
// what a ranking found among the first pops + 1 (lfin reports them in CallCtl pad[5])
constexpr uint32_t RF_TIES = 1u;  // equal sums
constexpr uint32_t RF_VIOL = 2u;  // a fast-path condition failed for a tied or late line

TV16_FN uint32_t fbits(float f) { return __builtin_bit_cast(uint32_t, f); }
TV16_FN float bitsf(uint32_t u) { return __builtin_bit_cast(float, u); }
TV16_FN uint32_t umin(uint32_t a, uint32_t b) { return b < a ? b : a; }
TV16_FN uint32_t clz32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__clz((int)x);
#else
    return (uint32_t)__builtin_clz(x);
#endif
}

// ---------------------------------------------------------------------------
// 1. the regime decision (thresholdv16.cpp:138-259), in three steps
// ---------------------------------------------------------------------------
struct Regime {
    uint32_t kb, r, lim;  // dst_len = 16 kb + r; lim lines fill it
    uint32_t c0, ct;      // pairs of the qualifying lines, then of the ragged tail (stage 3)
    uint32_t cnt, M, N;   // c0 + ct; lines the fill pops at most; the reference's candidate vector length
    bool regimeB, tail_cand, listw;  // listw: the window list holds the fill's lines
    float tail_key;
};

// the lines dst_len takes: the part of the head every chunk's emission needs
TV16_FN void regime_lines(Regime &R, uint32_t dst_len) {
    R.kb = dst_len / 16;
    R.r = dst_len % 16;
    R.lim = R.kb + (R.r ? 1u : 0u);
}
// the head: Qtot qualifying lines against dst_len
TV16_FN void regime_head(Regime &R, uint32_t dst_len, uint32_t Qtot) {
    regime_lines(R, dst_len);
    R.c0 = Qtot >= R.lim ? dst_len : 16u * Qtot;
}
// stage 3 looks at the ragged tail at all (only then is its sum taken)
TV16_FN bool regime_sums_tail(const Regime &R, uint32_t dst_len, uint32_t tl) { return R.c0 < dst_len && tl; }
// stage 3 (thresholdv16.cpp:212-236): sm is the tail's signed sum, added in
// order from 0.f; the tail qualifies whole, or joins the candidates with a
// line's key
// A site calls regime_no_tail, then regime_tail where regime_sums_tail holds.
TV16_FN void regime_no_tail(Regime &R) {
    R.ct = 0;
    R.tail_cand = false;
    R.tail_key = 0.f;
}
TV16_FN void regime_tail(Regime &R, float sm, float t, uint32_t tl, uint32_t dst_len) {
    if (sm * 16.0f >= t * (float)tl) R.ct = umin(dst_len - R.c0, tl);
    else { R.tail_cand = true; R.tail_key = sm * 16.0f / (float)tl; }
}
// after stage 3: the ordered scan left the output short (regime B).  On its
// own for a site that needs it ahead of the close.
TV16_FN bool regime_short(const Regime &R, uint32_t dst_len) { return R.c0 + R.ct < dst_len; }
// the close: the regime and what the fill has to find
TV16_FN void regime_close(Regime &R, uint32_t dst_len, uint32_t nb, uint32_t Qtot, uint32_t Wtot) {
    R.cnt = R.c0 + R.ct;
    R.regimeB = regime_short(R, dst_len);
    const uint32_t ncand = nb - Qtot;  // non-qualifying full lines
    R.M = R.regimeB ? umin((dst_len - R.cnt + 15u) / 16u, ncand) : 0u;
    R.listw = R.regimeB && Wtot >= R.M && Wtot + 1 <= CAND_CAP;
    R.N = ncand + (R.tail_cand ? 1u : 0u);
}

// ---------------------------------------------------------------------------
// 2. the AIMD step and the count (thresholdv16.cpp:243-259)
// ---------------------------------------------------------------------------
TV16_FN float next_threshold(float t, float inc, bool regimeB) {
    return regimeB ? (float)((double)t * 0.99) : t + inc;
}
TV16_FN uint32_t emitted_count(uint32_t dst_len, uint32_t nb, uint32_t tl) {
    const uint64_t n = (uint64_t)nb * 16 + tl;
    return n < dst_len ? (uint32_t)n : dst_len;
}

// ---------------------------------------------------------------------------
// 3. the Decision words (ws.h Decision): [0] = {tag:32 | flags:32},
//    [1] = {cnt:32 | M:32}, [2] = {Wtot:32 | tail key bits:32},
//    [3] = {Qtot:32 | t bits:32}
// ---------------------------------------------------------------------------
struct DecisionWords {
    uint64_t w[4];
};
TV16_FN uint64_t dec_word(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; }
TV16_FN uint32_t dec_hi(uint64_t w) { return (uint32_t)(w >> 32); }
TV16_FN uint32_t dec_lo(uint64_t w) { return (uint32_t)w; }
TV16_FN uint32_t decision_tag(uint32_t epoch) { return (epoch << 8) | TV16_TAG_DEC; }

TV16_FN uint32_t decision_flags(const Regime &R) {
    return R.regimeB ? (TV16_DEC_B | (R.tail_cand ? TV16_DEC_TAIL : 0u) | (R.listw ? TV16_DEC_WIN : 0u)) : 0u;
}
TV16_FN DecisionWords decision_pack(const Regime &R, uint32_t Wtot, uint32_t Qtot, float t, uint32_t tag) {
    DecisionWords d;
    d.w[0] = dec_word(tag, decision_flags(R));
    d.w[1] = dec_word(R.cnt, R.M);
    d.w[2] = dec_word(Wtot, fbits(R.tail_key));
    d.w[3] = dec_word(Qtot, fbits(t));
    return d;
}
// A ragged tail whose signed sum is NaN joins the reference's heap under a
// comparator that is then always false: only the literal heap reproduces what
// make_heap / pop_heap do with it (with 2^m - 1 candidates it climbs from the
// last leaf to the root and pops first), so every other way declines it.
TV16_FN bool nan_tail(uint32_t flags, uint32_t tail_bits) {
    return (flags & TV16_DEC_TAIL) && (tail_bits & 0x7fffffffu) > 0x7f800000u;
}
// the crew (tv16wide.h) orders the bucket: regime B with lines (or the tail)
// to fill, and the window does not hold them
TV16_FN bool crew_wants(uint32_t flags, uint32_t M, uint32_t mode, uint32_t tail_bits) {
    return (flags & TV16_DEC_B) && (M || (flags & TV16_DEC_TAIL)) && (!(flags & TV16_DEC_WIN) || mode == 4u) &&
           mode != 2u && !nan_tail(flags, tail_bits);  // mode 2 (tests): the literal heap for every regime-B bucket
}
struct DecisionView {
    uint32_t tag, flags, cnt, M, Wtot, tail_bits, Qtot, t_bits;
    uint32_t N, rem;  // the candidate vector's length; pairs still missing
    bool tail;        // the ragged tail is a candidate
};
TV16_FN DecisionView decision_unpack(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, uint32_t nb,
                                     uint32_t dst_len) {
    DecisionView v;
    v.tag = dec_hi(w0);
    v.flags = dec_lo(w0);
    v.cnt = dec_hi(w1);
    v.M = dec_lo(w1);
    v.Wtot = dec_hi(w2);
    v.tail_bits = dec_lo(w2);
    v.Qtot = dec_hi(w3);
    v.t_bits = dec_lo(w3);
    v.tail = (v.flags & TV16_DEC_TAIL) != 0;
    v.N = nb - v.Qtot + (v.tail ? 1u : 0u);
    v.rem = dst_len - v.cnt;
    return v;
}

// ---------------------------------------------------------------------------
// 4. the window [window_lo(bits(t)), bits(t)) just below t, and the ragged
//    tail's place in it
// ---------------------------------------------------------------------------
TV16_FN uint32_t window_lo(uint32_t tb) { return tb > TV16_WIN ? tb - TV16_WIN : 0u; }
TV16_FN bool tail_in_window(bool tail_cand, float tail_key, uint32_t tb) {
    return tail_cand && tail_key >= bitsf(window_lo(tb));
}
// its window offset as the scan bins a sum (bins of 256 ulps: offset >> 8)
TV16_FN uint32_t window_offset(uint32_t tb, uint32_t sum_bits) { return tb - 1u - sum_bits; }
TV16_FN uint32_t window_bin(uint32_t w) { return w >> 8; }

// ---------------------------------------------------------------------------
// 5. can the right-first ranking (tv16fill.hip (2), (3)) take this call?
// ---------------------------------------------------------------------------
TV16_FN bool rankers_can_take(const Regime &R, uint32_t Wtot, bool lists_ok, uint32_t mode, float t, uint32_t pos_lim) {
    const uint32_t tb = fbits(t);
    const bool tail_in = tail_in_window(R.tail_cand, R.tail_key, tb);
    const uint32_t W = Wtot + (tail_in ? 1u : 0u);
    return R.listw && lists_ok && R.N <= pos_lim && W != 0 && !mode &&
           // a -0.0 tail ties +0.0 sums in the reference's float compare, not in key order
           !(tail_in && (fbits(R.tail_key) & 0x80000000u)) &&
           // a tail key rounded up to t would sort above the window: the orderer takes it
           !(tail_in && !(R.tail_key < t)) &&
           !(R.tail_cand && R.tail_key != R.tail_key);  // a NaN tail: nan_tail
}

// ---------------------------------------------------------------------------
// 6. the pops: entry i of the fill's order goes to offset 16 i, less 16 - tl
//    after the ragged tail (rank tr, or NO_RANK), until rem pairs are out
// ---------------------------------------------------------------------------
TV16_FN uint32_t pop_offset(uint32_t i, uint32_t tr, uint32_t tl) { return 16u * i - (tr < i ? 16u - tl : 0u); }
TV16_FN uint32_t pop_len(uint32_t i, uint32_t tr, uint32_t tl, uint32_t off, uint32_t rem) {
    return umin(i == tr ? tl : 16u, rem - off);  // (off < rem)
}
TV16_FN uint32_t pops_p0(uint32_t rem) { return (rem + 15u) / 16u; }  // pops of full lines
// one rank past the pops, inside n entries: the conservative bound Ph the fast-path
// conditions use (the exact orderer counts its pops in (sum desc, index asc) order)
TV16_FN uint32_t pops_bound(uint32_t p, uint32_t n) { return umin(p + 1u, n - 1u); }
// Wk kept entries (the ragged tail among them or not) cannot cover rem
TV16_FN bool pops_short(uint32_t Wk, bool has_tail, uint32_t tl, uint32_t rem) {
    return 16u * Wk - (has_tail ? 16u - tl : 0u) < rem;
}
// start positions >= this are the last Ph + 1 of N
TV16_FN uint32_t pops_late(uint32_t N, uint32_t Ph) { return N > Ph + 1 ? N - (Ph + 1) : 0u; }
// the first rank whose output offset reaches rem
TV16_FN uint32_t pops_count(uint32_t rem, uint32_t tl, uint32_t tr) {
    const uint32_t p0 = pops_p0(rem);
    return tr < p0 ? (rem + (16u - tl) + 15u) / 16u : p0;
}
// ---------------------------------------------------------------------------
// 7. heap positions of libstdc++'s make_heap (node q = pos + 1 >= 1) and the
//    rankers' keys
// ---------------------------------------------------------------------------
TV16_FN uint32_t depth_of(uint32_t q) { return 31u - clz32(q); }
// right-first pre-order key of heap position pos (< 2^20 - 1): ancestors
// first, then the right subtree before the left one
TV16_FN uint32_t rf_key(uint32_t pos) {
    const uint32_t q = pos + 1, d = depth_of(q);
    const uint32_t path = q - (1u << d);
    const uint32_t inv = ~path & ((1u << d) - 1u);
    return ((inv << (19u - d)) << 5) | d;
}
TV16_FN bool is_desc(uint32_t q, uint32_t qt) {  // heap node q (pos + 1) below node qt
    const uint32_t dp = depth_of(q), dt = depth_of(qt);
    return dp > dt && (q >> (dp - dt)) == qt;
}
// the rankers' sort key: (sum desc = window offset asc, right-first pre-order
// of the start position asc)
TV16_FN uint64_t rank_key(uint32_t w, uint32_t cx) { return (uint64_t)w << 25 | rf_key(cx); }
TV16_FN uint32_t rank_key_offset(uint64_t g) { return (uint32_t)(g >> 25); }
// heap position c > 0: its parent and its sibling
TV16_FN uint32_t heap_parent(uint32_t c) { return (c - 1u) / 2u; }
TV16_FN uint32_t heap_sibling(uint32_t c) { return ((c - 1u) ^ 1u) + 1u; }
// start position cf is the parent or the sibling of the late line's ce (> 0)
TV16_FN bool parent_or_sibling(uint32_t cf, uint32_t ce) { return cf == heap_parent(ce) || cf == heap_sibling(ce); }
// a binned window entry of the one-bucket scan, {sum bits, chunk << 19 | line
// within the chunk << 10 | qualifying lines before it in the chunk}
struct WinEntry {
    uint32_t c, line, w, qb;  // chunk, line of the bucket, window offset, qualifying lines before it in its chunk
};
TV16_FN WinEntry win_entry(uint32_t sum_bits, uint32_t y, uint32_t tb, uint32_t lchunk) {
    WinEntry e;
    e.c = y >> 19;
    e.line = e.c * lchunk + ((y >> 10) & 511u);
    e.w = window_offset(tb, sum_bits);
    e.qb = y & 1023u;
    return e;
}
// its index in the candidate vector, qbefore qualifying lines before its chunk
TV16_FN uint32_t win_cand(const WinEntry &e, uint32_t qbefore) { return e.line - (qbefore + e.qb); }

}  // namespace tv16
}  // namespace stg
