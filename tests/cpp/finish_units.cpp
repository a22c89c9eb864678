// Host checks of stellatrain_amd/csrc/tv16_finish.h, the scalar rules the three
// thresholdv16 finishes share.  Plain C++: built by tests/test_finish_units.py
// with the address and undefined-behaviour sanitizers, nothing preloaded.
//
//   finish_units          the self-contained checks; prints "finish_units: ok"
//   finish_units regime   reads "n dst_len t_bits inc_bits" and n float bit
//                         patterns (hex) from stdin, decides the call as a
//                         finish does and prints the Regime (the Python side
//                         compares it with the oracle)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stellatrain_amd/csrc/tv16_finish.h"

using namespace stg;
using namespace stg::tv16;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

// ---- Decision round trip ----
static void check_decision() {
    const uint32_t ints[] = {0u, 1u, 0x80000000u, 0xffffffffu};
    const uint32_t tails[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x7f800000u, 0x7fc00000u, 0x7fa00000u};
    for (uint32_t cnt : ints) for (uint32_t M : ints) for (uint32_t Wtot : ints) for (uint32_t Qtot : ints)
        for (uint32_t tb : tails) for (uint32_t fl = 0; fl < 8; ++fl) {
            Regime R{};
            R.cnt = cnt;
            R.M = M;
            R.tail_key = bitsf(tb);
            R.regimeB = fl & 1u;
            R.listw = fl & 2u;
            R.tail_cand = fl & 4u;
            const uint32_t flags = decision_flags(R);
            CHECK(flags == ((fl & 1u) ? (TV16_DEC_B | ((fl & 2u) ? TV16_DEC_WIN : 0u) | ((fl & 4u) ? TV16_DEC_TAIL : 0u)) : 0u));
            const uint32_t tbits = 0x3f800000u ^ tb, nb = 0xfffffff0u, dst_len = 0xffffffffu, tag = decision_tag(0x00abcdefu);
            const DecisionWords w = decision_pack(R, Wtot, Qtot, bitsf(tbits), tag);
            const DecisionView v = decision_unpack(w.w[0], w.w[1], w.w[2], w.w[3], nb, dst_len);
            CHECK(v.tag == tag && v.tag == ((0x00abcdefu << 8) | TV16_TAG_DEC));
            CHECK(v.flags == flags && v.cnt == cnt && v.M == M && v.Wtot == Wtot && v.Qtot == Qtot);
            CHECK(v.tail_bits == tb && v.t_bits == tbits);  // bit patterns, signalling NaN included
            CHECK(v.tail == ((flags & TV16_DEC_TAIL) != 0));
            CHECK(v.N == nb - Qtot + (v.tail ? 1u : 0u) && v.rem == dst_len - cnt);
            CHECK(nan_tail(flags, tb) == (v.tail && (tb == 0x7fc00000u || tb == 0x7fa00000u)));
        }
}

// ---- window_lo ----
static void check_window() {
    CHECK(window_lo(0u) == 0u);
    CHECK(window_lo(TV16_WIN - 1u) == 0u);
    CHECK(window_lo(TV16_WIN) == 0u);
    CHECK(window_lo(TV16_WIN + 1u) == 1u);
    CHECK(window_lo(0x7f800000u) == 0x7f800000u - TV16_WIN);  // inf
    CHECK(window_lo(0x00800000u) == 0x00800000u - TV16_WIN);  // the smallest normal
    const uint32_t tb = fbits(1.0f);
    CHECK(tail_in_window(true, bitsf(tb - TV16_WIN), tb) && !tail_in_window(true, bitsf(tb - TV16_WIN - 1u), tb));
    CHECK(!tail_in_window(false, bitsf(tb - 1u), tb));
    CHECK(window_offset(tb, tb - 1u) == 0u && window_bin(window_offset(tb, tb - 257u)) == 1u);
    // the gate's tail conditions (the -0.0 key has no input that produces it: a sum starts from +0.f)
    Regime R{};
    R.regimeB = R.listw = R.tail_cand = true;
    R.N = 10;
    R.tail_key = bitsf(tb - 5u);
    CHECK(rankers_can_take(R, 4, true, 0, 1.0f, POS_LIM));
    CHECK(!rankers_can_take(R, 4, false, 0, 1.0f, POS_LIM) && !rankers_can_take(R, 4, true, 1, 1.0f, POS_LIM));
    CHECK(!rankers_can_take(R, 4, true, 0, 1.0f, 9));
    R.tail_key = 1.0f;  // at t
    CHECK(!rankers_can_take(R, 4, true, 0, 1.0f, POS_LIM));
    R.tail_key = bitsf(0x7fc00000u);
    CHECK(!rankers_can_take(R, 4, true, 0, 1.0f, POS_LIM));
    R.tail_key = -0.0f;
    CHECK(!rankers_can_take(R, 4, true, 0, bitsf(100u), POS_LIM));  // window [0, 100): -0.0 >= +0.0 is in it
    R.tail_key = bitsf(tb - TV16_WIN - 1u);  // below the window: not among the entries
    CHECK(rankers_can_take(R, 4, true, 0, 1.0f, POS_LIM) && !rankers_can_take(R, 0, true, 0, 1.0f, POS_LIM));
}

// ---- the pops against a walk over ranks ----
static void check_pops() {
    for (uint32_t rem = 1; rem <= 80; ++rem) for (uint32_t tl = 1; tl <= 15; ++tl) for (uint32_t Wk = 1; Wk <= 8; ++Wk)
        for (uint32_t t = 0; t <= Wk; ++t) {
            const uint32_t tr = t == Wk ? NO_RANK : t;
            // the walk: rank i starts where the lines before it end, the tail's line tl long
            uint32_t off[9], len[9], end = 0, P = Wk;
            bool found = false;
            for (uint32_t i = 0; i <= Wk; ++i) {
                off[i] = end;
                if (!found && end >= rem) { P = i; found = true; }  // the first P whose offsets cover rem
                const uint32_t l = i == tr ? tl : 16u;
                len[i] = end < rem ? (l < rem - end ? l : rem - end) : 0u;
                end += l;
            }
            const bool covered = off[Wk] >= rem;
            CHECK(pops_short(Wk, tr != NO_RANK, tl, rem) == !covered);
            const uint32_t N = Wk + 5u;
            const uint32_t Pc = umin(pops_count(rem, tl, tr), Wk), Ph = pops_bound(Pc, Wk);
            CHECK(Pc == P);
            CHECK(Ph == (P + 1u < Wk - 1u ? P + 1u : Wk - 1u));
            CHECK(pops_late(N, Ph) == (N > Ph + 1u ? N - (Ph + 1u) : 0u));
            if (covered) CHECK(pops_count(rem, tl, tr) == P);
            for (uint32_t i = 0; i < Wk; ++i) {
                CHECK(pop_offset(i, tr, tl) == off[i]);
                if (off[i] < rem) CHECK(pop_len(i, tr, tl, off[i], rem) == len[i]);
            }
            CHECK(pops_p0(rem) == (rem + 15u) / 16u);
        }
}

// ---- rf_key / is_desc against a right-first pre-order walk ----
static void preorder_rf(uint32_t pos, uint32_t n, std::vector<uint32_t> &out) {
    if (pos >= n) return;
    out.push_back(pos);
    preorder_rf(2 * pos + 2, n, out);
    preorder_rf(2 * pos + 1, n, out);
}
static void check_heap(uint32_t n) {
    std::vector<uint32_t> order;
    preorder_rf(0, n, order);
    CHECK(order.size() == n);
    for (uint32_t i = 0; i + 1 < n; ++i) CHECK(rf_key(order[i]) < rf_key(order[i + 1]));
    for (uint32_t a = 0; a < n; ++a)
        for (uint32_t b = 0; b < n; ++b) {
            bool below = false;  // a strictly below b: walk a's ancestors
            for (uint32_t x = a; x;) {
                x = (x - 1) / 2;
                if (x == b) below = true;
            }
            CHECK(is_desc(a + 1, b + 1) == below);
            if (a) CHECK(parent_or_sibling(b, a) == (b == (a - 1) / 2 || (b != a && b && (b - 1) / 2 == (a - 1) / 2) ||
                                                     (b == ((a - 1) ^ 1u) + 1)));
        }
    for (uint32_t a = 1; a < n; ++a) {
        CHECK(heap_parent(a) == (a - 1) / 2);
        CHECK(heap_sibling(a) != a && heap_parent(heap_sibling(a)) == heap_parent(a));
    }
    CHECK(rank_key_offset(rank_key(12345u, 7u)) == 12345u && (uint32_t)(rank_key(12345u, 7u) & 0x1ffffffu) == rf_key(7u));
    const WinEntry e = win_entry(fbits(1.0f) - 300u, (5u << 19) | (17u << 10) | 3u, fbits(1.0f), 512u);
    CHECK(e.c == 5u && e.line == 5u * 512u + 17u && e.w == 299u && e.qb == 3u && win_cand(e, 40u) == e.line - 43u);
}

// ---- one call, decided as a finish decides it ----
static float line_sum(const float *p) {  // the reference's tree over |x| (thresholdv16.cpp:57-73)
    float a[16];
    for (int i = 0; i < 16; ++i) a[i] = std::fabs(p[i]);
    const float lo = ((a[0] + a[4]) + (a[1] + a[5])) + ((a[2] + a[6]) + (a[3] + a[7]));
    const float hi = ((a[8] + a[12]) + (a[9] + a[13])) + ((a[10] + a[14]) + (a[11] + a[15]));
    return lo + hi;
}
static int regime_main() {
    unsigned n, dst_len, tbits, ibits;
    if (std::scanf("%u %u %x %x", &n, &dst_len, &tbits, &ibits) != 4) return 2;
    std::vector<float> src(n);
    for (unsigned i = 0; i < n; ++i) {
        unsigned b;
        if (std::scanf("%x", &b) != 1) return 2;
        src[i] = bitsf(b);
    }
    const float t = bitsf(tbits), inc = bitsf(ibits);
    const uint32_t nb = n / 16, tl = n % 16, tb = fbits(t), wlo = window_lo(tb);
    uint32_t Qtot = 0, Wtot = 0;
    for (uint32_t l = 0; l < nb; ++l) {
        const float s = line_sum(&src[(size_t)l * 16]);
        const uint32_t u = fbits(s);
        if (s >= t) ++Qtot;
        else if (u >= wlo && u < tb) ++Wtot;
    }
    Regime R;
    regime_head(R, dst_len, Qtot);
    regime_no_tail(R);
    if (regime_sums_tail(R, dst_len, tl)) {
        float sm = 0.f;
        for (uint32_t i = 0; i < tl; ++i) sm += src[(size_t)nb * 16 + i];
        regime_tail(R, sm, t, tl, dst_len);
    }
    CHECK(regime_short(R, dst_len) == (R.c0 + R.ct < dst_len));
    regime_close(R, dst_len, nb, Qtot, Wtot);
    CHECK(R.regimeB == regime_short(R, dst_len));
    std::printf("Qtot=%u Wtot=%u kb=%u r=%u lim=%u c0=%u ct=%u cnt=%u M=%u N=%u regimeB=%d tail_cand=%d listw=%d "
                "tail_key=%08x tail_in=%d next_t=%08x count=%u\n",
                Qtot, Wtot, R.kb, R.r, R.lim, R.c0, R.ct, R.cnt, R.M, R.N, (int)R.regimeB, (int)R.tail_cand, (int)R.listw,
                fbits(R.tail_key), (int)tail_in_window(R.tail_cand, R.tail_key, tb),
                fbits(next_threshold(t, inc, R.regimeB)), emitted_count(dst_len, nb, tl));
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !std::strcmp(argv[1], "regime")) return regime_main();
    check_decision();
    check_window();
    check_pops();
    check_heap(63);
    check_heap(100);
    std::printf("finish_units: ok\n");
    return 0;
}
