// ws.h -- per-stream workspace layout shared by host launchers and kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "common.h"
#include "tv16_const.h"  // CAND_CAP, TV16_WIN, the Decision flags and tag

namespace stg {

constexpr uint32_t CAND_WORDS = 4 * CAND_CAP; // per bucket: line-sum bits | line position | candidate index | spare
constexpr uint32_t TV16_SCAN_LDS = 35584;     // LDS bytes of a scan workgroup (bound; tv16.hip checks)

constexpr uint32_t TV_TILE = 8192;           // top-k elements per tile (32 KiB)
constexpr uint32_t TOPK_SUP_CAP = 1024;      // top-k superset entries kept per tile
constexpr uint32_t TOPK_LIST_CAP = 4096;     // top-k: keys of T's level-2 bin listed for the final select
constexpr uint32_t TOPK_LIST_TILES = 8192;   // ... when the bucket has at most this many tiles (64 Mi floats)
constexpr uint32_t TV_MAXG = 2048;           // threshold-v ranges (workgroups) per call
constexpr uint32_t TV_SCAP = 4096;           // threshold-v qualifiers listed per range (32 KiB of LDS)

constexpr uint32_t RS_BINS = 2048;           // radix-select bins (11 bits)
constexpr uint32_t RS_SHARDS = 8;            // histogram copies: workgroup w adds into shard w % RS_SHARDS
constexpr uint32_t RS_SH_HIST = 4;           // ... of which rs_hist's one workgroup per CU uses the first 4

// thresholdv16 in-launch control block (one launch = a batch of <= MAX_BATCH
// buckets cut into fixed 2048-line chunks).  The per-call chunk counter comes
// in two copies selected by the call epoch's parity; every launch zeroes the
// other copy for the next call (the next call on this workspace is
// stream-ordered after this launch).  Words handed between workgroups carry
// the call tag (epoch << 8 | kind) so stale words of earlier calls never match.
constexpr uint32_t MAX_BATCH = 32;
constexpr uint32_t TV16_CHUNK = 2048;        // lines (16 floats) per chunk = 128 KiB
struct CallCtl {
    uint32_t next;      // dynamic chunk counter
    uint32_t pad[31];
    uint32_t crew_ticket[32];  // the crew's ticket (its own line: taken by every crew workgroup)
    uint32_t crew_done[32];    // the crew's completed units per phase (polled)
};
// Per-bucket regime decision, written by the finisher of the bucket's last
// chunk: [1..3] first, drained, then [0] = {tag:32 | flags:32}; read by the
// follow-on fill launch.
struct alignas(32) Decision {
    uint64_t w[4];      // packed and unpacked by tv16_finish.h (decision_pack, decision_unpack)
};
constexpr uint32_t POISON_COUNT = 0xffffffffu;  // *count_out of a launch that hit a device failure
struct FillCtl {
    CallCtl cc[2];                     // [epoch parity]
    Decision dec[MAX_BATCH];
};
// Per-chunk descriptor (16 B): {tag:32 | qualifying lines:16 | window lines:16}
// by the chunk's last streaming wave.
struct alignas(16) ChunkDesc {
    uint64_t agg;
    uint64_t pad;
};

// Per-call scalars handed from the scan kernel to the fill kernel.
struct CallParams {
    float t;
    float inc;
    uint32_t pad[2];
};

// Radix-select state (first thresholds, top-k).
struct RSel {
    uint32_t prefix;    // bits fixed so far
    uint32_t mask;      // which bits are fixed
    uint32_t rank;      // remaining rank (0-based, descending) inside the prefix
    uint32_t cnt_gt;    // keys strictly above the prefix range
    uint32_t done;      // classes of workgroups done with the current pass (the last one picks)
    uint32_t pad[3];    // pad[0]: top-k's superset floor; [1]: keys in the last picked bin; [2]: top-k list length
    uint32_t done64[64];  // workgroups done, per class blockIdx.x % 64
    // The level histogram in RS_SHARDS copies, summed by the pick: device-scope
    // atomics on one word serialise at the memory side (~90 per us), so a
    // 2048-workgroup pass adding into one copy spent ~15 us on its hot bins
    // (into 8 copies: 256 adds per word, spread over the pass).
    uint32_t hist[RS_SHARDS][RS_BINS];
};

// thresholdv16 one-bucket path: a scan launch with no waits between
// workgroups (tv16_lscan, tv16lone.hip) lists, per chunk, its qualifying and
// window lines; the fill launch (tv16fill.hip, lfin mode) finishes the call.
constexpr uint32_t LCHUNK = 512;  // lines (16 floats) per chunk = 32 KiB: one per 256-thread workgroup
constexpr uint32_t LQCAP = 64;    // qualifying lines listed per chunk (~5 at k = 1 %; more: the finish re-reads it)
constexpr uint32_t LWCAP = 32;    // window lines listed per chunk (~2; more: likewise)
constexpr uint32_t LMAXC = 4096;  // chunks of a bucket the one-bucket path takes (128 MiB)
// ... and its window entries binned by the scan: bin b = (bits(t) - 1 - bits(sum)) >> 8
// (256 ulps, 1024 bins over the window), LBCAP entries per bin {sum bits,
// chunk << 19 | line within the chunk << 10 | qualifying lines before it};
// the counts are zeroed by the finish's last workgroup after use
constexpr uint32_t LNBIN = 1024;
constexpr uint32_t LBCAP = 32;
// bin b's count word: bins interleaved over 32 lines (b mod 32 picks the
// line), so the bins the window fills near t sit on as many 128-byte lines
// (the scan's returning atomics on one line queue behind each other)
__host__ __device__ constexpr uint32_t whist_word(uint32_t b) { return (b & 31u) * 32u + (b >> 5); }
static_assert(LNBIN == 1024, "32 lines x 32 words");

// thresholdv16 regime-B crew (tv16wide.h): per bucket slot of a launch, the
// level-1 histogram of the candidates' keys and the hand-offs between phases
constexpr uint32_t CREW_BINS = 8192;
struct CrewCtl {
    uint32_t hist[CREW_BINS];  // zeroed by the bucket's phase Z
    // The hand-off words on a 128-byte line of their own.  Packed behind hist
    // (32 bytes), they shared a line with the next slot's hist[0 .. 23]: with
    // two buckets in the crew, phase C of bucket j + 1 loads that line (an sc1
    // load into LDS, not into registers) while phase D of bucket j has yet to
    // store P, tail_rank and op, and an emission unit of bucket j on that XCD
    // could then read the previous call's P and skip its share.
    uint32_t beta, nL, status, P, tail_rank, op, pad[26];
};
static_assert(sizeof(CrewCtl) % 128 == 0 && offsetof(CrewCtl, beta) % 128 == 0, "hand-off words on their own line");

// top-k steered by the key's last k-th magnitude (topk1.hip): per-call control
// block, two copies by call tag parity (each call zeroes the next call's), and
// the band histogram (one bin per ulp, two copies by parity)
constexpr uint32_t TK1_NPH = 9;     // phases of the select's way
constexpr uint32_t TK1_SH = 8;      // ticket / completion shards (tile % 8); superset regions
constexpr uint32_t TK1_LINE = 32;   // words per 128-byte line: every shard counter on a line of its own
constexpr uint32_t TK2_FINE = 1u << 18;               // band bins: one per ulp
constexpr uint32_t TK2_CSH = 8;                       // coarse bins: 256 ulps
constexpr uint32_t TK2_COARSE = TK2_FINE >> TK2_CSH;  // 1024
constexpr uint32_t kTk2Cshards = 1;  // 4 and 8 copies measured slower (profiles/r05_topk_finish_ab.jsonl)
constexpr uint32_t TK2_CSHARDS = kTk2Cshards;     // copies of the coarse bins (each tile adds into one)
constexpr uint32_t TK2_HI = 16;                       // shards of the count of keys above the band
constexpr uint32_t TK2_REG = 32;                      // superset regions (tile mod 32), an offset counter each
constexpr uint32_t kTk2Ut = 16;
constexpr uint32_t TK2_UT = kTk2Ut;               // tiles per emission unit (at most)
constexpr uint32_t TK2_UNITS = TOPK_LIST_TILES / TK2_UT;
struct alignas(128) TopkCtl {
    // the stream launch's band [F, H): the next call's stream launch zeroes
    // the fine bins [0, H - F) it touched and every line after this one
    uint32_t band_F, band_H, band_ok;
    uint32_t bpad[TK1_LINE - 3];
    uint32_t tk[TK1_NPH][TK1_SH][TK1_LINE];    // tickets per phase and shard
    uint32_t done[TK1_NPH][TK1_SH][TK1_LINE];  // units done per phase and shard
    uint32_t sdone[TK1_NPH][TK1_LINE];         // shards done per phase
    uint32_t flag[TK1_NPH];                    // = the call tag once single-unit phase p is done
    uint32_t ovf, res_T;                       // a superset region overflowed; the select's T
    uint32_t pad[TK1_LINE - TK1_NPH - 2];
    uint32_t utk[TK1_LINE];                    // emission units taken
    uint32_t hi[TK2_HI][TK1_LINE];             // keys >= H, by tile % TK2_HI
    uint32_t shn[TK2_REG][TK1_LINE];           // superset entries placed in region tile % TK2_REG
    uint32_t coarse[TK2_CSHARDS][TK2_COARSE];  // band keys per 256 ulps, by tile % TK2_CSHARDS
    uint64_t udesc[TK2_UNITS];                 // emission unit u: bit 63 | > T count << 32 | == T count
};

struct DevWS {
    FillCtl *ctl;
    TopkCtl *tkctl;      // [2]
    uint32_t *tkfine;    // [2][TK2_FINE] band histograms by call parity, zero between calls
    CrewCtl *crew;       // MAX_BATCH slots
    ChunkDesc *desc;     // thresholdv16 chunk descriptors (grown per launch, zeroed)
    CallParams *cp;
    RSel *rsel;
    uint32_t *fail;      // sticky failure bits
    uint32_t *cand;      // regime-B window entries, CAND_WORDS per bucket of a launch
    uint32_t *misc;      // small scratch (counts)
    uint64_t *tv_ticket;   // threshold-v: ranges taken, monotonic over the workspace's life
    float *sums;         // thresholdv16: one sum per 16-float line
    uint32_t *tile_cnt;  // per-tile qualifier counts
    uint32_t *tile_aux;  // per-tile secondary counts (threshold-v max, top-k ties)
    uint32_t *stage_pos; // threshold-v staged positions
    float *stage_val;    // threshold-v staged values
    uint2 *ldesc;        // one-bucket path: per chunk {qualifying lines, window lines}
    uint32_t *lq;        // ... the chunk's qualifying lines in order (LQCAP per chunk, line within the chunk)
    uint2 *lw;           // ... its window lines in order: {sum bits, line within the chunk | qualifying before << 16}
    float4 *lv;          // ... the qualifying lines' data (LQCAP x 4 float4 per chunk)
    uint32_t *whist;     // ... window entries per bin (2 x LNBIN by call parity, zero between calls)
    uint32_t *larr;      // ... the scan's finish: per role the tag of the last call it finished
    uint2 *went;         // ... the entries by bin (LNBIN x LBCAP)
};

// ---- launchers (implemented in the .hip files) ----
constexpr uint32_t GATHER_MAX = 16;  // local GPUs per node the gather-add accepts
struct GatherArgs {
    float *dst;                    // grad[0]
    const float *resid;            // residual (or null: no residual term)
    const void *src[GATHER_MAX];   // src[1 .. nsrc-1] = grad[1 .. N-1].  src[0]: the typed launchers' first term
                                   // when not null (dst is then write-only); the fp32 launchers ignore it
    uint32_t nsrc;                 // N, the node's GPU count
    uint32_t dtypes;               // typed launchers: src[s]'s STG_DT_* type in bits 2 s, 2 s + 1 (one scalar
                                   // word, as PublishTask::dtypes); the fp32 launchers read every source as float
};
// How a typed gather-add runs over n elements: `head` scalar elements, then
// lane groups of `width` elements (8: one 16-byte load per 16-bit stream and
// two per fp32 stream; 4: 8 and 16 bytes), then a scalar tail < width.  A
// stream is dst, the residual or a source, taken at the first element of the
// range: addr[i] its byte address there, esz[i] its element size (4 or 2).
// The 8-wide group runs when one head < 8 brings every fp32 stream to 16 bytes
// and every 16-bit stream to 16 bytes; else the 4-wide one when one head < 4
// brings them to 16 and 8 bytes; else width 0, every element scalar (head 0).
// head <= n always (a range shorter than its head is all head).
struct GatherPlan {
    uint32_t width, head;
};
inline GatherPlan gather_plan(const uintptr_t *addr, const uint32_t *esz, uint32_t ns, uint64_t n, uint32_t max_width = 8) {
    for (uint32_t w = 8; w >= 4; w >>= 1) {
        if (w > max_width) continue;
        for (uint32_t h = 0; h < w; ++h) {
            bool ok = true;
            for (uint32_t i = 0; i < ns && ok; ++i)
                ok = ((addr[i] + (uintptr_t)esz[i] * h) & (esz[i] == 4 ? 15u : 2u * w - 1u)) == 0;
            if (ok) return GatherPlan{w, (uint32_t)(h < n ? h : n)};
        }
    }
    return GatherPlan{0, 0};
}
// the plan of a's streams over [start, end), as launch_gather_add_typed takes it
GatherPlan gather_plan_of(const GatherArgs &a, size_t start, size_t end);
struct Tv16Bucket {
    const float *src;
    size_t n;
    uint32_t k;
    uint32_t dst_len;
    uint32_t *idx;
    float *val;
    int32_t idx_offset;
    uint32_t *count_out;
    KeyState *state;
    bool first;        // no AIMD state yet: compute the first threshold
    float *sums;       // per-bucket scratch: first-threshold line sums; the fill's candidate heap
                       // (2 words per line: (nb + 1) * 2 floats)
    float *resid;      // MERGE error feedback: receives the bucket's full lines, or null
    const GatherArgs *gather;  // intra-node gather-add fused into the scan (dst = src), or null
    uint32_t wflag;    // the emission writes the wire form (STG_WIRE_* flags; idx / val typed by it)
};
struct Tv16Launch {
    const Tv16Bucket *b;
    uint32_t nb;       // buckets in this launch (<= MAX_BATCH)
    int num_cu;
    hipEvent_t *ev;    // optional [before, mid, after] the codec launch(es)
    uint32_t epoch;    // per-workspace call counter, 1..2^24-1 (hand-off tags)
    uint32_t max_wg;     // fused-kernel workgroups at most (its share of 2 per CU)
    uint32_t desc_cap;   // ChunkDesc entries at ws.desc
    uint32_t lone_cap;   // chunks the one-bucket lists (ws.ldesc / lq / lw) hold (0: none)
    uint32_t *lone_calls;  // the workspace's one-bucket path calls (host; its parity picks the
                           // window histogram and arrival block, each call zeroing the other copy)
};
hipError_t launch_tv16(const Tv16Launch &a, const DevWS &ws, hipStream_t s);
bool tv16_debug_count();  // STG_DEBUG_TV16_COUNT, as the launcher read it (tv16.hip)
// thresholdv16 regime-B heap fill (tv16fill.hip): one workgroup per bucket
struct Tv16FillBucket {
    const float *src;
    uint32_t *idx;
    float *val;
    uint32_t *count_out;
    uint32_t nb, tl, dst_len;
    int32_t idx_offset;
    const uint32_t *cand;  // the bucket's window entries (CAND_WORDS)
    uint2 *heap;           // full-path scratch: (nb + 1) candidates {key bits, element position}
    uint32_t wflag, wend;  // wire form of the emitted pairs (wire_dev.h; 0: u32 / f32)
};
struct Tv16FillArgs {
    Tv16FillBucket bk[MAX_BATCH];
    uint32_t nbk;
    uint32_t epoch;
    const Decision *dec;
    uint32_t *fail;
    uint32_t *dbg;         // diagnostics: phase stamps of workgroup 0 (ws.misc)
    uint32_t mode;         // tests (STG_DEBUG_TV16_FILL): 1 = always the shadow heap, 2 = always the literal heap,
                           // 3 = always the leader over the window, 4 = always the crew
    uint32_t crew;         // extra workgroups that order window-miss buckets (tv16wide.h; 0: none)
    CrewCtl *crew_ctl;     // MAX_BATCH slots
    bool lone;             // a one-bucket launch: the fill variant that takes the CU's registers
    uint32_t helpers;      // lone: extra workgroups that emit shares of the order (0: none)
    CallCtl *cc;           // this call's counters: [pad 0] fill tickets, [1] order ready, [2] pops, [3] tail rank,
                           // [4] lfin workers done
    // lfin: the launch also finishes a one-bucket scan (tv16_lscan): `workers`
    // workgroups emit the qualifying lines, list the window and decide; the
    // last of them to finish orders the regime-B fill; `helpers` more emit it
    bool lfin;
    uint32_t workers;
    uint32_t nc;           // chunks of the bucket
    const uint2 *ldesc;
    const uint32_t *lq;
    const uint2 *lw;
    const float4 *lv;
    uint32_t *whist;       // the scan's binned window (this call's copy; the scan zeroes the next call's)
    const uint2 *went;
    uint32_t rankers;      // workgroups that order the regime-B fill in parallel (0: the orderer alone)
    KeyState *state;
    const CallParams *cp;  // {t, inc} as the scan read them
    float *resid;          // fused error feedback: the ragged tail is copied by the finish
    // the scan launch finished the call (tv16lf2.h): every role of this launch
    // leaves when fin_done[0 .. fin) all hold fin_tag (fin == 0: never)
    const uint32_t *fin_done;
    uint32_t fin, fin_tag;
};
hipError_t launch_tv16_fill(const Tv16FillArgs &a, hipStream_t s);
// the same fill built to write the wire form of buckets with wflag set (tv16fill.hip)
hipError_t launch_tv16_fill_wire(const Tv16FillArgs &a, hipStream_t s);
inline hipError_t launch_tv16_fill_any(const Tv16FillArgs &a, hipStream_t s) {
    bool w = false;
    for (uint32_t i = 0; i < a.nbk; ++i) w |= a.bk[i].wflag != 0;
    return w ? launch_tv16_fill_wire(a, s) : launch_tv16_fill(a, s);
}
// one-bucket scan (tv16lone.hip): every workgroup streams its chunks and lists
// them; nothing waits on another workgroup
constexpr uint32_t LF2_MAXF = 64;                     // finish roles of a one-bucket scan at most (tv16lf2.h)
constexpr uint32_t LARR_WORDS = LF2_MAXF;             // per role: the call tag once its part is written
struct LScanArgs {
    const float *src;
    uint32_t nb;           // full lines
    uint32_t nc;           // chunks
    KeyState *state;
    CallParams *cp;        // receives {t, inc} as read
    float *resid;          // fused error feedback (or null)
    uint2 *ldesc;
    uint32_t *lq;
    uint2 *lw;
    float4 *lv;
    uint32_t *whist;       // window entries per bin (zero at the start of the call)
    uint2 *went;           // ... and the entries, LBCAP per bin
    uint32_t *zero_next;   // the next call's counter block (CallCtl), zeroed here
    // the gather-add fused into the stream (gather.hip's sum, in its order):
    // src += gres + gsrc[1] + ... + gsrc[gn - 1], stored back to src once
    const float *gres;     // residual term (null: none)
    const float *gsrc[GATHER_MAX];
    uint32_t gn;           // 0: no gather; else N (gsrc[0] unused)
    uint32_t tl;           // the ragged tail's floats (summed by workgroup 0 under the gather)
    // the finish inside the scan launch (tv16lf2.h): `fin` roles (0: none, the
    // fill launch finishes), `nwk` of them workers; arrival block of this call
    // and of the next (zeroed here), and the next call's window histogram
    uint32_t fin, nwk, mode;
    uint32_t tag;          // the call's tag (>= 1) on every chunk's counts
    uint32_t skip;         // diagnostics (STG_LF2_SKIP): a role stops at that point (5: the lists carry a wrong tag)
    uint32_t *done;        // per role: the tag once its part is written (LARR_WORDS)
    uint32_t *whist_next;
    uint32_t *out_idx;
    float *out_val;
    uint32_t *count_out;
    uint32_t dst_len;
    int32_t idx_offset;
    uint32_t *fail, *dbg;
};
hipError_t launch_tv16_lscan(LScanArgs &a, int num_cu, hipStream_t s);

struct TvLaunch {
    const float *src;
    size_t n;
    uint32_t k;
    uint32_t cap;
    uint32_t *idx;
    float *val;
    uint32_t *count_out;
    KeyState *state;
    bool first;
    int num_cu;
    hipEvent_t *ev;
    uint32_t tag;          // call tag (>= 1) of the range descriptors at ws.tile_cnt (2 words per range)
    uint64_t ticket_base;  // ws.tv_ticket's value when this call starts
    uint32_t *grid_out;    // receives the launch's range count (the ticket advances by it)
};
hipError_t launch_tv(const TvLaunch &a, const DevWS &ws, hipStream_t s);

struct TopkLaunch {
    const float *src;
    size_t n;
    uint32_t k;
    uint32_t cap;
    uint32_t *idx;
    float *val;
    int32_t idx_offset;
    bool bug_compat;
    uint32_t *count_out;
    int num_cu;
    hipEvent_t *ev;
};
hipError_t launch_topk(const TopkLaunch &a, const DevWS &ws, hipStream_t s);
// top-k steered by the key's last k-th magnitude (topk1.hip), buckets of at
// most TOPK_LIST_TILES tiles: a key's first call (!hinted) runs launch_topk and
// seeds the hint; later calls stream once and emit (the select's way inside
// the emission launch when the band misses)
hipError_t launch_topk1(const TopkLaunch &a, const DevWS &ws, KeyState *state, bool hinted, uint32_t *tag,
                        hipStream_t s);

// Radix select: the key of descending rank `rank` among (bits(a[i]) & 0x7fffffff),
// i < m, with the last element's bits additionally masked by `last_mask`, plus
// `extra_zeros` implicit zero keys.  Result in ws.rsel (prefix = key bits,
// cnt_gt = keys strictly greater, rank = rank among equal keys).
hipError_t launch_radix_select(const float *a, size_t m, uint32_t last_mask, uint64_t extra_zeros, uint32_t rank,
                               const DevWS &ws, int num_cu, hipStream_t s);
hipError_t launch_radix_level1(const float *a, size_t m, uint32_t last_mask, uint64_t extra_zeros, uint32_t rank,
                               const DevWS &ws, int num_cu, hipStream_t s);

hipError_t launch_synth(float *dst, size_t n, uint64_t seed, int dist, uint32_t param, hipStream_t s);

// world == 1 in one launch after the winner election: tagged per-tile counts
// and a ticket counter of the (device, stream) scratch.  Every merge passes
// one; desc, ticket, dup and fail are always set (world > 1 reads none of them).
struct Win1Desc {
    uint64_t *desc;       // per tile {tag:32 | winners:32}, zero at creation
    uint64_t *ticket;     // tile counter, zeroed by each call's win_mark
    uint32_t tag;         // call tag >= 1
    uint32_t *fail;       // sticky failure word of the scratch (a look-back that gave up)
    uint32_t *dup;        // set when an index repeats; the ticket then counts from 0 (win_mark zeroes it)
    const struct SgdLaunch *sgd = nullptr;    // the SGD step fused into the emission (null: none)
    const struct AdamLaunch *adam = nullptr;  // ... or the Adam step (no amsgrad)
};
constexpr uint32_t MERGE_TILE = STG_WG * 16;  // pairs / marks per scatter-merge tile
// `launches` of the MERGE and step launchers below: where given, the kernel
// launches enqueued are added to it as they are enqueued (the batched entries'
// counter, stg_merge_batch_launches).
inline void count_launch(uint64_t *launches, uint32_t k = 1) {
    if (launches) *launches += k;
}
// MERGE decompress of `world` rank streams of per_rank pairs each, every one
// read where it landed, in the form its flag says it arrived in (STG_WIRE_*
// bits; wire_dev.h).  Flag 0 is the decoded form (u32 / f32) and takes the
// decoded kernels.
struct RankStream {
    const void *idx, *val;
    uint32_t flag;
};
hipError_t launch_scatter_merge(const RankStream *ranks, size_t per_rank, int world, size_t n, float *dense,
                                uint8_t *mark, uint32_t *out_idx, float *out_val, uint32_t *out_count,
                                uint32_t *scratch_tiles, uint32_t *win, int num_cu, hipStream_t s,
                                const Win1Desc &w1, uint64_t *launches = nullptr);

struct SgdLaunch {
    float *param;
    uint32_t param_len;
    const float *grad;
    const uint32_t *gidx;
    uint32_t grad_len;
    const uint32_t *d_grad_len;
    float *mom;      // momentum buffer (param_len floats) or null when momentum == 0
    bool first;
    float momentum, dampening, weight_decay;
    double lr;
    bool nesterov;
    // smart momentum (sgd.cpp:225-227, 258-259): the factor is
    // pow(momentum, iter - last[id]) in place of momentum
    uint32_t *last;        // per name: the iteration that last touched each index (param_len words); null: option off
    uint32_t iter;         // the optimizer's call count before this call (shared by all names)
    const float *pow_tab;  // pow_tab[d] = (float)pow((double)momentum, (double)d), filled by the host's libm
    uint32_t pow_len;      // its entries; the last one is 0.f and so is every factor past it
    uint32_t *fail;        // sticky failure word of the optimizer handle (SGD_FAIL_FACTOR)
};
constexpr uint32_t SGD_FAIL_FACTOR = 1u;  // a factor outside [0, 1): an index repeated within one call
hipError_t launch_sgd(const SgdLaunch &a, hipStream_t s, uint64_t *launches = nullptr);

struct AdamLaunch {
    float *param;
    uint32_t param_len;
    const float *grad;
    const uint32_t *gidx;
    uint32_t grad_len;          // capacity of grad/gidx (grid size)
    const uint32_t *d_grad_len; // device count (min'd with grad_len) or null
    float *m, *v;               // per-name moment arrays (param_len floats each)
    float *vmax;                // per-name running max (one float on the device)
    uint32_t *tiles;            // amsgrad look-back words: one uint64 per ADAM_TILE tile (zeroed at allocation)
    uint32_t tag;               // amsgrad word tag: the name's tick of this call (>= 1)
    uint32_t *fail;             // sticky device failure word of the optimizer handle
    float b1, b2, eps, weight_decay;
    double lr, c1, c2;          // c = 1 - pow(b, tick), computed on the host (adam.cpp:42-43,67-68)
    bool amsgrad, maximize;
};
constexpr uint32_t ADAM_TILE = STG_WG * 4;  // amsgrad: elements per workgroup tile
hipError_t launch_adam(const AdamLaunch &a, hipStream_t s, uint64_t *launches = nullptr);

// Batched world-1 MERGE decompress + fused optimizer step (merge_batch.hip):
// one election launch and one emission launch for up to MERGE_BATCH tensors.
// The table travels by value in the kernel arguments (under 2 KiB of the
// 4 KiB they may take), so the group is 16 like WireBatch's, not 32.
constexpr uint32_t MERGE_BATCH = 16;       // tensors per launch pair
constexpr uint32_t MERGE_BATCH_WP = 4;     // pairs per lane, as the per-tensor emission
constexpr uint32_t MERGE_BATCH_TILE = MERGE_BATCH_WP * STG_WG;  // pairs per workgroup of either launch
// winner words (the sum of the tensors' n) one launch may ask of the scratch:
// 32 MiB.  A launch closes before the sum would pass it; a tensor larger than
// the cap runs in a launch of its own, on the words a per-tensor call would take.
constexpr size_t MERGE_BATCH_WIN_CAP = size_t(1) << 23;
// A tensor slot's hand-off words, each on a 128-byte line of its own.
struct alignas(128) MergeSlotCtl {
    uint64_t ticket;     // tiles taken in the ticketed path (zeroed by the election launch)
    uint32_t pad0[30];
    uint32_t dup;        // set by the election when an index repeats or is >= n; cleared by the last tile
    uint32_t pad1[31];
    uint32_t fail_tag;   // the tag of the last launch in which a look-back of this slot gave up
    uint32_t pad2[31];
};
struct MergeTensor {
    const void *idx, *val;  // the rank stream where it landed, typed by `flag` (0: u32 / f32)
    uint32_t *out_idx;
    float *out_val;
    uint32_t *out_count;
    float *param;
    float *s0;              // SGD: the momentum buffer (null: momentum 0); Adam: m
    void *s1;               // SGD smart momentum: the last-touched words; Adam: v
    union {
        struct { double c1, c2; } adam;          // the name's bias corrections at its tick
        struct { uint32_t iter, first; } sgd;    // the task's iteration; the name's first call
    } u;
    uint32_t m, n;          // pairs; parameter length
    uint32_t flag;
    uint32_t blk0;          // first workgroup of this tensor in either launch (as WireBucket::blk0)
    uint32_t win0, desc0;   // its slices of the scratch: winner words, tagged tile counts
};
struct MergeBatchArgs {
    MergeTensor t[MERGE_BATCH];
    uint32_t nt;
    uint32_t tag;           // the launch pair's tag >= 1 on every tile count
    uint32_t *win;
    uint64_t *desc;
    MergeSlotCtl *ctl;      // MERGE_BATCH slots
    uint32_t *fail;         // the scratch's sticky failure word
    SgdLaunch sgd;          // the handle-wide scalars (per-tensor fields unset), opt 0 / 1
    AdamLaunch adam;        // ... opt 2
};
static_assert(sizeof(MergeBatchArgs) <= 2048, "kernel arguments: stay well under 4 KiB");
// opt: 0 = SGD, 1 = SGD with smart momentum, 2 = Adam (no amsgrad); blocks =
// the sum of the tensors' tiles
hipError_t launch_merge_batch(const MergeBatchArgs &w, uint32_t blocks, int opt, hipStream_t s,
                              uint64_t *launches = nullptr);

// Batched world > 1 MERGE decompress + fused optimizer step
// (merge_batch_world.hip): up to MERGE_BATCH tensors of one world share
// world + 1 scatter launches, the mark count, its scan and the emission.  A
// tensor works on its own slices of the (device, stream) scratch, which start
// at `off` elements (a multiple of 16, so every slice is 16-byte aligned):
// dense floats and mark bytes at off, its 2 n winner words at 2 off.  The sum
// of a group's n stays at MERGE_BATCH_WIN_CAP / 2, so the winner words keep
// the 32 MiB bound above (16 MiB of dense, 4 MiB of marks).
constexpr uint32_t MERGE_WORLD_ALIGN = 16;  // elements between slice starts: a multiple of this
struct MergeScatterTensor {
    const void *sidx, *sval;  // the rank this launch scatters (null: none, the first launch)
    const void *midx;         // the rank it elects (null: none, the last launch)
    uint32_t sflag, mflag;
    uint32_t m, n;            // pairs per rank; parameter length
    uint32_t blk0;            // first workgroup of this tensor (STG_WG threads over 2 m)
    uint32_t off;
};
struct MergeScatterArgs {
    MergeScatterTensor t[MERGE_BATCH];
    uint32_t nt;
    uint32_t rank;            // the launch: scatters rank - 1, elects rank
    uint32_t *win;
    float *dense;
    uint8_t *mark;
};
struct MergeWorldTensor {
    uint32_t *out_idx;
    float *out_val;
    uint32_t *out_count;
    float *param;
    float *s0;                // as MergeTensor's
    void *s1;
    union {
        struct { double c1, c2; } adam;
        struct { uint32_t iter, first; } sgd;
    } u;
    uint32_t n;               // parameter length
    uint32_t blk0;            // first workgroup (= MERGE_TILE tile) in the count and the emission;
                              // its 2 * tiles tile words start at 2 * blk0
    uint32_t off;
    uint32_t pad;
};
struct MergeWorldArgs {
    MergeWorldTensor t[MERGE_BATCH];
    uint32_t nt;
    float world;
    uint32_t *tiles;
    float *dense;
    uint8_t *mark;
    SgdLaunch sgd;            // the handle-wide scalars (per-tensor fields unset), opt 0 / 1
    AdamLaunch adam;          // ... opt 2
};
static_assert(sizeof(MergeScatterArgs) <= 2048 && sizeof(MergeWorldArgs) <= 2048,
              "kernel arguments: stay well under 4 KiB");
// launch `w.rank` of a group's world + 1 (blocks = the sum over its tensors of ceil(2 m / STG_WG))
hipError_t launch_merge_world_scatter(const MergeScatterArgs &w, uint32_t blocks, hipStream_t s,
                                      uint64_t *launches = nullptr);
// the mark count, its scan and the emission with the step (opt as above; blocks = the sum of the tensors' tiles)
hipError_t launch_merge_world_emit(const MergeWorldArgs &w, uint32_t blocks, int opt, hipStream_t s,
                                   uint64_t *launches = nullptr);
hipError_t launch_gather_add(const GatherArgs &a, size_t start, size_t end, int num_cu, hipStream_t s);
// ... with 16-bit sources and / or a first term read from src[0] (gather.hip)
hipError_t launch_gather_add_typed(const GatherArgs &a, size_t start, size_t end, int num_cu, hipStream_t s);
uint32_t gather_max_width();  // 8; STG_DEBUG_GATHER_WIDTH=4 keeps the typed launchers to 4-wide groups (measurements)
constexpr uint32_t WIRE_BATCH = 16;  // buckets per batched wire launch
struct WireBucket {
    const uint32_t *idx;
    const float *val;
    void *idx_out, *val_out;
    uint64_t n;
    uint32_t flag, blk0;  // blk0: first workgroup of this bucket in the launch
};
struct WireBatch {
    WireBucket t[WIRE_BATCH];
    uint32_t nt;
};
hipError_t launch_wire_encode_batch(const WireBatch &w, uint32_t blocks, hipStream_t s);
// The one-call MERGE send path (send_batch.hip): the gather-add before the
// scans and the error feedback + wire packing after them, each for up to
// SEND_BATCH tensors per launch.  The tables travel by value in the kernel
// arguments, workgroups dealt by blk0 as above.
constexpr uint32_t SEND_BATCH = 16;                   // tensors per launch of either kernel
constexpr uint32_t SEND_GATHER_TILE = STG_WG * 16;    // elements per gather workgroup (four float4 per lane)
struct SendGather {
    float *dst;                    // grad[0]
    const float *resid;            // residual term (or null)
    const void *src[GATHER_MAX];   // src[1 .. nsrc-1] = grad[1 .. N-1]; src[0] as GatherArgs::src[0]
    uint64_t n;
    uint32_t nsrc;                 // N
    uint32_t blk0;                 // first workgroup of this tensor in the launch
    uint32_t vec;                  // fp32 launch: every pointer shares one 16-byte phase (float4 body);
                                   // typed launch: GatherPlan::width (0: scalar tiles)
    uint32_t head;                 // vec: elements before the first lane group (< 4; typed: < 8; <= n)
    uint32_t dtypes;               // as GatherArgs::dtypes (typed launch)
};
struct SendGatherBatch {
    SendGather t[SEND_BATCH];
    uint32_t nt;
};
static_assert(sizeof(SendGatherBatch) <= 3072, "kernel arguments: stay under 4 KiB");
hipError_t launch_gather_add_batch(const SendGatherBatch &w, uint32_t blocks, hipStream_t s);
// the same launch for tables with a 16-bit source or a typed first term (vec = the plan's width)
hipError_t launch_gather_add_batch_typed(const SendGatherBatch &w, uint32_t blocks, hipStream_t s);
// workgroups of a typed task of n elements under plan p
inline uint64_t send_gather_blocks(uint64_t n, GatherPlan p) {
    const uint64_t per = p.width ? SEND_GATHER_TILE / p.width : SEND_GATHER_TILE;
    const uint64_t units = p.width ? (n - p.head) / p.width : n;
    return units ? (units + per - 1) / per : 1;
}
struct SendFinish {
    const uint32_t *idx;           // the scan's staged pairs: true indices (+ idx_offset) ...
    const float *val;              // ... and values, `count` of each
    void *idx_out, *val_out;       // the task's wire-form outputs, typed by flag
    float *grad, *resid;           // error feedback (resid null: pack only)
    uint64_t n;
    uint32_t count;                // min(idx_cap, n) pairs
    uint32_t flag, blk0;
    uint32_t zero0;                // idx_cap > count: the unused slots' index 0 is zeroed too
};
struct SendFinishBatch {
    SendFinish t[SEND_BATCH];
    uint32_t nt;
};
static_assert(sizeof(SendFinishBatch) <= 2048, "kernel arguments: stay well under 4 KiB");
hipError_t launch_ef_pack_batch(const SendFinishBatch &w, uint32_t blocks, hipStream_t s);
// The same path for threshold-v (tv_batch.hip, send_batch.hip): one scan launch
// for up to SEND_BATCH tasks, then a finish that reads each task's pair count
// from the device.
//
// The scan's ranges (1024-thread workgroups, as tv_pass's): a task of n floats
// takes tv_batch_ranges(n), each of at most TV_BATCH_RANGE float4; a launch
// closes at SEND_BATCH tasks or before its ranges would pass
// tv_batch_range_cap(num_cu); a task with more ranges than that runs alone
// through launch_tv.
constexpr uint32_t TV_BATCH_RANGE = 4096;  // float4 per range at most (64 KiB)
inline uint64_t tv_batch_ranges(uint64_t n) {
    return std::max<uint64_t>(1, (n / 4 + TV_BATCH_RANGE - 1) / TV_BATCH_RANGE);
}
inline uint64_t tv_batch_range_cap(int num_cu) {
    return std::max<uint64_t>(1, std::min<uint64_t>(TV_MAXG, (uint64_t)std::max(num_cu, 1)));
}
struct TvBatchTask {
    const float *src;              // the gathered grad[0]
    float *resid;                  // receives every element of src (null: no error feedback)
    uint32_t *idx;                 // staged pairs: positions ...
    float *val;                    // ... and values, cap of each
    uint32_t *count_out;
    KeyState *state;
    uint64_t n;
    uint32_t k, cap;
    uint32_t blk0;                 // the task's first range (ticket) in the launch
    uint32_t ranges;               // tv_batch_ranges(n)
};
struct TvBatch {
    TvBatchTask t[SEND_BATCH];
    uint32_t nt;
    uint32_t tag;                  // the launch's tag (>= 1) on every range word, from the workspace's tv_pass sequence
    uint64_t base;                 // ws.tv_ticket's value when the launch starts (it advances by the launch's ranges)
};
static_assert(sizeof(TvBatch) <= 2048, "kernel arguments: stay well under 4 KiB");
// ranges = the sum of the tasks' ranges <= tv_batch_range_cap; the range words
// are ws.tile_cnt / ws.tile_aux (TV_MAXG pairs, zero when fresh), as launch_tv's
hipError_t launch_tv_batch(const TvBatch &w, uint32_t ranges, const DevWS &ws, hipStream_t s);
// a key's first threshold from its gathered bucket (tv.hip's, ahead of the scan launch)
hipError_t launch_tv_first(const float *src, size_t n, uint32_t k, KeyState *state, const DevWS &ws, int num_cu,
                           hipStream_t s);
struct SendFinishDc {
    const uint32_t *idx;           // the scan's staged pairs, *count of them valid
    const float *val;
    const uint32_t *count;         // the task's device count (POISON_COUNT: nothing is written)
    void *idx_out, *val_out;       // the task's wire-form outputs, typed by flag
    float *grad, *resid;           // error feedback (resid null: pack only)
    uint64_t n;
    uint32_t slots;                // W = min(idx_cap, n): all of them are written
    uint32_t flag, blk0;
};
struct SendFinishDcBatch {
    SendFinishDc t[SEND_BATCH];
    uint32_t nt;
};
static_assert(sizeof(SendFinishDcBatch) <= 2048, "kernel arguments: stay well under 4 KiB");
hipError_t launch_ef_pack_batch_dc(const SendFinishDcBatch &w, uint32_t blocks, hipStream_t s);
// The same path for exact top-k (topk_batch.hip): a batched radix select and
// ordered emission for up to SEND_BATCH tasks, then ef_pack_batch with count =
// W = min(idx_cap, n) (the emission stages the unused slots as (0, 0.0f)).
//
// Tiles are TV_TILE floats, one 256-thread workgroup each: a task of n floats
// takes topk_batch_tiles(n); a group closes at SEND_BATCH tasks or before its
// tiles would pass topk_batch_tile_cap(num_cu); a task with more tiles than
// that runs alone through launch_topk1 / launch_topk.
inline uint64_t topk_batch_tiles(uint64_t n) { return std::max<uint64_t>(1, (n + TV_TILE - 1) / TV_TILE); }
// One tile per compute unit: a group's five passes re-read at most num_cu x 32
// KiB (8 MiB at 256 CUs), which stays in the cache between the launches, and
// every pass is a single wave of workgroups.  Larger buckets are bandwidth
// bound, where the per-tensor route reads the bucket once.
inline uint64_t topk_batch_tile_cap(int num_cu) { return (uint64_t)std::max(num_cu, 1); }
constexpr float TOPK_HINT_SEED = 1.0f / 256.0f;  // KeyState.inc of a key's first call (topk1.hip's D_SEED, tk2_seed)
// A task slot's select block: zero at allocation and after every complete group
// (the last workgroup of each pass zeroes what the pass filled).
struct alignas(128) TopkBatchSel {
    uint32_t done[3];              // workgroups done with level 1, 2, 3 (the last one picks, then zeroes it)
    uint32_t prefix;               // bits of T fixed so far; T after level 3
    uint32_t rank;                 // remaining descending rank inside the prefix
    uint32_t cnt_gt;               // keys strictly above the prefix range; above T after level 3
    uint32_t pad[26];
    uint32_t hist[2048 + 2048 + 512];  // the three levels' bins (11 / 11 / 9 bits)
};
struct TopkBatchTask {
    const float *src;              // the gathered grad[0]
    float *resid;                  // receives every element of src (null: no error feedback)
    uint32_t *idx;                 // staged pairs: indices (+ idx_offset) ...
    float *val;                    // ... and values, slots of each written
    uint32_t *count_out;           // = cap (POISON_COUNT after FAIL_SELECT)
    KeyState *state;               // t = T, init = 1 (inc seeded when init was 0)
    TopkBatchSel *sel;
    uint32_t n;
    uint32_t kk;                   // min(k, n) winners
    uint32_t cap;                  // idx_cap
    uint32_t slots;                // W = min(idx_cap, n): [kk, W) staged as (0, 0.0f)
    int32_t idx_offset;
    uint32_t blk0;                 // the task's first tile (workgroup) in the group
    uint32_t tiles;                // topk_batch_tiles(n)
};
struct TopkBatch {
    TopkBatchTask t[SEND_BATCH];
    uint32_t nt;
    uint32_t *tile_gt, *tile_eq;   // per tile of the group: keys > T and == T (ws.tile_cnt / ws.tile_aux)
    uint32_t *fail;                // the workspace's sticky failure word
};
static_assert(sizeof(TopkBatch) <= 2048, "kernel arguments: stay well under 4 KiB");
// tiles = the sum of the tasks' tiles <= topk_batch_tile_cap; five launches whatever nt is
hipError_t launch_topk_batch(const TopkBatch &w, uint32_t tiles, hipStream_t s);
// Publishing a step's changed parameters to the node's model replicas
// (publish.hip): replica[j] = cvt(param[j]) at the indices of the step's
// merged stream, for up to PUBLISH_BATCH tasks per launch.  The table --
// replica pointers included, as SendGather's source pointers -- travels by
// value in the kernel arguments, workgroups dealt by blk0 as above.
constexpr uint32_t PUBLISH_BATCH = 16;    // tasks per launch
constexpr uint32_t PUBLISH_MAXR = 16;     // replicas per task
constexpr uint32_t PUBLISH_WP = 4;        // consecutive stream slots per lane, as MERGE_BATCH_WP
constexpr uint32_t PUBLISH_TILE = 1024;   // stream slots per workgroup
static_assert(PUBLISH_TILE == PUBLISH_WP * STG_WG, "one lane, PUBLISH_WP slots");
constexpr uint32_t PUBLISH_GRID_PER_CU = 8;  // a launch closes before num_cu * 8 workgroups, as the send path's gather
constexpr uint32_t PUBLISH_F32 = 0, PUBLISH_BF16 = 1, PUBLISH_F16 = 2;  // = STG_DT_*
struct PublishTask {
    const float *param;            // the master parameter, n floats (read only)
    const uint32_t *idx;           // the step's merged indices ...
    const uint32_t *count;         // ... and the device word that counts them
    void *rep[PUBLISH_MAXR];       // rep[0 .. nrep-1], element-aligned
    uint32_t dtypes;               // rep[r]'s type in bits 2 r, 2 r + 1 (one scalar word, not a table to load from)
    uint32_t n;
    uint32_t cap;                  // slots at idx: a count above it publishes nothing
    uint32_t nrep;
    uint32_t blk0;                 // first workgroup of this task in the launch
};
struct PublishBatch {
    PublishTask t[PUBLISH_BATCH];
    uint32_t nt;
};
static_assert(sizeof(PublishBatch) <= 3072, "kernel arguments: stay under 4 KiB");
// runs: consecutive indices take wide stores where the replica's address
// allows (false: every element a store of its own; kept for measurements)
hipError_t launch_param_publish_batch(const PublishBatch &w, uint32_t blocks, bool runs, hipStream_t s);
struct WireRx {  // one received stream of a batched decode
    const void *idx_in, *val_in;
    uint32_t *idx;
    float *val;
    uint64_t n;
    uint32_t flag, blk0;  // blk0: first workgroup of this stream in the launch
};
struct WireRxBatch {
    WireRx t[WIRE_BATCH];
    uint32_t nt;
};
hipError_t launch_wire_decode_batch(const WireRxBatch &w, uint32_t blocks, hipStream_t s);
hipError_t launch_wire_encode(const uint32_t *idx, const float *val, size_t n, uint32_t flag, void *idx_out,
                              void *val_out, int num_cu, hipStream_t s);
hipError_t launch_wire_decode(const void *idx_in, const void *val_in, size_t n, uint32_t flag, uint32_t *idx,
                              float *val, int num_cu, hipStream_t s);
hipError_t launch_ef_zero(float *grad, float *resid, const uint32_t *idx, size_t numel, size_t n, int num_cu,
                          hipStream_t s);
hipError_t launch_error_feedback(float *grad, size_t n, const uint32_t *idx, size_t numel, float *resid, int num_cu,
                                 hipStream_t s);

}  // namespace stg
