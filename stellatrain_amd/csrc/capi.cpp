// capi.cpp -- host side of the C-ABI declared in include/stg/codec.h.
//
// Owns: codec handles (method, device), the per-key AIMD state slots (device
// resident, 16 B each, in never-moving chunks), and one workspace per HIP
// stream.  The reference keeps the threshold maps in the compressor object
// behind a mutex (thresholdv16.h:11-14, thresholdv16.cpp:84-91,255-258) and
// is called concurrently from up to 32 ThreadPool workers on different keys
// (engine/config.h:7, core_module_api.cpp:7-24); here every call locks the
// handle only to look up its slot and its stream's workspace, and the launch
// sequence of one call holds that workspace's lock so calls sharing a stream
// cannot interleave their kernels.
#include <cmath>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <map>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include <dlfcn.h>

#include "../../include/stg/codec.h"
#include "batch_pack.h"
#include "devbuf.h"
#include "scan_grid.h"
#include "ws.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

// a switch's value as read with getenv (unset: dflt)
int env_int(const char *e, int dflt) { return e ? atoi(e) : dflt; }

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return fail(STG_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

enum Method { M_TV16 = 0, M_TV = 1, M_TOPK = 2, M_TOPK_EXACT = 3 };

constexpr uint32_t SLOTS_PER_CHUNK = 4096;

// "current device and its CU count" for the entries that take no handle
// (the count of a device never changes: cached per device)
int device_cus(int *ncu, int *dev = nullptr) {
    static std::mutex mu;
    static std::unordered_map<int, int> cus;
    int d = 0;
    HIP_TRY(hipGetDevice(&d));
    if (dev) *dev = d;
    std::lock_guard<std::mutex> g(mu);
    auto it = cus.find(d);
    if (it == cus.end()) {
        int n = 256;
        HIP_TRY(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d));
        it = cus.emplace(d, n).first;
    }
    *ncu = it->second;
    return STG_OK;
}

// the one-bucket path's lists (tv16lone.hip) as one chunk's worth each, so the
// four buffers count their capacities in chunks
struct LqChunk { uint32_t w[stg::LQCAP]; };
struct LwChunk { uint2 w[stg::LWCAP]; };
struct LvChunk { float4 v[stg::LQCAP * 4]; };

struct Workspace {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    stg::DevWS d{};  // what the launchers take: set by init() and publish()
    // Grow-only scratch, each buffer with its own capacity.  Growing waits for
    // this stream's in-flight work.
    stg::DevBuf<char> fixed;
    stg::DevBuf<float> sums, stage_val;
    stg::DevBuf<uint32_t> tile_cnt, tile_aux, stage_pos;
    stg::DevBuf<stg::ChunkDesc> desc;
    stg::DevBuf<uint2> ldesc;
    stg::DevBuf<LqChunk> lq;
    stg::DevBuf<LwChunk> lw;
    stg::DevBuf<LvChunk> lv;
    uint32_t epoch = 0;  // thresholdv16 call counter (hand-off tags)
    uint32_t tk_tag = 0; // one-launch top-k call counter (topk1.hip)
    uint32_t lone_calls = 0;  // thresholdv16 one-bucket path calls (tv16.hip: parity of its per-call blocks)
    // threshold-v: the ticket's value at the next call and the last call's
    // range-descriptor tag
    uint64_t tv_base = 0;
    uint32_t tv_tag = 0;
    // device buffers of the host-memory entry point
    stg::DevBuf<float> h_src, h_val;
    stg::DevBuf<uint32_t> h_idx, h_count;
    uint32_t *pinned_count = nullptr;
    // one-bucket wire path staging (stg_codec_compress_wire_batch_device)
    std::mutex wire_mu;
    stg::DevBuf<uint32_t> wst_pos;
    stg::DevBuf<float> wst_val;
    // batched exact top-k (topk_batch.hip): a select block per task slot of a
    // group, zero at allocation and after every complete group
    stg::DevBuf<stg::TopkBatchSel> tkb_sel;

    ~Workspace() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (pinned_count) (void)hipHostFree(pinned_count);
    }

    int init() {
        size_t off = 0;
        auto carve = [&](size_t bytes) {
            const size_t o = off;
            off = (off + bytes + 255) & ~size_t(255);
            return o;
        };
        const size_t o_ctl = carve(sizeof(stg::FillCtl));
        const size_t o_cp = carve(sizeof(stg::CallParams));
        const size_t o_rs = carve(sizeof(stg::RSel));
        const size_t o_fail = carve(sizeof(uint32_t));
        const size_t o_cand = carve(sizeof(uint32_t) * stg::CAND_WORDS * stg::MAX_BATCH);
        const size_t o_misc = carve(sizeof(uint32_t) * 64);
        const size_t o_tvt = carve(sizeof(uint64_t));
        const size_t o_wh = carve(sizeof(uint32_t) * 2 * stg::LNBIN);
        const size_t o_larr = carve(sizeof(uint32_t) * stg::LARR_WORDS);
        const size_t o_we = carve(sizeof(uint2) * stg::LNBIN * stg::LBCAP);
        const size_t o_crew = carve(sizeof(stg::CrewCtl) * stg::MAX_BATCH);
        const size_t o_tkc = carve(sizeof(stg::TopkCtl) * 2);
        const size_t o_tkf = carve(sizeof(uint32_t) * 2 * stg::TK2_FINE);
        // zeroed on this workspace's stream: the launches that read the
        // control block are ordered after it (a plain hipMemset runs on the
        // null stream, which a non-blocking stream does not wait for)
        HIP_TRY(fixed.reserve(off, stream, true));
        char *b = fixed.get();
        d.ctl = reinterpret_cast<stg::FillCtl *>(b + o_ctl);
        d.cp = reinterpret_cast<stg::CallParams *>(b + o_cp);
        d.rsel = reinterpret_cast<stg::RSel *>(b + o_rs);
        d.fail = reinterpret_cast<uint32_t *>(b + o_fail);
        d.cand = reinterpret_cast<uint32_t *>(b + o_cand);
        d.misc = reinterpret_cast<uint32_t *>(b + o_misc);
        d.tv_ticket = reinterpret_cast<uint64_t *>(b + o_tvt);
        d.whist = reinterpret_cast<uint32_t *>(b + o_wh);
        d.larr = reinterpret_cast<uint32_t *>(b + o_larr);
        d.went = reinterpret_cast<uint2 *>(b + o_we);
        d.crew = reinterpret_cast<stg::CrewCtl *>(b + o_crew);
        d.tkctl = reinterpret_cast<stg::TopkCtl *>(b + o_tkc);
        d.tkfine = reinterpret_cast<uint32_t *>(b + o_tkf);
        return STG_OK;
    }

    // The grown buffers as the launchers see them; every sizing routine ends
    // here, whatever it returns, so d never names a freed block.
    int publish(hipError_t e) {
        d.sums = sums.get();
        d.desc = desc.get();
        d.tile_cnt = tile_cnt.get();
        d.tile_aux = tile_aux.get();
        d.stage_pos = stage_pos.get();
        d.stage_val = stage_val.get();
        d.ldesc = ldesc.get();
        d.lq = reinterpret_cast<uint32_t *>(lq.get());
        d.lw = reinterpret_cast<uint2 *>(lw.get());
        d.lv = reinterpret_cast<float4 *>(lv.get());
        if (e != hipSuccess) return fail(STG_ERR_HIP, std::string("workspace scratch: ") + hipGetErrorString(e));
        return STG_OK;
    }

    // thresholdv16 chunk descriptors: zeroed on (re)allocation, so no stale
    // word carries a live call tag (epochs start at 1)
    int ensure_desc(size_t n) { return publish(desc.reserve(n, stream, true)); }

    // one-bucket path lists (tv16lone.hip): per chunk a tagged count pair and
    // the qualifying / window line lists.  The finish inside the scan launch
    // (tv16lf2.h) POLLS the count pairs while chunks are still being listed and
    // takes a pair as this call's once its high word equals the call tag, so
    // the pairs are zeroed on (re)allocation: recycled device memory (a freed
    // workspace's pairs, whose tags restart at 1 in every workspace) could
    // otherwise already hold a live tag with another call's counts.  Tags are
    // >= 1 and only this workspace writes its pairs afterwards, so no stale
    // pair ever matches a later call.  The lists themselves are read only
    // behind a matched pair.  (nc <= LMAXC, which also bounds the growth.)
    int ensure_lone(size_t nc) {
        static const bool stale = env_int(getenv("STG_DEBUG_LDESC_STALE"), 0) == 1;
        bool fresh = false;
        hipError_t e = ldesc.reserve(nc, stream, !stale, &fresh, stg::LMAXC);
        if (e == hipSuccess) e = lq.reserve(nc, stream, false, nullptr, stg::LMAXC);
        if (e == hipSuccess) e = lw.reserve(nc, stream, false, nullptr, stg::LMAXC);
        if (e == hipSuccess) e = lv.reserve(nc, stream, false, nullptr, stg::LMAXC);
        if (e == hipSuccess && fresh && stale) {  // diagnostics: what a recycled block looks like (every pair tagged 1..8, counts 0)
            std::vector<uint2> p(ldesc.cap());
            for (size_t i = 0; i < p.size(); ++i) p[i] = make_uint2(0u, 1u + (uint32_t)(i & 7u));
            e = hipMemcpyAsync(ldesc.get(), p.data(), p.size() * sizeof(uint2), hipMemcpyHostToDevice, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
        }
        return publish(e);
    }
    // chunks every one-bucket list holds
    size_t lone_cap() const { return std::min({ldesc.cap(), lq.cap(), lw.cap(), lv.cap()}); }

    int ensure_wire_stage(size_t n) {  // (caller holds wire_mu)
        HIP_TRY(wst_pos.reserve(n, stream, false));
        HIP_TRY(wst_val.reserve(n, stream, false));
        return STG_OK;
    }

    // zero_tiles: the tile words carry call tags (threshold-v), so fresh memory is zeroed
    int ensure(size_t nsums, size_t tiles, size_t stage, bool zero_tiles = false) {
        hipError_t e = sums.reserve(nsums, stream, false);
        if (e == hipSuccess) e = tile_cnt.reserve(tiles, stream, zero_tiles);
        if (e == hipSuccess) e = tile_aux.reserve(tiles, stream, zero_tiles);
        if (e == hipSuccess) e = stage_pos.reserve(stage, stream, false);
        if (e == hipSuccess) e = stage_val.reserve(stage, stream, false);
        return publish(e);
    }
};

}  // namespace

struct stg_codec {
    Method method;
    int device = 0;
    int num_cu = 256;
    std::string name;
    std::mutex mu;
    std::unordered_map<std::string, uint32_t> slot_of;
    std::vector<stg::DevBuf<KeyState>> chunks;  // never-moving blocks of SLOTS_PER_CHUNK states
    uint32_t nslots = 0;
    std::unordered_map<hipStream_t, std::unique_ptr<Workspace>> ws;
    // kernel timing (stg_codec_set_timing)
    bool timing = false;
    std::vector<std::array<hipEvent_t, 3>> ev_pending, ev_pool;
    double ms_acc[3] = {0, 0, 0};
    uint64_t timed_calls = 0;

    ~stg_codec() {
        (void)hipSetDevice(device);
        ws.clear();
        for (auto *v : {&ev_pending, &ev_pool})
            for (auto &e : *v)
                for (auto x : e) (void)hipEventDestroy(x);
    }

    // Events for one timed call (nullptr when timing is off).
    int take_events(std::array<hipEvent_t, 3> *e, bool *on) {
        std::lock_guard<std::mutex> g(mu);
        *on = timing;
        if (!timing) return STG_OK;
        if (!ev_pool.empty()) { *e = ev_pool.back(); ev_pool.pop_back(); }
        else for (auto &x : *e) HIP_TRY(hipEventCreate(&x));
        ev_pending.push_back(*e);
        return STG_OK;
    }

    KeyState *slot_ptr(uint32_t s) { return chunks[s / SLOTS_PER_CHUNK].get() + (s % SLOTS_PER_CHUNK); }

    // Returns the state slot of `key`; *fresh = true when it was just created.
    int slot(const std::string &key, KeyState **out, bool *fresh) {
        std::lock_guard<std::mutex> g(mu);
        auto it = slot_of.find(key);
        if (it != slot_of.end()) { *out = slot_ptr(it->second); *fresh = false; return STG_OK; }
        if (nslots % SLOTS_PER_CHUNK == 0) {
            stg::DevBuf<KeyState> c;
            // states are read on any stream: zero them before any launch sees them
            HIP_TRY(c.reserve(SLOTS_PER_CHUNK, nullptr, true));
            HIP_TRY(hipStreamSynchronize(nullptr));
            chunks.push_back(std::move(c));
        }
        const uint32_t s = nslots++;
        slot_of.emplace(key, s);
        *out = slot_ptr(s);
        *fresh = true;
        return STG_OK;
    }

    int workspace(hipStream_t s, Workspace **out) {
        std::lock_guard<std::mutex> g(mu);
        auto it = ws.find(s);
        if (it != ws.end()) { *out = it->second.get(); return STG_OK; }
        auto w = std::make_unique<Workspace>();
        w->device = device;
        w->stream = s;
        int rc = w->init();
        if (rc) return rc;
        *out = w.get();
        ws.emplace(s, std::move(w));
        return STG_OK;
    }
};

struct stg_sgd {
    int device = 0;
    float lr, momentum, dampening, weight_decay;
    bool nesterov, maximize;
    uint32_t iter = 0;
    std::mutex mu;
    // per-name state: the buffer and the param_len it was created for
    template <typename T>
    struct Named {
        stg::DevBuf<T> buf;
        uint32_t len = 0;
    };
    std::unordered_map<std::string, Named<float>> mom;
    // smart momentum (sgd.cpp:54, 225-232, 258-259)
    bool smart = false;
    std::unordered_map<std::string, Named<uint32_t>> last;  // per name, zeroed when first needed
    stg::DevBuf<float> pow_tab;  // pow(momentum, d), d < its capacity; built once (the momentum never changes), kept until destroy
    stg::DevBuf<uint32_t> fail;  // device failure word (SGD_FAIL_FACTOR)
    ~stg_sgd() { (void)hipSetDevice(device); }  // (the members free on this device)
};

struct stg_adam {
    int device = 0;
    stg::DevBuf<uint32_t> fail;  // device failure word (amsgrad look-back timeout)
    float lr, b1, b2, eps, weight_decay;
    bool amsgrad, maximize;
    struct Name {
        stg::DevBuf<float> mvv;       // one allocation: m | v | vmax (L, L and 1 floats, L = max(len, 1))
        stg::DevBuf<uint64_t> tiles;  // amsgrad look-back words, one per ADAM_TILE of param_len
        uint32_t len = 0, tick = 1;
        float *m() const { return mvv.get(); }
        float *v() const { return mvv.get() + std::max<size_t>(len, 1); }
        float *vmax() const { return mvv.get() + 2 * std::max<size_t>(len, 1); }
    };
    std::mutex mu;
    std::unordered_map<std::string, Name> st;
    ~stg_adam() { (void)hipSetDevice(device); }  // (the members free on this device)
};

namespace {

std::string state_key(Method m, const char *key, const void *src) {
    if (m == M_TV) {  // thresholdv.cpp:44: keyed by the src pointer
        char b[32];
        snprintf(b, sizeof b, "\x01%p", src);
        return b;
    }
    return key ? std::string(key) : std::string();
}

// Device-wide admission of thresholdv16 launches.  No launch waits on a
// workgroup that is not running (chunks are taken dynamically), so admission
// is a throughput policy, not a correctness one.  (Scans one at a time per
// device, each waiting for the previous one's on another stream, measured
// slower: profiles/r02_streams.jsonl.)
//  * STG_TV16_INFLIGHT (1-4; default unlimited) launches per device in
//    flight: a launch on stream s first makes s wait for the oldest in-flight
//    launch of another stream when the lane is full.  Unlimited (the default)
//    records no events at all: concurrent callers on their own streams
//    overlap freely (the reference's per-task compress() from many pool
//    workers, engine/modules/compress.cpp:141, core_module_api.cpp:7-24).
//  * The streams of the device's last 16 batched launches (all handles of
//    the process) size a launch's grid: see launch_tv16_group.
struct FusedLane {
    std::mutex mu;
    std::vector<std::pair<hipEvent_t, hipStream_t>> inflight;  // oldest first
    std::vector<hipEvent_t> pool;
    static constexpr uint32_t RING = 16;
    hipStream_t ring[RING] = {};
    uint32_t ring_n = 0, ring_at = 0;
    // Records a batched launch on stream s; returns the distinct streams among
    // the last RING launches, this one included (caller holds mu).
    uint32_t note_stream(hipStream_t s) {
        ring[ring_at] = s;
        ring_at = (ring_at + 1) % RING;
        ring_n = std::min(ring_n + 1, RING);
        uint32_t distinct = 0;
        for (uint32_t i = 0; i < ring_n; ++i) {
            bool seen = false;
            for (uint32_t j = 0; j < i; ++j) seen |= ring[j] == ring[i];
            distinct += !seen;
        }
        return distinct;
    }
};

FusedLane g_lanes[64];

// Hardware queues of the process: GPU_MAX_HW_QUEUES as the HIP runtime reads
// it (default 4).  Only read, never set.
uint32_t hw_queues() {
    static const uint32_t v = (uint32_t)std::max(1, env_int(getenv("GPU_MAX_HW_QUEUES"), 4));
    return v;
}

// Diagnostics: STG_DEBUG_TV16_GRID = workgroups of every thresholdv16 scan
// launch (1 .. TV16_MAXG; unset or 0: the policy above).  Read once.
uint32_t forced_grid() {
    static const uint32_t v =
        (uint32_t)std::min<int>(std::max(0, env_int(getenv("STG_DEBUG_TV16_GRID"), 0)), stg::TV16_MAXG);
    return v;
}

uint32_t fused_inflight() {  // 0: unlimited
    static const uint32_t v = (uint32_t)std::min(4, std::max(0, env_int(getenv("STG_TV16_INFLIGHT"), 0)));
    return v;
}

thread_local std::unordered_map<int, hipStream_t> t_streams;

int thread_stream(int device, hipStream_t *s) {
    auto it = t_streams.find(device);
    if (it != t_streams.end()) { *s = it->second; return STG_OK; }
    hipStream_t st;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    t_streams.emplace(device, st);
    *s = st;
    return STG_OK;
}

int validate(const stg_codec *h, size_t n, uint32_t k, size_t idx_cap, size_t val_cap, const uint32_t *d_count) {
    if (val_cap < idx_cap) return fail(STG_ERR_INVALID, "value capacity smaller than index capacity");
    if ((h->method == M_TOPK || h->method == M_TOPK_EXACT) && idx_cap < k)
        return fail(STG_ERR_INVALID, "Invalid parameter k");  // topk.cpp:33-34
    if (n >= (size_t(1) << 32) || idx_cap >= (size_t(1) << 32))
        return fail(STG_ERR_UNSUPPORTED, "bucket larger than 2^32-1 elements (uint32 indices)");
    if (!d_count) return fail(STG_ERR_INVALID, "null count pointer");
    return STG_OK;
}

// One thresholdv16 launch over `nb` buckets with distinct keys (caller holds
// ws->mu).  Scratch is carved per bucket from ws->d.sums: the first-threshold
// line sums, later the fill's candidate heap (two words per line).
int launch_tv16_group(stg_codec *h, Workspace *ws, std::vector<stg::Tv16Bucket> &grp, hipStream_t s) {
    if (grp.empty()) return STG_OK;
    size_t need = 0;
    for (auto &b : grp) need += 2 * ((b.n + 15) / 16 + 64);
    int rc;
    if ((rc = ws->ensure(need, 1, 1))) return rc;
    size_t off = 0, chunks = 0;
    for (auto &b : grp) {
        b.sums = ws->sums.get() + off;
        off += 2 * ((b.n + 15) / 16 + 64);
        chunks += std::max<size_t>(1, (b.n / 16 + stg::TV16_CHUNK - 1) / stg::TV16_CHUNK);
    }
    if ((rc = ws->ensure_desc(chunks))) return rc;
    if (grp.size() == 1) {  // the one-bucket path's lists (tv16lone.hip), in its own chunks
        const size_t lc = std::max<size_t>(1, (grp[0].n / 16 + stg::LCHUNK - 1) / stg::LCHUNK);
        if (lc <= stg::LMAXC && (rc = ws->ensure_lone(lc))) return rc;
    }
    std::array<hipEvent_t, 3> evs{};
    bool timed = false;
    if ((rc = h->take_events(&evs, &timed))) return rc;
    // 24-bit call epochs tag every hand-off word ({epoch:24 | kind:8});
    // epoch parity selects the per-call counters.  On wrap, clear the blocks.
    if (++ws->epoch >= (1u << 24)) {
        ws->epoch = 1;
        HIP_TRY(hipMemsetAsync(ws->d.ctl, 0, sizeof(stg::FillCtl), s));
        HIP_TRY(hipMemsetAsync(ws->desc.get(), 0, ws->desc.cap() * sizeof(stg::ChunkDesc), s));
    }
    stg::Tv16Launch a{};
    a.b = grp.data();
    a.nb = (uint32_t)grp.size();
    a.num_cu = h->num_cu;
    a.ev = timed ? evs.data() : nullptr;
    a.epoch = ws->epoch;
    const uint32_t inflight = fused_inflight();
    // A one-bucket launch may use the whole chip (two scan workgroups per
    // CU).  A batched launch takes its share of it by the streams that
    // launched the device's last scans (scan_grid.h): workgroups past what the
    // launch can keep streaming start only after its chunks are gone, take
    // nothing and leave, holding slots other launches' workgroups wait for.
    a.max_wg = (uint32_t)(2 * h->num_cu);
    if (grp.size() > 1) {
        FusedLane &lane = g_lanes[h->device & 63];
        std::lock_guard<std::mutex> lg(lane.mu);
        chunks = std::min<size_t>(chunks, 0xffffffffu);
        a.max_wg = stg::tv16_scan_grid((uint32_t)h->num_cu, lane.note_stream(s), hw_queues(), (uint32_t)chunks);
    }
    if (const uint32_t forced = forced_grid()) a.max_wg = forced;
    a.desc_cap = (uint32_t)std::min<size_t>(ws->desc.cap(), 0xffffffffu);
    a.lone_cap = (uint32_t)ws->lone_cap();
    a.lone_calls = &ws->lone_calls;
    if (!inflight) {  // no admission: nothing to track
        HIP_TRY(stg::launch_tv16(a, ws->d, s));
        grp.clear();
        return STG_OK;
    }
    FusedLane &lane = g_lanes[h->device & 63];
    std::lock_guard<std::mutex> lg(lane.mu);
    const size_t max_inflight = inflight;
    while (lane.inflight.size() >= max_inflight) {
        auto old = lane.inflight.front();
        lane.inflight.erase(lane.inflight.begin());
        if (old.second != s) HIP_TRY(hipStreamWaitEvent(s, old.first, 0));
        lane.pool.push_back(old.first);
    }
    HIP_TRY(stg::launch_tv16(a, ws->d, s));
    hipEvent_t done;
    if (!lane.pool.empty()) { done = lane.pool.back(); lane.pool.pop_back(); }
    else HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(done, s));
    lane.inflight.emplace_back(done, s);
    grp.clear();
    return STG_OK;
}

// thresholdv16 over a sequence of buckets: runs of distinct keys (<= 16)
// share one launch; the per-key state makes a repeated key wait for the
// launch that updates it.  `gather` (if any) belongs to bucket gather_at.
int run_tv16(stg_codec *h, const stg_bucket_t *bk, size_t nbk, hipStream_t s, float *const *resid = nullptr,
             const stg::GatherArgs *gather = nullptr, const int *wire_flags = nullptr, size_t gather_at = 0) {
    HIP_TRY(hipSetDevice(h->device));
    Workspace *ws = nullptr;
    int rc = h->workspace(s, &ws);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(ws->mu);
    std::vector<stg::Tv16Bucket> grp;
    grp.reserve(stg::MAX_BATCH);
    for (size_t i = 0; i < nbk; ++i) {
        const stg_bucket_t &b = bk[i];
        if (b.n == 0) {
            HIP_TRY(hipMemsetAsync(b.d_count, 0, sizeof(uint32_t), s));
            continue;
        }
        KeyState *st;
        bool fresh;
        if ((rc = h->slot(state_key(h->method, b.key, b.d_src), &st, &fresh))) return rc;
        bool dup = false;
        for (auto &x : grp) dup |= x.state == st;
        if (dup || grp.size() == stg::MAX_BATCH)
            if ((rc = launch_tv16_group(h, ws, grp, s))) return rc;
        stg::Tv16Bucket t{};
        t.src = b.d_src;
        t.n = b.n;
        t.k = b.k;
        t.dst_len = (uint32_t)b.idx_cap;
        t.idx = b.d_idx;
        t.val = b.d_val;
        t.idx_offset = b.idx_offset;
        t.count_out = b.d_count;
        t.state = st;
        t.first = fresh;
        t.resid = resid ? resid[i] : nullptr;
        t.gather = i == gather_at ? gather : nullptr;
        t.wflag = wire_flags ? (uint32_t)wire_flags[i] & 3u : 0u;
        grp.push_back(t);
    }
    return launch_tv16_group(h, ws, grp, s);
}

// ModuleCompress::run MERGE error feedback (compress.cpp:172-186) after the
// codec: the ragged tail (not streamed by the fused kernel) is copied, then the
// numel = idx_cap selected slots are zeroed in the bucket and the residual.
int ef_after(stg_codec *h, const stg_bucket_t &b, float *resid, bool fused, hipStream_t s) {
    float *g = const_cast<float *>(b.d_src);
    if (!fused) {
        HIP_TRY(stg::launch_error_feedback(g, b.n, b.d_idx, b.idx_cap, resid, h->num_cu, s));
        return STG_OK;
    }
    const size_t full = b.n / 16 * 16;
    if (b.n > full)
        HIP_TRY(hipMemcpyAsync(resid + full, g + full, (b.n - full) * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(stg::launch_ef_zero(g, resid, b.d_idx, b.idx_cap, b.n, h->num_cu, s));
    return STG_OK;
}

// One top-k bucket (n > 0) through the per-tensor launches; the caller holds ws->mu.
int run_topk_one(stg_codec *h, Workspace *ws, const stg_bucket_t &b, const void *key_ptr, hipEvent_t *ev,
                 hipStream_t s) {
    int rc;
    const size_t n = b.n;
    const size_t ntiles = (n + stg::TV_TILE - 1) / stg::TV_TILE;
    // superset entries (two words each, stg::TOPK_SUP_CAP per tile); per-tile
    // counts, their prefixes and the superset counts
    // + the level-2 bin's list (two words per key)
    // (whole groups of TK2_REG tiles: topk1.hip's fixed superset slots)
    const size_t stiles = (ntiles + stg::TK2_REG - 1) / stg::TK2_REG * stg::TK2_REG;
    if ((rc = ws->ensure(2 * stiles * stg::TOPK_SUP_CAP + 2 * stg::TOPK_LIST_CAP, 3 * ntiles + 1, 1))) return rc;
    stg::TopkLaunch a{b.d_src, n, b.k, (uint32_t)b.idx_cap, b.d_idx, b.d_val, b.idx_offset, h->method == M_TOPK,
                      b.d_count, h->num_cu, ev};
    const size_t m = h->method == M_TOPK ? (n + 3) / 4 : n;
    if ((m + stg::TV_TILE - 1) / stg::TV_TILE <= stg::TOPK_LIST_TILES) {
        // one launch, steered by the key's last k-th magnitude (its first call: the select inside it)
        KeyState *st;
        bool fresh;
        if ((rc = h->slot(state_key(h->method, b.key, key_ptr), &st, &fresh))) return rc;
        HIP_TRY(stg::launch_topk1(a, ws->d, st, !fresh, &ws->tk_tag, s));
    } else {
        HIP_TRY(stg::launch_topk(a, ws->d, s));
    }
    return STG_OK;
}

int run_device(stg_codec *h, const char *key, const float *d_src, const void *key_ptr, size_t n, uint32_t k,
               uint32_t *d_idx, size_t idx_cap, float *d_val, size_t val_cap, int32_t idx_offset, uint32_t *d_count,
               hipStream_t s) {
    if (!h) return fail(STG_ERR_INVALID, "null codec handle");
    int rc = validate(h, n, k, idx_cap, val_cap, d_count);
    if (rc) return rc;
    if (h->method == M_TV16) {
        const stg_bucket_t b{key, d_src, n, k, d_idx, idx_cap, d_val, val_cap, idx_offset, d_count};
        return run_tv16(h, &b, 1, s);
    }
    HIP_TRY(hipSetDevice(h->device));
    Workspace *ws = nullptr;
    if ((rc = h->workspace(s, &ws))) return rc;
    std::lock_guard<std::mutex> g(ws->mu);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(uint32_t), s));
        return STG_OK;
    }
    std::array<hipEvent_t, 3> evs{};
    bool timed = false;
    if ((rc = h->take_events(&evs, &timed))) return rc;
    hipEvent_t *ev = timed ? evs.data() : nullptr;
    if (h->method == M_TV) {
        KeyState *st;
        bool fresh;
        if ((rc = h->slot(state_key(h->method, key, key_ptr), &st, &fresh))) return rc;
        // range descriptors (tv.hip): counts at tile_cnt, maxima at tile_aux, two words per range
        // (zeroed when fresh: no stale tags)
        if ((rc = ws->ensure(1, 2 * (size_t)stg::TV_MAXG, 1, true))) return rc;
        if (++ws->tv_tag == 0) ws->tv_tag = 1;
        uint32_t grid = 0;
        stg::TvLaunch a{d_src, n, k, (uint32_t)idx_cap, d_idx, d_val, d_count, st, fresh, h->num_cu, ev,
                        ws->tv_tag, ws->tv_base, &grid};
        HIP_TRY(stg::launch_tv(a, ws->d, s));
        ws->tv_base += grid;
    } else {
        const stg_bucket_t b{key, d_src, n, k, d_idx, idx_cap, d_val, val_cap, idx_offset, d_count};
        return run_topk_one(h, ws, b, key_ptr, ev, s);
    }
    return STG_OK;
}

// MERGE decompress scratch, one per (device, stream): the per-tile counts and
// the u32 winner words (zero between calls).  Keyed like the codec
// workspaces, so merges issued from one thread on several streams or devices
// never share scratch.  Growing waits for the stream's in-flight work.
struct MergeScratch {
    std::mutex mu;
    int device = 0;
    stg::DevBuf<uint32_t> tiles, win;
    // world == 1 in one launch: tagged per-tile counts (as many as `tiles`, zeroed
    // whenever reallocated); the tile ticket and the duplicate flag
    stg::DevBuf<uint64_t> desc, ticket;
    uint32_t tag = 0;
    stg::DevBuf<uint32_t> fail;  // sticky device failure word (a look-back that gave up)
    // batched launches (merge_batch.hip): a ticket, duplicate flag and failed-launch
    // tag per tensor slot, zero at creation; they share win, desc, tag and fail
    stg::DevBuf<stg::MergeSlotCtl> bctl;
    // batched world > 1 groups (merge_batch_world.hip): the group's dense floats
    // and mark bytes, zero at creation and after every call; its winner words
    // are `win`, its tile counts `tiles`
    stg::DevBuf<float> wdense;
    stg::DevBuf<uint8_t> wmark;
    // kernel launches the batched entries have enqueued on this stream (stg_merge_batch_launches)
    uint64_t launches = 0;
    ~MergeScratch() { (void)hipSetDevice(device); }  // (the members free on this device)
};
std::mutex g_merge_mu;
// shared: a caller holds its reference for the whole call, so a concurrent
// stg_scatter_merge_release never frees a scratch another thread has looked up
std::map<std::pair<int, hipStream_t>, std::shared_ptr<MergeScratch>> g_merge;

std::shared_ptr<MergeScratch> merge_scratch(int dev, hipStream_t s) {
    std::lock_guard<std::mutex> g(g_merge_mu);
    auto &slot = g_merge[{dev, s}];
    if (!slot) { slot = std::make_shared<MergeScratch>(); slot->device = dev; }
    return slot;
}

// Caller holds m->mu.  min_tiles: tagged tile counts a batched launch needs
// (the sum of its tensors' tiles; n is then the sum of their lengths).
// group: elements of dense and marks a batched world > 1 group needs (n is then
// that too, and world > 1: two winner words per element).
int merge_scratch_ensure(MergeScratch *m, hipStream_t s, size_t n, size_t per_rank, int world, size_t min_tiles = 0,
                         size_t group = 0) {
    // per-tile counts and their prefixes (the world > 1 mark scan)
    // ... and the world-1 emission's tagged tile counts (tiles of >= MERGE_TILE / 16 pairs)
    const size_t tiles = std::max({2 * ((std::max(n, per_rank) + stg::MERGE_TILE - 1) / stg::MERGE_TILE) + 2,
                                   (per_rank + stg::MERGE_TILE / 16 - 1) / (stg::MERGE_TILE / 16) + 2, min_tiles});
    // (sized to the need exactly, as the tile counts always were)
    HIP_TRY(m->tiles.reserve(tiles, s, false, nullptr, tiles));
    HIP_TRY(m->desc.reserve(tiles, s, true, nullptr, tiles));  // zeroed: no stale tags
    // [0]: the emission's tile ticket; [1]: the duplicate flag (low word)
    HIP_TRY(m->ticket.reserve(2, s, true));
    // [0] sticky failure bits, [1] the tag of the last call that failed
    HIP_TRY(m->fail.reserve(2, s, true));
    if (min_tiles) HIP_TRY(m->bctl.reserve(stg::MERGE_BATCH, s, true));
    if (group) {
        HIP_TRY(m->wdense.reserve(group, s, true));
        HIP_TRY(m->wmark.reserve(group, s, true));
    }
    const size_t words = std::max<size_t>(world > 1 ? 2 * n : n, 1);  // world > 1: two election halves
    HIP_TRY(m->win.reserve(words, s, true));
    return STG_OK;
}

// grad[0] += residual + grad[1 .. N-1] as the gather launchers take it
stg::GatherArgs gather_args(float *dst, const float *resid, const float *const *d_grads, int num_gpus) {
    stg::GatherArgs g{};
    g.dst = dst;
    g.resid = resid;
    g.nsrc = (uint32_t)num_gpus;
    for (int i = 1; i < num_gpus; ++i) g.src[i] = d_grads[i];
    return g;
}

// The same from typed sources (num_gpus in 1..16), checked: *why names what is
// refused (STG_ERR_INVALID): an unknown dtype, a pointer not aligned to its
// element, with n > 0 a null source at index >= 1 or a null array at
// num_gpus > 1.  srcs[0] null, or fp32 and equal to dst, is the in-place first
// term (src[0] stays null).  *typed: a launcher of the typed kernels is needed
// (a 16-bit source or a first term read from srcs[0]); otherwise g is what
// gather_args gives and the fp32 launchers take it.
int typed_gather_args(float *dst, const float *resid, const stg_grad_src_t *srcs, int num_gpus, uint64_t n,
                      stg::GatherArgs *g, bool *typed, std::string *why) {
    *g = stg::GatherArgs{};
    g->dst = dst;
    g->resid = resid;
    g->nsrc = (uint32_t)num_gpus;
    *typed = false;
    if (!srcs) {
        if (num_gpus > 1 && n) { *why = "null srcs"; return STG_ERR_INVALID; }
        g->nsrc = 1;
        return STG_OK;
    }
    for (int i = 0; i < num_gpus; ++i) {
        const stg_grad_src_t &x = srcs[i];
        if (!x.d_grad) {
            if (i == 0 || !n) continue;
            *why = "null source";
            return STG_ERR_INVALID;
        }
        if (x.dtype != STG_DT_F32 && x.dtype != STG_DT_BF16 && x.dtype != STG_DT_F16) {
            *why = "unknown source dtype";
            return STG_ERR_INVALID;
        }
        if (reinterpret_cast<uintptr_t>(x.d_grad) & (x.dtype == STG_DT_F32 ? 3u : 1u)) {
            *why = "source not aligned to its element size";
            return STG_ERR_INVALID;
        }
        if (i == 0 && x.dtype == STG_DT_F32 && x.d_grad == dst) continue;  // in place
        g->src[i] = x.d_grad;
        g->dtypes |= (uint32_t)x.dtype << (2 * i);
        *typed |= i == 0 || x.dtype != STG_DT_F32;
    }
    return STG_OK;
}

// The table of one of ws.h's batched launchers on stream s (batch_pack.h): a
// launch closes at the table's capacity or before its grid would pass `limit`.
template <class Table>
auto stream_packer(uint64_t limit, hipError_t (*launch)(const Table &, uint32_t, hipStream_t), hipStream_t s) {
    return stg::make_packer<Table>(limit, [launch, s](Table &w, uint32_t blocks) -> int {
        HIP_TRY(launch(w, blocks, s));
        return STG_OK;
    });
}
constexpr uint64_t GRID_MAX = 0x7fffffffull;  // workgroups of one launch

// The launches of a publish call (publish.hip), by the one rule the entry
// point and stg_debug_publish_launches share: task i of cap(i) > 0 index slots
// takes ceil(cap / PUBLISH_TILE) workgroups of a table that closes at
// PUBLISH_BATCH tasks or before num_cu * PUBLISH_GRID_PER_CU workgroups;
// fill(i, item) writes the item, launch(table, workgroups) enqueues it.
template <class Cap, class Fill, class Launch>
int publish_pack(size_t ntasks, int num_cu, Cap cap, Fill fill, Launch launch) {
    auto pk = stg::make_packer<stg::PublishBatch>((uint64_t)num_cu * stg::PUBLISH_GRID_PER_CU, launch);
    for (size_t i = 0; i < ntasks; ++i) {
        const uint32_t c = cap(i);
        if (!c) continue;
        stg::PublishTask *d;
        if (const int rc = pk.add(((uint64_t)c + stg::PUBLISH_TILE - 1) / stg::PUBLISH_TILE, &d)) return rc;
        fill(i, d);
    }
    return pk.flush();
}
// low address bits that must be clear for a replica of this STG_DT_* type
uintptr_t publish_elem_mask(int dtype) { return dtype == STG_DT_F32 ? 3u : 1u; }

// The scan launches of a threshold-v send call (tv_batch.hip), by the one rule
// the entry point and stg_debug_tv_batch_plan share: task i of n(i) > 0 floats
// takes tv_batch_ranges(n) ranges of a table that closes at SEND_BATCH tasks or
// before tv_batch_range_cap(num_cu) ranges; a task with more ranges than the
// cap runs alone(i) -- the pending table is launched first, so the launches
// keep the tasks' order.  fill(i, item) writes the item (blk0 and ranges are
// set), launch(table, ranges) enqueues it.
template <class N, class Fill, class Launch, class Alone>
int tv_batch_pack(size_t ntasks, int num_cu, N n, Fill fill, Launch launch, Alone alone) {
    const uint64_t cap = stg::tv_batch_range_cap(num_cu);
    auto pk = stg::make_packer<stg::TvBatch>(cap, launch);
    for (size_t i = 0; i < ntasks; ++i) {
        const uint64_t ni = n(i);
        if (!ni) continue;
        const uint64_t ranges = stg::tv_batch_ranges(ni);
        if (ranges > cap) {
            if (const int rc = pk.flush()) return rc;
            if (const int rc = alone(i)) return rc;
            continue;
        }
        stg::TvBatchTask *d;
        if (const int rc = pk.add(ranges, &d)) return rc;
        d->ranges = (uint32_t)ranges;
        fill(i, d);
    }
    return pk.flush();
}

// The threshold-v scans of a send call, after its gather launches: bk[i] is
// task i's bucket with d_idx / d_val pointing into the staging, res[i] its
// residual (the scan copies the gathered bucket to it) or null.
int run_tv_send(stg_codec *h, Workspace *ws, const stg_bucket_t *bk, float *const *res, size_t ntasks, hipStream_t s) {
    std::lock_guard<std::mutex> g(ws->mu);
    int rc;
    // range words (tv.hip): counts at tile_cnt, maxima at tile_aux, two words per range (zeroed when fresh)
    if ((rc = ws->ensure(1, 2 * (size_t)stg::TV_MAXG, 1, true))) return rc;
    std::vector<KeyState *> st(ntasks, nullptr);
    std::vector<char> fresh(ntasks, 0);
    const uint64_t cap = stg::tv_batch_range_cap(h->num_cu);
    for (size_t i = 0; i < ntasks; ++i) {
        const stg_bucket_t &b = bk[i];
        if (!b.n) {
            HIP_TRY(hipMemsetAsync(b.d_count, 0, sizeof(uint32_t), s));
            continue;
        }
        bool f;
        if ((rc = h->slot(state_key(h->method, b.key, b.d_src), &st[i], &f))) return rc;
        fresh[i] = f;
        // a key's first call: its threshold from the gathered bucket, ahead of
        // the scan launch (a task that runs alone: inside launch_tv)
        if (f && stg::tv_batch_ranges(b.n) <= cap)
            HIP_TRY(stg::launch_tv_first(b.d_src, b.n, b.k, st[i], ws->d, h->num_cu, s));
    }
    auto next_tag = [ws] {
        if (++ws->tv_tag == 0) ws->tv_tag = 1;
        return ws->tv_tag;
    };
    return tv_batch_pack(
        ntasks, h->num_cu, [&](size_t i) { return (uint64_t)bk[i].n; },
        [&](size_t i, stg::TvBatchTask *d) {
            const stg_bucket_t &b = bk[i];
            d->src = b.d_src;
            d->resid = res[i];
            d->idx = b.d_idx;
            d->val = b.d_val;
            d->count_out = b.d_count;
            d->state = st[i];
            d->n = b.n;
            d->k = b.k;
            d->cap = (uint32_t)b.idx_cap;
        },
        [&](stg::TvBatch &w, uint32_t ranges) -> int {
            w.tag = next_tag();
            w.base = ws->tv_base;
            HIP_TRY(stg::launch_tv_batch(w, ranges, ws->d, s));
            ws->tv_base += ranges;
            return STG_OK;
        },
        [&](size_t i) -> int {
            const stg_bucket_t &b = bk[i];
            uint32_t grid = 0;
            stg::TvLaunch a{b.d_src, b.n, b.k, (uint32_t)b.idx_cap, b.d_idx, b.d_val, b.d_count, st[i],
                            fresh[i] != 0, h->num_cu, nullptr, next_tag(), ws->tv_base, &grid};
            HIP_TRY(stg::launch_tv(a, ws->d, s));
            ws->tv_base += grid;
            // (tv_pass does not write the residual: the copy pass of the per-tensor sequence)
            if (res[i])
                HIP_TRY(hipMemcpyAsync(res[i], b.d_src, b.n * sizeof(float), hipMemcpyDeviceToDevice, s));
            return STG_OK;
        });
}

// The select groups of an exact top-k send call (topk_batch.hip), by the one
// rule the entry point and stg_debug_topk_batch_plan share: task i of n(i) > 0
// floats takes topk_batch_tiles(n) tiles of a table that closes at SEND_BATCH
// tasks or before topk_batch_tile_cap(num_cu) tiles; a task with more tiles
// than the cap runs alone(i) -- the pending table is launched first, so the
// groups keep the tasks' order.  fill(i, item) writes the item (blk0 and tiles
// are set), launch(table, tiles) enqueues the group.
template <class N, class Fill, class Launch, class Alone>
int topk_batch_pack(size_t ntasks, int num_cu, N n, Fill fill, Launch launch, Alone alone) {
    const uint64_t cap = stg::topk_batch_tile_cap(num_cu);
    auto pk = stg::make_packer<stg::TopkBatch>(cap, launch);
    for (size_t i = 0; i < ntasks; ++i) {
        const uint64_t ni = n(i);
        if (!ni) continue;
        const uint64_t tiles = stg::topk_batch_tiles(ni);
        if (tiles > cap) {
            if (const int rc = pk.flush()) return rc;
            if (const int rc = alone(i)) return rc;
            continue;
        }
        stg::TopkBatchTask *d;
        if (const int rc = pk.add(tiles, &d)) return rc;
        d->tiles = (uint32_t)tiles;
        fill(i, d);
    }
    return pk.flush();
}

// The exact top-k selects of a send call, after its gather launches: bk[i] is
// task i's bucket with d_idx / d_val pointing into the staging, res[i] its
// residual (the select's first pass copies the gathered bucket to it) or null.
// Every task has passed validation: the key slots are taken here.
int run_topk_send(stg_codec *h, Workspace *ws, const stg_bucket_t *bk, float *const *res, size_t ntasks,
                  hipStream_t s) {
    std::lock_guard<std::mutex> g(ws->mu);
    int rc;
    const uint64_t cap = stg::topk_batch_tile_cap(h->num_cu);
    // the groups' per-tile counts (tile_cnt / tile_aux) and the per-slot select blocks, zero when fresh
    if ((rc = ws->ensure(1, cap, 1))) return rc;
    HIP_TRY(ws->tkb_sel.reserve(stg::SEND_BATCH, s, true));
    std::vector<KeyState *> st(ntasks, nullptr);
    for (size_t i = 0; i < ntasks; ++i) {
        const stg_bucket_t &b = bk[i];
        if (!b.n) {
            HIP_TRY(hipMemsetAsync(b.d_count, 0, sizeof(uint32_t), s));
            continue;
        }
        bool fresh;  // (a fresh slot is zero: the level-3 pick seeds it as tk2_seed does)
        if (stg::topk_batch_tiles(b.n) <= cap &&
            (rc = h->slot(state_key(h->method, b.key, b.d_src), &st[i], &fresh)))
            return rc;
    }
    return topk_batch_pack(
        ntasks, h->num_cu, [&](size_t i) { return (uint64_t)bk[i].n; },
        [&](size_t i, stg::TopkBatchTask *d) {
            const stg_bucket_t &b = bk[i];
            d->src = b.d_src;
            d->resid = res[i];
            d->idx = b.d_idx;
            d->val = b.d_val;
            d->count_out = b.d_count;
            d->state = st[i];
            d->n = (uint32_t)b.n;
            d->kk = (uint32_t)std::min<size_t>(b.k, b.n);
            d->cap = (uint32_t)b.idx_cap;
            d->slots = (uint32_t)std::min<size_t>(b.idx_cap, b.n);
            d->idx_offset = b.idx_offset;
        },
        [&](stg::TopkBatch &w, uint32_t tiles) -> int {
            for (uint32_t j = 0; j < w.nt; ++j) w.t[j].sel = ws->tkb_sel.get() + j;
            w.tile_gt = ws->d.tile_cnt;
            w.tile_eq = ws->d.tile_aux;
            w.fail = ws->d.fail;
            HIP_TRY(stg::launch_topk_batch(w, tiles, s));
            return STG_OK;
        },
        [&](size_t i) -> int {
            // the per-tensor route into the staging slice: slots [min(k, n), W) as the zeroed temporaries hold them
            const stg_bucket_t &b = bk[i];
            const size_t kk = std::min<size_t>(b.k, b.n), slots = std::min<size_t>(b.idx_cap, b.n);
            if (slots > kk) {
                HIP_TRY(hipMemsetAsync(b.d_idx + kk, 0, (slots - kk) * sizeof(uint32_t), s));
                HIP_TRY(hipMemsetAsync(b.d_val + kk, 0, (slots - kk) * sizeof(float), s));
            }
            if ((rc = run_topk_one(h, ws, b, b.d_src, nullptr, s))) return rc;
            // (the per-tensor launches do not write the residual: the copy pass of the per-tensor sequence)
            if (res[i]) HIP_TRY(hipMemcpyAsync(res[i], b.d_src, b.n * sizeof(float), hipMemcpyDeviceToDevice, s));
            return STG_OK;
        });
}

}  // namespace

extern "C" {

const char *stg_last_error(void) { return g_err.c_str(); }

int stg_codec_create(const char *method, int device, stg_codec_t *out) {
    if (!method || !out) return fail(STG_ERR_INVALID, "null argument");
    const std::string m(method);
    auto h = std::make_unique<stg_codec>();
    if (m == "thresholdv16") { h->method = M_TV16; h->name = "Thresholdv16"; }
    else if (m == "thresholdv") { h->method = M_TV; h->name = "Thresholdv"; }
    else if (m == "topk") { h->method = M_TOPK; h->name = "Topk"; }
    else if (m == "topk_exact") { h->method = M_TOPK_EXACT; h->name = "Topk"; }
    else return fail(STG_ERR_UNKNOWN, "Unknown compression method " + m + ".");  // core.cpp:117
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(STG_ERR_INVALID, "no such HIP device");
    h->device = device;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipDeviceGetAttribute(&h->num_cu, hipDeviceAttributeMultiprocessorCount, device));
    *out = h.release();
    return STG_OK;
}

int stg_codec_destroy(stg_codec_t h) {
    delete h;
    return STG_OK;
}

const char *stg_codec_name(stg_codec_t h) { return h ? h->name.c_str() : ""; }

namespace {
// The reference times each compress task as "CRIT_PATH_compress"
// (engine/modules/compress.cpp:140-142, record_stat_start/end).  With
// STG_ROCTX=1 every compress entry point is a roctx range of that name, so
// `rocprofv3 --marker-trace --kernel-trace` shows the host side of each call
// next to its kernels.
struct CritPath {
    // the roctx library is opened only when STG_ROCTX=1 (no link-time
    // dependency on rocprofiler-sdk for an opt-in diagnostic); a missing
    // library leaves the ranges off
    typedef int (*push_fn)(const char *);
    typedef int (*pop_fn)();
    struct Api {
        push_fn push = nullptr;
        pop_fn pop = nullptr;
    };
    const Api &api;
    CritPath() : api(get()) {
        if (api.push) api.push("CRIT_PATH_compress");
    }
    ~CritPath() {
        if (api.pop) api.pop();
    }
    static const Api &get() {
        static const Api a = [] {
            Api r;
            if (env_int(getenv("STG_ROCTX"), 0) != 1) return r;
            void *h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
            if (!h) h = dlopen("/opt/rocm/lib/librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
            if (!h) return r;
            r.push = reinterpret_cast<push_fn>(dlsym(h, "roctxRangePushA"));
            r.pop = reinterpret_cast<pop_fn>(dlsym(h, "roctxRangePop"));
            if (!r.push || !r.pop) r = Api{};
            return r;
        }();
        return a;
    }
};
}  // namespace

int stg_codec_compress_device(stg_codec_t h, const char *key, const float *d_src, size_t n, uint32_t k,
                              uint32_t *d_idx, size_t idx_cap, float *d_val, size_t val_cap, int32_t idx_offset,
                              uint32_t *d_count, void *stream) {
    CritPath crit_path;
    return run_device(h, key, d_src, d_src, n, k, d_idx, idx_cap, d_val, val_cap, idx_offset, d_count,
                      static_cast<hipStream_t>(stream));
}

int stg_codec_compress_batch_device(stg_codec_t h, const stg_bucket_t *buckets, size_t nbuckets, void *stream) {
    CritPath crit_path;
    if (!h) return fail(STG_ERR_INVALID, "null codec handle");
    if (nbuckets && !buckets) return fail(STG_ERR_INVALID, "null bucket array");
    for (size_t i = 0; i < nbuckets; ++i) {
        const stg_bucket_t &b = buckets[i];
        const int rc = validate(h, b.n, b.k, b.idx_cap, b.val_cap, b.d_count);
        if (rc) return rc;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (h->method == M_TV16) return run_tv16(h, buckets, nbuckets, s);
    for (size_t i = 0; i < nbuckets; ++i) {
        const stg_bucket_t &b = buckets[i];
        const int rc = run_device(h, b.key, b.d_src, b.d_src, b.n, b.k, b.d_idx, b.idx_cap, b.d_val, b.val_cap,
                                  b.idx_offset, b.d_count, s);
        if (rc) return rc;
    }
    return STG_OK;
}

int stg_merge_compress_batch_device(stg_codec_t h, const stg_bucket_t *buckets, float *const *d_residuals,
                                    size_t nbuckets, void *stream) {
    CritPath crit_path;
    if (!h) return fail(STG_ERR_INVALID, "null codec handle");
    if (nbuckets && (!buckets || !d_residuals)) return fail(STG_ERR_INVALID, "null bucket or residual array");
    for (size_t i = 0; i < nbuckets; ++i) {
        const stg_bucket_t &b = buckets[i];
        const int rc = validate(h, b.n, b.k, b.idx_cap, b.val_cap, b.d_count);
        if (rc) return rc;
        if (b.n && !d_residuals[i]) return fail(STG_ERR_INVALID, "null residual");
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool fused = h->method == M_TV16;
    int rc;
    if (fused) {
        if ((rc = run_tv16(h, buckets, nbuckets, s, d_residuals))) return rc;
    } else {
        for (size_t i = 0; i < nbuckets; ++i) {
            const stg_bucket_t &b = buckets[i];
            if ((rc = run_device(h, b.key, b.d_src, b.d_src, b.n, b.k, b.d_idx, b.idx_cap, b.d_val, b.val_cap,
                                 b.idx_offset, b.d_count, s)))
                return rc;
        }
    }
    for (size_t i = 0; i < nbuckets; ++i)
        if (buckets[i].n && (rc = ef_after(h, buckets[i], d_residuals[i], fused, s))) return rc;
    return STG_OK;
}

int stg_codec_compress_wire_batch_device(stg_codec_t h, const stg_bucket_t *buckets, const int *flags,
                                         size_t nbuckets, void *stream) {
    CritPath crit_path;
    if (!h) return fail(STG_ERR_INVALID, "null codec handle");
    if (nbuckets && (!buckets || !flags)) return fail(STG_ERR_INVALID, "null bucket or flag array");
    if (h->method != M_TV16)
        return fail(STG_ERR_UNSUPPORTED, "wire-form emission is fused into thresholdv16 only "
                                         "(compress, then stg_wire_encode_device)");
    for (size_t i = 0; i < nbuckets; ++i) {
        const stg_bucket_t &b = buckets[i];
        const int rc = validate(h, b.n, b.k, b.idx_cap, b.val_cap, b.d_count);
        if (rc) return rc;
        if (flags[i] & ~3) return fail(STG_ERR_INVALID, "unknown wire flag bits");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // One bucket of 16-64 MiB: the one-bucket launch with its in-scan finish
    // (tv16lf2.h, which has no wire instance) into the workspace's staging,
    // then the separate packing -- 30.9 against 35.5 us fused for 64 MiB fp16
    // (profiles/r05_bench_configs_end.jsonl).
    if (nbuckets == 1 && flags[0] && buckets[0].n >= (size_t(1) << 22) &&
        buckets[0].n <= (size_t(1) << 24)) {
        const stg_bucket_t &b = buckets[0];
        HIP_TRY(hipSetDevice(h->device));
        Workspace *ws = nullptr;
        int rc = h->workspace(s, &ws);
        if (rc) return rc;
        stg_bucket_t t = b;
        // staging of its own, held for the whole sequence: another thread on
        // this stream cannot grow (free) it between the compress and the packing
        std::lock_guard<std::mutex> g(ws->wire_mu);
        if ((rc = ws->ensure_wire_stage(std::max<size_t>(b.idx_cap, 1)))) return rc;
        t.d_idx = ws->wst_pos.get();
        t.d_val = ws->wst_val.get();
        t.val_cap = t.idx_cap;
        if ((rc = run_tv16(h, &t, 1, s))) return rc;
        const size_t numel = std::min<size_t>(b.idx_cap, b.n);  // the pairs the fill writes
        HIP_TRY(stg::launch_wire_encode(t.d_idx, t.d_val, numel, (uint32_t)flags[0], b.d_idx, b.d_val, h->num_cu, s));
        return STG_OK;
    }
    return run_tv16(h, buckets, nbuckets, s, nullptr, nullptr, flags);
}

int stg_merge_gather_compress_device(stg_codec_t h, const stg_bucket_t *bucket, float *d_residual,
                                     const float *const *d_grads, int num_gpus, void *stream) {
    if (!h || !bucket) return fail(STG_ERR_INVALID, "null codec or bucket");
    if (num_gpus < 1 || num_gpus > (int)stg::GATHER_MAX) return fail(STG_ERR_INVALID, "num_gpus must be in [1, 16]");
    if (num_gpus > 1 && !d_grads) return fail(STG_ERR_INVALID, "null d_grads");
    for (int i = 1; i < num_gpus; ++i)
        if (bucket->n && !d_grads[i]) return fail(STG_ERR_INVALID, "null source");
    const stg_bucket_t &b = *bucket;
    int rc = validate(h, b.n, b.k, b.idx_cap, b.val_cap, b.d_count);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(h->device));
    const stg::GatherArgs g = gather_args(const_cast<float *>(b.d_src), d_residual, d_grads, num_gpus);
    if (h->method == M_TV16 && b.n) {
        float *res[1] = {d_residual};
        if ((rc = run_tv16(h, &b, 1, s, d_residual ? res : nullptr, &g))) return rc;
        return d_residual ? ef_after(h, b, d_residual, true, s) : STG_OK;
    }
    // the other codecs: the gather-add pass, then the task as without it
    HIP_TRY(stg::launch_gather_add(g, 0, b.n, h->num_cu, s));
    if (d_residual) return stg_merge_compress_batch_device(h, &b, &d_residual, 1, stream);
    return run_device(h, b.key, b.d_src, b.d_src, b.n, b.k, b.d_idx, b.idx_cap, b.d_val, b.val_cap, b.idx_offset,
                      b.d_count, s);
}

int stg_merge_gather_compress_typed_device(stg_codec_t h, const stg_bucket_t *bucket, float *d_residual,
                                           const stg_grad_src_t *srcs, int num_gpus, void *stream) {
    if (!h || !bucket) return fail(STG_ERR_INVALID, "null codec or bucket");
    if (num_gpus < 1 || num_gpus > (int)stg::GATHER_MAX) return fail(STG_ERR_INVALID, "num_gpus must be in [1, 16]");
    const stg_bucket_t &b = *bucket;
    stg::GatherArgs g;
    bool typed;
    std::string why;
    int rc = typed_gather_args(const_cast<float *>(b.d_src), d_residual, srcs, num_gpus, b.n, &g, &typed, &why);
    if (rc) return fail(rc, why);
    if (!typed) {  // fp32 in place: the fp32 entry point, its launchers and the in-scan gather
        const float *f32[stg::GATHER_MAX] = {};
        for (int i = 1; i < num_gpus; ++i) f32[i] = static_cast<const float *>(g.src[i]);
        return stg_merge_gather_compress_device(h, bucket, d_residual, f32, num_gpus, stream);
    }
    if ((rc = validate(h, b.n, b.k, b.idx_cap, b.val_cap, b.d_count))) return rc;
    if (b.n && !b.d_src) return fail(STG_ERR_INVALID, "null bucket buffer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(h->device));
    // the typed gather-add pass, then the task as without a gather (thresholdv16: the plain scan)
    HIP_TRY(stg::launch_gather_add_typed(g, 0, b.n, h->num_cu, s));
    if (d_residual) return stg_merge_compress_batch_device(h, &b, &d_residual, 1, stream);
    return run_device(h, b.key, b.d_src, b.d_src, b.n, b.k, b.d_idx, b.idx_cap, b.d_val, b.val_cap, b.idx_offset,
                      b.d_count, s);
}

// the layout include/stg/codec.h documents (and stellatrain_amd/_capi.py mirrors)
static_assert(sizeof(stg_grad_src_t) == 16 && offsetof(stg_grad_src_t, dtype) == 8, "stg_grad_src_t layout");
static_assert(sizeof(stg_bucket_t) == 80 && offsetof(stg_bucket_t, d_count) == 72, "stg_bucket_t layout");
static_assert(sizeof(stg_send_task_t) == 104 && offsetof(stg_send_task_t, d_residual) == 80 &&
                  offsetof(stg_send_task_t, d_grads) == 88 && offsetof(stg_send_task_t, num_gpus) == 96 &&
                  offsetof(stg_send_task_t, wire_flag) == 100,
              "stg_send_task_t layout");

// stg_merge_send_batch_device (srcs null) and stg_merge_send_batch_typed_device:
// task i gathers from srcs[i] when srcs and srcs[i] are given, else from its
// fp32 d_grads.  A call none of whose tasks has a 16-bit source or a typed first
// term takes the fp32 launchers exactly as before.
static int send_batch(stg_codec_t h, const stg_send_task_t *tasks, const stg_grad_src_t *const *srcs, size_t ntasks,
                      void *stream) {
    CritPath crit_path;
    if (!h) return fail(STG_ERR_INVALID, "null codec handle");
    if (ntasks && !tasks) return fail(STG_ERR_INVALID, "null task array");
    if (h->method == M_TOPK)
        return fail(STG_ERR_UNSUPPORTED, "the one-call send path takes thresholdv16, thresholdv or topk_exact: the "
                                         "shipped top-k writes idx[i] = i, so its selected entries have no true "
                                         "indices to zero (gather-compress, then stg_wire_encode_device)");
    // all or nothing: every task is checked before any device call or key state exists
    auto tfail = [](size_t i, int code, const std::string &msg) {
        return fail(code, "task " + std::to_string(i) + ": " + msg);
    };
    std::unordered_map<std::string, size_t> seen;
    size_t live = 0, one = 0;  // tasks with n > 0; the last of them
    std::vector<stg::GatherArgs> typed_g(srcs ? ntasks : 0);  // the gathers of the tasks with srcs[i]
    bool any_typed = false;
    for (size_t i = 0; i < ntasks; ++i) {
        const stg_send_task_t &t = tasks[i];
        const stg_bucket_t &b = t.bucket;
        const int rc = validate(h, b.n, b.k, b.idx_cap, b.val_cap, b.d_count);
        if (rc) return tfail(i, rc, std::string(g_err));
        if (t.wire_flag & ~3) return tfail(i, STG_ERR_INVALID, "unknown wire flag bits");
        if (t.num_gpus < 1 || t.num_gpus > (int)stg::GATHER_MAX)
            return tfail(i, STG_ERR_INVALID, "num_gpus must be in [1, 16]");
        const stg_grad_src_t *ts = srcs ? srcs[i] : nullptr;
        if (ts) {
            bool typed;
            std::string why;
            const int rc = typed_gather_args(const_cast<float *>(b.d_src), t.d_residual, ts, t.num_gpus, b.n,
                                             &typed_g[i], &typed, &why);
            if (rc) return tfail(i, rc, why);
            any_typed |= typed && b.n;
        }
        if (b.n) {
            if (!b.d_src || (b.idx_cap && (!b.d_idx || !b.d_val))) return tfail(i, STG_ERR_INVALID, "null bucket buffer");
            if (!ts) {
                if (t.num_gpus > 1 && !t.d_grads) return tfail(i, STG_ERR_INVALID, "null d_grads");
                for (int r = 1; r < t.num_gpus; ++r)
                    if (!t.d_grads[r]) return tfail(i, STG_ERR_INVALID, "null source");
            }
            ++live;
            one = i;
        }
        if (h->method == M_TV && !b.n) continue;  // (keyed by the bucket's pointer: an empty task has no key)
        const auto ins = seen.emplace(state_key(h->method, b.key, b.d_src), i);
        if (!ins.second)
            return tfail(i, STG_ERR_INVALID, "key repeats task " + std::to_string(ins.first->second) +
                                                 "'s (one task per key per call)");
    }
    if (!ntasks) return STG_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(h->device));
    Workspace *ws = nullptr;
    int rc = h->workspace(s, &ws);
    if (rc) return rc;
    // The scans write u32 / f32 pairs into staging, sized before the first
    // launch and held for the whole call: it never moves between a task's scan
    // and its finish.  Slices start on 256 bytes (the emission stores 16 bytes).
    std::lock_guard<std::mutex> wg(ws->wire_mu);
    auto slice = [](size_t cap) { return (cap + 63) / 64 * 64; };
    size_t total = 0;
    for (size_t i = 0; i < ntasks; ++i)
        if (tasks[i].bucket.n) total += slice(tasks[i].bucket.idx_cap);
    if ((rc = ws->ensure_wire_stage(std::max<size_t>(total, 1)))) return rc;
    std::vector<stg_bucket_t> bk(ntasks);
    std::vector<float *> res(ntasks);
    size_t off = 0;
    for (size_t i = 0; i < ntasks; ++i) {
        bk[i] = tasks[i].bucket;
        res[i] = tasks[i].d_residual;
        if (!bk[i].n) continue;  // (run_tv16 writes its zero count)
        bk[i].d_idx = ws->wst_pos.get() + off;
        bk[i].d_val = ws->wst_val.get() + off;
        bk[i].val_cap = bk[i].idx_cap;
        off += slice(bk[i].idx_cap);
    }
    auto gather_of = [&](size_t i) {
        const stg_send_task_t &t = tasks[i];
        if (srcs && srcs[i]) return typed_g[i];
        return gather_args(const_cast<float *>(t.bucket.d_src), t.d_residual, t.d_grads, t.num_gpus);
    };
    // One task of 16-64 MiB alone: the one-bucket scan sums the sources in its
    // own streaming pass (tv16lone.hip), one pass over the bucket instead of two.
    // That pass reads fp32 sources only: with a 16-bit source or a typed first
    // term the typed gather-add runs first, then the plain scan (the same bits).
    // (thresholdv16's: a threshold-v or top-k task always takes the gather launches below)
    const bool tv = h->method == M_TV, topk = h->method == M_TOPK_EXACT;
    const bool lone = !tv && !topk && live == 1 && tasks[one].bucket.n >= (size_t(1) << 22) &&
                      tasks[one].bucket.n <= (size_t(1) << 24);
    // the scans (top-k: the selects) of the call, after its gather launches
    auto scan = [&]() {
        if (topk) return run_topk_send(h, ws, bk.data(), res.data(), ntasks, s);
        return tv ? run_tv_send(h, ws, bk.data(), res.data(), ntasks, s) : run_tv16(h, bk.data(), ntasks, s, res.data());
    };
    if (lone && any_typed) {
        HIP_TRY(stg::launch_gather_add_typed(gather_of(one), 0, tasks[one].bucket.n, h->num_cu, s));
        if ((rc = run_tv16(h, bk.data(), ntasks, s, res.data()))) return rc;
    } else if (lone) {
        const stg::GatherArgs g = gather_of(one);
        if ((rc = run_tv16(h, bk.data(), ntasks, s, res.data(), &g, nullptr, one))) return rc;
    } else if (any_typed) {
        // the typed table for the whole call (an fp32 task is type 0 throughout): as many launches as below
        auto gb = stream_packer<stg::SendGatherBatch>((uint64_t)h->num_cu * 8, stg::launch_gather_add_batch_typed, s);
        for (size_t i = 0; i < ntasks; ++i) {
            const size_t n = tasks[i].bucket.n;
            if (!n) continue;
            const stg::GatherArgs g = gather_of(i);
            if (!g.resid && g.nsrc <= 1 && !g.src[0]) continue;  // (no term to add)
            const stg::GatherPlan p = stg::gather_plan_of(g, 0, n);
            stg::SendGather *d;
            if ((rc = gb.add(stg::send_gather_blocks(n, p), &d))) return rc;
            d->dst = g.dst;
            d->resid = g.resid;
            for (uint32_t r = 0; r < g.nsrc; ++r) d->src[r] = g.src[r];
            d->n = n;
            d->nsrc = g.nsrc;
            d->vec = p.width;
            d->head = p.head;
            d->dtypes = g.dtypes;
        }
        if ((rc = gb.flush())) return rc;
        if ((rc = scan())) return rc;
    } else {
        // gather groups: a launch closes at SEND_BATCH tasks or before its grid
        // would pass num_cu * 8 workgroups (a larger tensor runs alone)
        auto gb = stream_packer<stg::SendGatherBatch>((uint64_t)h->num_cu * 8, stg::launch_gather_add_batch, s);
        for (size_t i = 0; i < ntasks; ++i) {
            const stg_send_task_t &t = tasks[i];
            const size_t n = t.bucket.n;
            if (!n || (!t.d_residual && t.num_gpus <= 1)) continue;  // (no term to add)
            const stg::GatherArgs g = gather_of(i);
            auto phase = [](const void *p) { return reinterpret_cast<uintptr_t>(p) & 15u; };
            const uintptr_t ph = phase(g.dst);
            bool vec = (ph & 3u) == 0;
            if (g.resid) vec &= phase(g.resid) == ph;
            for (uint32_t r = 1; r < g.nsrc; ++r) vec &= phase(g.src[r]) == ph;
            const size_t head = vec ? std::min<size_t>(n, ((16u - ph) & 15u) / 4u) : 0;
            const uint64_t nbk = vec ? std::max<uint64_t>(1, ((n - head) / 4 + stg::SEND_GATHER_TILE / 4 - 1) /
                                                                 (stg::SEND_GATHER_TILE / 4))
                                     : (n + stg::SEND_GATHER_TILE - 1) / stg::SEND_GATHER_TILE;
            stg::SendGather *d;
            if ((rc = gb.add(nbk, &d))) return rc;
            d->dst = g.dst;
            d->resid = g.resid;
            for (uint32_t r = 1; r < g.nsrc; ++r) d->src[r] = g.src[r];
            d->n = n;
            d->nsrc = g.nsrc;
            d->vec = vec;
            d->head = (uint32_t)head;
        }
        if ((rc = gb.flush())) return rc;
        if ((rc = scan())) return rc;
    }
    if (tv) {
        // finish groups: every slot's wire form by the device count, error feedback by the true indices
        auto fd = stream_packer<stg::SendFinishDcBatch>(GRID_MAX, stg::launch_ef_pack_batch_dc, s);
        for (size_t i = 0; i < ntasks; ++i) {
            const stg_bucket_t &b = tasks[i].bucket;
            const size_t slots = std::min<size_t>(b.idx_cap, b.n);  // the slots the engine sends
            if (!slots) continue;
            stg::SendFinishDc *d;
            if ((rc = fd.add((slots + STG_WG - 1) / STG_WG, &d))) return rc;
            d->idx = bk[i].d_idx;
            d->val = bk[i].d_val;
            d->count = b.d_count;
            d->idx_out = b.d_idx;
            d->val_out = b.d_val;
            d->grad = const_cast<float *>(b.d_src);
            d->resid = tasks[i].d_residual;
            d->n = b.n;
            d->slots = (uint32_t)slots;
            d->flag = (uint32_t)tasks[i].wire_flag;
        }
        return fd.flush();
    }
    // finish groups: tail copy, error feedback by the true indices, wire form
    auto fb = stream_packer<stg::SendFinishBatch>(GRID_MAX, stg::launch_ef_pack_batch, s);
    for (size_t i = 0; i < ntasks; ++i) {
        const stg_bucket_t &b = tasks[i].bucket;
        if (!b.n) continue;
        const size_t count = std::min<size_t>(b.idx_cap, b.n);  // the pairs the fill writes
        if (!count && !tasks[i].d_residual) continue;
        const uint64_t nbk = std::max<uint64_t>(1, (count + STG_WG - 1) / STG_WG);
        stg::SendFinish *d;
        if ((rc = fb.add(nbk, &d))) return rc;
        d->idx = bk[i].d_idx;
        d->val = bk[i].d_val;
        d->idx_out = b.d_idx;
        d->val_out = b.d_val;
        d->grad = const_cast<float *>(b.d_src);
        d->resid = tasks[i].d_residual;
        d->n = b.n;
        d->count = (uint32_t)count;
        d->flag = (uint32_t)tasks[i].wire_flag;
        d->zero0 = b.idx_cap > count;
    }
    return fb.flush();
}

int stg_merge_send_batch_device(stg_codec_t h, const stg_send_task_t *tasks, size_t ntasks, void *stream) {
    return send_batch(h, tasks, nullptr, ntasks, stream);
}

int stg_merge_send_batch_typed_device(stg_codec_t h, const stg_send_task_t *tasks,
                                      const stg_grad_src_t *const *srcs, size_t ntasks, void *stream) {
    return send_batch(h, tasks, srcs, ntasks, stream);
}

int stg_codec_compress_host(stg_codec_t h, const char *key, const float *src, size_t n, uint32_t k,
                            uint32_t *dst_idx, size_t idx_cap, float *dst_val, size_t val_cap, int32_t idx_offset,
                            size_t *out_count) {
    CritPath crit_path;
    if (!h || !out_count) return fail(STG_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s;
    int rc = thread_stream(h->device, &s);
    if (rc) return rc;
    Workspace *ws = nullptr;
    if ((rc = h->workspace(s, &ws))) return rc;
    {
        std::lock_guard<std::mutex> g(ws->mu);
        HIP_TRY(ws->h_src.reserve(std::max<size_t>(n, 1), s, false));
        HIP_TRY(ws->h_idx.reserve(std::max<size_t>(idx_cap, 1), s, false));
        HIP_TRY(ws->h_val.reserve(std::max<size_t>(idx_cap, 1), s, false));
        HIP_TRY(ws->h_count.reserve(1, s, false));
        if (!ws->pinned_count) HIP_TRY(hipHostMalloc(&ws->pinned_count, 2 * sizeof(uint32_t)));
        if (n) HIP_TRY(hipMemcpyAsync(ws->h_src.get(), src, n * sizeof(float), hipMemcpyHostToDevice, s));
    }
    // threshold-v keys its state by the caller's (host) src pointer
    rc = run_device(h, key, ws->h_src.get(), src, n, k, ws->h_idx.get(), idx_cap, ws->h_val.get(), idx_cap, idx_offset,
                    ws->h_count.get(), s);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(ws->mu);
    HIP_TRY(hipMemcpyAsync(ws->pinned_count, ws->h_count.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (idx_cap) {
        HIP_TRY(hipMemcpyAsync(dst_idx, ws->h_idx.get(), idx_cap * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(dst_val, ws->h_val.get(), std::min(idx_cap, val_cap) * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    // the workspace's sticky failure word rides along: a device-side failure
    // (a bounded wait that gave up) is an error, never a silent wrong result
    HIP_TRY(hipMemcpyAsync(ws->pinned_count + 1, ws->d.fail, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (ws->pinned_count[1]) {
        char b[96];
        snprintf(b, sizeof b, "device failure flags 0x%x (details: stg_codec_check)", ws->pinned_count[1]);
        return fail(STG_ERR_DEVICE, b);
    }
    *out_count = *ws->pinned_count;
    return STG_OK;
}

int stg_codec_get_state(stg_codec_t h, const char *key, const void *key_ptr, float *threshold, float *threshold_inc,
                        void *stream) {
    if (!h) return fail(STG_ERR_INVALID, "null codec handle");
    HIP_TRY(hipSetDevice(h->device));
    KeyState *st = nullptr;
    {
        std::lock_guard<std::mutex> g(h->mu);
        auto it = h->slot_of.find(state_key(h->method, key, key_ptr));
        if (it == h->slot_of.end()) return fail(STG_ERR_INVALID, "key has no state yet");
        st = h->slot_ptr(it->second);
    }
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    KeyState hs;
    HIP_TRY(hipMemcpy(&hs, st, sizeof hs, hipMemcpyDeviceToHost));
    if (threshold) *threshold = hs.t;
    if (threshold_inc) *threshold_inc = hs.inc;
    return STG_OK;
}

int stg_codec_set_timing(stg_codec_t h, int enable) {
    if (!h) return fail(STG_ERR_INVALID, "null codec handle");
    std::lock_guard<std::mutex> g(h->mu);
    h->timing = enable != 0;
    return STG_OK;
}

int stg_codec_get_timing(stg_codec_t h, double *ms3, uint64_t *calls) {
    if (!h || !ms3 || !calls) return fail(STG_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> g(h->mu);
    for (auto &e : h->ev_pending) {
        HIP_TRY(hipEventSynchronize(e[2]));
        float a = 0, b = 0, c = 0;
        HIP_TRY(hipEventElapsedTime(&a, e[0], e[1]));
        HIP_TRY(hipEventElapsedTime(&b, e[1], e[2]));
        HIP_TRY(hipEventElapsedTime(&c, e[0], e[2]));
        h->ms_acc[0] += a;
        h->ms_acc[1] += b;
        h->ms_acc[2] += c;
        h->timed_calls++;
        h->ev_pool.push_back(e);
    }
    h->ev_pending.clear();
    for (int i = 0; i < 3; ++i) { ms3[i] = h->ms_acc[i]; h->ms_acc[i] = 0; }
    *calls = h->timed_calls;
    h->timed_calls = 0;
    return STG_OK;
}

int stg_codec_check(stg_codec_t h) {
    if (!h) return fail(STG_ERR_INVALID, "null codec handle");
    HIP_TRY(hipSetDevice(h->device));
    std::lock_guard<std::mutex> g(h->mu);
    for (auto &kv : h->ws) {
        HIP_TRY(hipStreamSynchronize(kv.first));
        uint32_t f[48] = {};
        HIP_TRY(hipMemcpy(f, kv.second->d.fail, sizeof f, hipMemcpyDeviceToHost));
        if (f[0]) {
            std::string m = "device failure flags 0x";
            char b[160];
            snprintf(b, sizeof b, "%x", f[0]);
            m += b;
            if (f[1]) {  // spin-timeout records (tv16.hip Ctx::spin_fail)
                snprintf(b, sizeof b, " (first spin timeout: site %u, workgroup %u, %u %u %u, epoch %u)", f[1] - 1, f[2],
                         f[3], f[4], f[5], f[6]);
                m += b;
                for (uint32_t site = 0; site < 10; ++site) {
                    const uint32_t *r = f + 8 + 4 * site;
                    if (!r[0]) continue;
                    snprintf(b, sizeof b, " [site %u: wg %u, %u %u %u]", site, r[0] - 1, r[1], r[2], r[3]);
                    m += b;
                }
            }
            return fail(STG_ERR_DEVICE, m);
        }
        // diagnostics (STG_DEBUG_TV16_COUNT): the scan's counters of this workspace
        if (stg::tv16_debug_count()) {
            uint32_t w[5] = {};
            HIP_TRY(hipMemcpy(w, kv.second->d.misc, sizeof w, hipMemcpyDeviceToHost));
            fprintf(stderr, "stg: tv16 scan counters, stream %p: launches %u, dead workgroups %u (most in one launch %u)\n",
                    (void *)kv.first, w[4], w[1], w[2]);
        }
    }
    return STG_OK;
}

int stg_debug_tv16_scan_grid(int num_cu, int streams, int hw_queues, uint32_t chunks) {
    if (num_cu < 1 || streams < 0 || hw_queues < 0) return 0;
    return (int)stg::tv16_scan_grid((uint32_t)num_cu, (uint32_t)streams, (uint32_t)hw_queues, chunks);
}

int stg_codec_debug_words(stg_codec_t h, void *stream, uint32_t *out, int n) {
    if (!h || !out || n < 0 || n > 64) return fail(STG_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    Workspace *ws = nullptr;
    int rc = h->workspace(s, &ws);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(out, ws->d.misc, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return STG_OK;
}

int stg_error_feedback_device(float *d_grad, size_t n, const uint32_t *d_idx, size_t numel, float *d_residual,
                              void *stream) {
    if ((n && (!d_grad || !d_residual)) || (numel && !d_idx)) return fail(STG_ERR_INVALID, "null argument");
    int ncu;
    if (const int rc = device_cus(&ncu)) return rc;
    HIP_TRY(stg::launch_error_feedback(d_grad, n, d_idx, numel, d_residual, ncu, static_cast<hipStream_t>(stream)));
    return STG_OK;
}

}  // extern "C"

namespace {

// One MERGE decompress call: the rank streams as the launcher takes them, built
// once at the C entry point, and the entry's other arguments.
struct MergeCall {
    std::vector<stg::RankStream> rs;  // `world` streams (none at a wire entry given world < 1 or a null array)
    bool wire;                        // a wire entry: the streams' flags and buffers are checked
    size_t per_rank;
    int world;
    size_t n;
    float *dense;
    uint8_t *mark;
    uint32_t *out_idx;
    float *out_val;
    uint32_t *out_count;
    void *stream;
};

// decoded pairs back to back: the wire form with flag 0
static std::vector<stg::RankStream> decoded_streams(const uint32_t *idx, const float *val, size_t per_rank,
                                                    int world) {
    std::vector<stg::RankStream> rs((size_t)std::max(world, 0));
    for (size_t r = 0; r < rs.size(); ++r) rs[r] = stg::RankStream{idx + r * per_rank, val + r * per_rank, 0u};
    return rs;
}

static std::vector<stg::RankStream> wire_streams(const stg_rank_stream_t *ranks, int world) {
    std::vector<stg::RankStream> rs(ranks ? (size_t)std::max(world, 0) : 0);
    for (size_t r = 0; r < rs.size(); ++r)
        rs[r] = stg::RankStream{ranks[r].d_idx, ranks[r].d_val, (uint32_t)ranks[r].flag};
    return rs;
}

// The argument checks of every MERGE entry, none of which needs a device.
static int merge_check(const MergeCall &c) {
    if (c.world < 1) return fail(STG_ERR_INVALID, "world must be >= 1");
    if (c.wire) {
        if (c.rs.empty()) return fail(STG_ERR_INVALID, "null rank stream array");
        for (const stg::RankStream &k : c.rs) {
            if (k.flag & ~(uint32_t)(STG_WIRE_U16_IDX | STG_WIRE_F16_VAL))
                return fail(STG_ERR_INVALID, "unknown wire flag bits in a rank stream");
            if (c.per_rank && (!k.idx || !k.val)) return fail(STG_ERR_INVALID, "null rank stream buffer");
            // a 16-bit buffer needs its 2-byte alignment, a 32-bit one its 4-byte alignment
            if ((reinterpret_cast<uintptr_t>(k.idx) & (k.flag & STG_WIRE_U16_IDX ? 1u : 3u)) ||
                (reinterpret_cast<uintptr_t>(k.val) & (k.flag & STG_WIRE_F16_VAL ? 1u : 3u)))
                return fail(STG_ERR_INVALID, "rank stream buffer misaligned for its element type");
        }
    }
    if (c.world > 1 && (!c.dense || !c.mark)) return fail(STG_ERR_INVALID, "dense/mark scratch required for world > 1");
    if (c.world > 1 && (reinterpret_cast<uintptr_t>(c.mark) & 15u)) return fail(STG_ERR_INVALID, "mark scratch must be 16-byte aligned");
    // the emission reads and zeroes a lane's 16 dense floats as four float4
    if (c.world > 1 && (reinterpret_cast<uintptr_t>(c.dense) & 15u)) return fail(STG_ERR_INVALID, "dense scratch must be 16-byte aligned");
    return STG_OK;
}

// The sizes every launch path can index (uint32 indices and positions).
static int merge_size_check(const MergeCall &c) {
    if (c.n >= (size_t(1) << 32) || c.per_rank >= (size_t(1) << 32))
        return fail(STG_ERR_UNSUPPORTED, "more than 2^32-1 elements (uint32 indices)");
    return STG_OK;
}

// merge_run on a scratch the caller has looked up and locked (ms->mu held; the
// scratch of the current device and c.stream): size it, tag the call, launch.
static int merge_run_locked(const MergeCall &c, MergeScratch *ms, int ncu, const stg::SgdLaunch *sgd,
                            const stg::AdamLaunch *adam, uint64_t *launches = nullptr) {
    hipStream_t s = static_cast<hipStream_t>(c.stream);
    int rc = merge_scratch_ensure(ms, s, c.n, c.per_rank, c.world);
    if (rc) return rc;
    if (++ms->tag == 0) ms->tag = 1;
    const stg::Win1Desc w1{ms->desc.get(), ms->ticket.get(), ms->tag, ms->fail.get(),
                           reinterpret_cast<uint32_t *>(ms->ticket.get() + 1), sgd, adam};
    HIP_TRY(stg::launch_scatter_merge(c.rs.data(), c.per_rank, c.world, c.n, c.dense, c.mark, c.out_idx, c.out_val,
                                      c.out_count, ms->tiles.get(), ms->win.get(), ncu, s, w1, launches));
    return STG_OK;
}

// A checked call on the current device's (device, stream) scratch: look it up,
// lock, size it, tag the call, launch -- with the optimizer step `sgd` or
// `adam` (at most one; world 1 only) fused into the emission.
static int merge_run(const MergeCall &c, const stg::SgdLaunch *sgd = nullptr, const stg::AdamLaunch *adam = nullptr) {
    int rc = merge_size_check(c);
    if (rc) return rc;
    int dev, ncu;
    if ((rc = device_cus(&ncu, &dev))) return rc;
    const std::shared_ptr<MergeScratch> ms = merge_scratch(dev, static_cast<hipStream_t>(c.stream));
    std::lock_guard<std::mutex> g(ms->mu);
    return merge_run_locked(c, ms.get(), ncu, sgd, adam);
}

static int scatter_merge(const MergeCall &c) {
    int rc = merge_check(c);
    return rc ? rc : merge_run(c);
}

// The fused world-1 step's own limits (per_rank > 0 here).
static int merge_fused_limits(const MergeCall &c, uint32_t param_len) {
    if (c.per_rank >= (size_t(1) << 32) || param_len == 0)
        return fail(STG_ERR_UNSUPPORTED, "more than 2^32-1 elements or an empty parameter");
    return STG_OK;
}

// A name's buffer of an SGD handle (momentum, last-touched words) read back once
// the stream's work is done.
template <typename T>
static int sgd_read_back(stg_sgd_t o, const std::unordered_map<std::string, stg_sgd::Named<T>> &of, const char *name,
                         T *host_out, uint32_t len, void *stream, const char *missing) {
    HIP_TRY(hipSetDevice(o->device));
    T *b = nullptr;
    uint32_t n = 0;
    {
        std::lock_guard<std::mutex> g(o->mu);
        auto it = of.find(name);
        if (it == of.end()) return fail(STG_ERR_INVALID, missing);
        b = it->second.buf.get();
        n = it->second.len;
    }
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    HIP_TRY(hipMemcpy(host_out, b, std::min(len, n) * sizeof(T), hipMemcpyDeviceToHost));
    return STG_OK;
}

// ---- the two optimizers' policies ----
// What SGD and Adam differ in at every entry that steps: the handle's state of a
// name, whether the step fuses into a world-1 emission, the launch, and the
// fields a tensor of a batched launch carries.
struct SgdBatch {
    using Handle = stg_sgd_t;
    using Launch = stg::SgdLaunch;
    static bool fuses(Handle) { return true; }
    static int refuse(Handle, uint32_t, uint32_t) { return STG_OK; }
    static uint32_t step_cap(Handle, uint32_t) { return 0xffffffffu; }
    static bool len_checked(Handle o) { return o->smart; }  // only the last-touched array pins a name's length
    static int len_check(Handle o, const char *name, uint32_t param_len) {
        auto it = o->last.find(name);
        if (it != o->last.end() && it->second.len != param_len)
            return fail(STG_ERR_INVALID, "param_len differs from the name's first smart-momentum call");
        return STG_OK;
    }
    // One optimize_raw call's launch arguments (the momentum buffer of `name`,
    // created zeroed on its first call: sgd.cpp:40-47; the iteration count).
    // Caller holds o->mu.
    static int prepare_locked(Handle o, const char *name, float *d_param, uint32_t param_len, hipStream_t s,
                              Launch *out) {
        bool first = false;
        float *mom = nullptr;
        uint32_t *last = nullptr;
        uint32_t iter;
        if (o->smart) {  // the reference's array is zero until the option is on (sgd.cpp:46-47, 258-259)
            auto it = o->last.find(name);
            if (it == o->last.end()) {
                stg_sgd::Named<uint32_t> b;
                HIP_TRY(b.buf.reserve(std::max<size_t>(param_len, 1), s, true));
                b.len = param_len;
                it = o->last.emplace(name, std::move(b)).first;
            }
            if (it->second.len != param_len)
                return fail(STG_ERR_INVALID, "param_len differs from the name's first smart-momentum call");
            last = it->second.buf.get();
        }
        iter = o->iter;
        if (o->momentum != 0.f) {
            auto it = o->mom.find(name);
            if (it == o->mom.end()) {  // sgd.cpp:40-47: zeroed buffer, first = true
                stg_sgd::Named<float> b;
                HIP_TRY(b.buf.reserve(std::max<size_t>(param_len, 1), s, true));
                b.len = param_len;
                it = o->mom.emplace(name, std::move(b)).first;
                first = true;
            }
            mom = it->second.buf.get();
        }
        o->iter++;  // sgd.cpp:262
        stg::SgdLaunch a{};
        a.param = d_param;
        a.param_len = param_len;
        a.mom = mom;
        a.first = first;
        a.momentum = o->momentum;
        a.dampening = o->dampening;
        a.weight_decay = o->weight_decay;
        a.lr = o->maximize ? -(double)o->lr : (double)o->lr;  // sgd.cpp:51
        a.nesterov = o->nesterov;
        a.last = last;
        a.iter = iter;
        a.pow_tab = o->pow_tab.get();
        a.pow_len = (uint32_t)o->pow_tab.cap();
        a.fail = o->fail.get();
        *out = a;
        return STG_OK;
    }
    static hipError_t launch(const Launch &a, hipStream_t s, uint64_t *n) { return stg::launch_sgd(a, s, n); }
    static const stg::SgdLaunch *sgd(const Launch *a) { return a; }
    static const stg::AdamLaunch *adam(const Launch *) { return nullptr; }
    static int opt(const Launch &a) { return a.last ? 1 : 0; }
    template <class W>
    static void common(const Launch &a, W &w) { w.sgd = a; }
    template <class D>
    static void fill(const Launch &a, D &d) {
        d.s0 = a.mom;
        d.s1 = a.last;
        d.u.sgd.iter = a.iter;
        d.u.sgd.first = a.first;
    }
};

struct AdamBatch {
    using Handle = stg_adam_t;
    using Launch = stg::AdamLaunch;
    static bool fuses(Handle o) { return !o->amsgrad; }  // amsgrad is never fused ...
    static int refuse(Handle o, uint32_t grad_len, uint32_t param_len) {
        if (o->amsgrad && grad_len > param_len)
            return fail(STG_ERR_INVALID, "amsgrad: grad_len > param_len (indices must be unique)");
        return STG_OK;
    }
    static uint32_t step_cap(Handle o, uint32_t param_len) { return o->amsgrad ? param_len : 0xffffffffu; }  // ... and caps the step's length
    static bool len_checked(Handle) { return true; }
    static int len_check(Handle o, const char *name, uint32_t param_len) {
        auto it = o->st.find(name);
        if (it != o->st.end() && it->second.len != param_len)
            return fail(STG_ERR_INVALID, "param_len differs from the name's first call");
        return STG_OK;
    }
    // One optimize_raw call's launch arguments: the name's state (created zeroed
    // on its first call: adam.cpp:28-35), its tick and the bias corrections.
    // Caller holds o->mu.
    static int prepare_locked(Handle o, const char *name, float *d_param, uint32_t param_len, hipStream_t s,
                              Launch *out) {
        stg::AdamLaunch a{};
        uint32_t tick;
        HIP_TRY(o->fail.reserve(1, s, true));  // the handle's failure word, allocated with its first state
        auto it = o->st.find(name);
        if (it == o->st.end()) {  // adam.cpp:28-35: zeroed m and v, vmax 0, tick 1
            stg_adam::Name nm;
            const size_t L = std::max<size_t>(param_len, 1);
            HIP_TRY(nm.mvv.reserve(2 * L + 1, s, true));
            if (o->amsgrad)  // one tagged uint64 per tile; zero never matches a tick (>= 1)
                HIP_TRY(nm.tiles.reserve((L + stg::ADAM_TILE - 1) / stg::ADAM_TILE, s, true));
            nm.len = param_len;
            it = o->st.emplace(name, std::move(nm)).first;
        }
        if (it->second.len != param_len) return fail(STG_ERR_INVALID, "param_len differs from the name's first call");
        a.m = it->second.m();
        a.v = it->second.v();
        a.vmax = it->second.vmax();
        a.tiles = reinterpret_cast<uint32_t *>(it->second.tiles.get());
        tick = it->second.tick++;  // adam.cpp:40,82
        a.param = d_param;
        a.param_len = param_len;
        a.b1 = o->b1;
        a.b2 = o->b2;
        a.eps = o->eps;
        a.weight_decay = o->weight_decay;
        a.lr = (double)o->lr;
        a.c1 = 1.0 - std::pow((double)o->b1, (double)tick);  // adam.cpp:42,67
        a.c2 = 1.0 - std::pow((double)o->b2, (double)tick);  // adam.cpp:43,68
        a.amsgrad = o->amsgrad;
        a.maximize = o->maximize;
        a.tag = tick;
        a.fail = o->fail.get();
        *out = a;
        return STG_OK;
    }
    static hipError_t launch(const Launch &a, hipStream_t s, uint64_t *n) { return stg::launch_adam(a, s, n); }
    static const stg::SgdLaunch *sgd(const Launch *) { return nullptr; }
    static const stg::AdamLaunch *adam(const Launch *a) { return a; }
    static int opt(const Launch &) { return 2; }
    template <class W>
    static void common(const Launch &a, W &w) { w.adam = a; }
    template <class D>
    static void fill(const Launch &a, D &d) {
        d.s0 = a.m;
        d.s1 = a.v;
        d.u.adam.c1 = a.c1;
        d.u.adam.c2 = a.c2;
    }
};

// The step of a prepared call over grad_len pairs at most (none: no launch).
template <class P>
static int step(typename P::Launch a, const float *d_grad, const uint32_t *d_idx, uint32_t grad_len,
                const uint32_t *d_grad_len, hipStream_t s, uint64_t *launches = nullptr) {
    a.grad = d_grad;
    a.gidx = d_idx;
    a.grad_len = grad_len;
    a.d_grad_len = d_grad_len;
    if (grad_len) HIP_TRY(P::launch(a, s, launches));
    return STG_OK;
}

// ... over a merge's output
template <class P>
static int merge_step(typename P::Handle o, const typename P::Launch &a, const MergeCall &c,
                      uint64_t *launches = nullptr) {
    const size_t cap = std::min<size_t>(c.per_rank * (size_t)c.world, P::step_cap(o, a.param_len));
    return step<P>(a, c.out_val, c.out_idx, (uint32_t)cap, c.out_count, static_cast<hipStream_t>(c.stream),
                   launches);
}

template <class P>
static int prepare(typename P::Handle o, const char *name, float *d_param, uint32_t param_len, hipStream_t s,
                   typename P::Launch *out) {
    std::lock_guard<std::mutex> g(o->mu);
    return P::prepare_locked(o, name, d_param, param_len, s, out);
}

// stg_*_optimize_raw_device
template <class P>
static int optimize_raw(typename P::Handle o, const char *name, float *d_param, uint32_t param_len,
                        const float *d_grad, const uint32_t *d_idx, uint32_t grad_len, const uint32_t *d_grad_len,
                        void *stream) {
    if (!o || !name) return fail(STG_ERR_INVALID, "null argument");
    int rc = P::refuse(o, grad_len, param_len);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(o->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    typename P::Launch a;
    if ((rc = prepare<P>(o, name, d_param, param_len, s, &a))) return rc;
    return step<P>(a, d_grad, d_idx, grad_len, d_grad_len, s);
}

// The MERGE decompress `c` over the parameter (c.n == param_len), then the step
// on its output -- or, where it can be fused, inside its emission.
template <class P>
static int merge_optimize(typename P::Handle o, const char *name, float *d_param, uint32_t param_len,
                          const MergeCall &c) {
    if (!o || !name) return fail(STG_ERR_INVALID, "null argument");
    int rc = merge_check(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(o->device));
    // world 1: the election, then the emission with every winner's step in the
    // same pass (each index is elected once, so the updates commute).  Otherwise
    // the merge (of several ranks) first, then the step over its output.
    const bool fused = c.world == 1 && c.per_rank != 0 && P::fuses(o);
    if ((rc = fused ? merge_fused_limits(c, param_len) : merge_run(c))) return rc;
    typename P::Launch a;
    if ((rc = prepare<P>(o, name, d_param, param_len, static_cast<hipStream_t>(c.stream), &a))) return rc;
    return fused ? merge_run(c, P::sgd(&a), P::adam(&a)) : merge_step<P>(o, a, c);
}

// ---- the iteration's ModuleCpuOptimize tasks in one call ----
// elements (the sum of its tensors' n) a world > 1 group may hold: two winner
// words each, so the winner words keep MERGE_BATCH_WIN_CAP
constexpr size_t GROUP_CAP = stg::MERGE_BATCH_WIN_CAP / 2;
template <class P>
static int merge_optimize_batch(typename P::Handle o, const stg_merge_task_t *tasks, size_t ntasks, void *stream) {
    if (!o) return fail(STG_ERR_INVALID, "null argument");
    if (!ntasks) return STG_OK;
    if (!tasks) return fail(STG_ERR_INVALID, "null task array");
    const auto refuse = [](size_t i, int rc) {
        g_err = "task " + std::to_string(i) + ": " + g_err;
        return rc;
    };
    // every check of every task, before any device call or state change
    std::vector<MergeCall> calls;
    calls.reserve(ntasks);
    // 0: the per-tensor sequence; 1: a world-1 launch pair; 2: a world > 1 group
    std::vector<uint8_t> fused(ntasks);
    for (size_t i = 0; i < ntasks; ++i) {
        const stg_merge_task_t &t = tasks[i];
        if (!t.name) return refuse(i, fail(STG_ERR_INVALID, "null name"));
        calls.push_back(MergeCall{wire_streams(t.ranks, t.world), true, t.per_rank, t.world, t.param_len, t.d_dense,
                                  t.d_mark, t.d_out_idx, t.d_out_val, t.d_out_count, stream});
        int rc = merge_check(calls[i]);
        if (t.per_rank > 0 && P::fuses(o))
            fused[i] = t.world == 1 ? 1 : t.param_len > 0 && t.param_len <= GROUP_CAP ? 2 : 0;
        if (!rc && fused[i] == 1) rc = merge_fused_limits(calls[i], t.param_len);
        if (!rc) rc = merge_size_check(calls[i]);
        if (rc) return refuse(i, rc);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<typename P::Launch> L(ntasks);
    {   // the batch's iterations and ticks, contiguous: task i prepares as the i-th call would
        std::lock_guard<std::mutex> g(o->mu);
        if (P::len_checked(o)) {
            std::unordered_map<std::string, uint32_t> seen;
            for (size_t i = 0; i < ntasks; ++i) {
                int rc = P::len_check(o, tasks[i].name, tasks[i].param_len);
                const auto ins = seen.emplace(tasks[i].name, tasks[i].param_len);
                if (!rc && ins.first->second != tasks[i].param_len)
                    rc = fail(STG_ERR_INVALID, "param_len differs from an earlier task of the same name");
                if (rc) return refuse(i, rc);
            }
        }
        HIP_TRY(hipSetDevice(o->device));
        for (size_t i = 0; i < ntasks; ++i) {
            const int rc = P::prepare_locked(o, tasks[i].name, tasks[i].d_param, tasks[i].param_len, s, &L[i]);
            if (rc) return refuse(i, rc);  // a HIP failure: the tasks before it keep their iterations
        }
    }
    int dev, ncu;
    if (const int rc = device_cus(&ncu, &dev)) return rc;
    const std::shared_ptr<MergeScratch> ms = merge_scratch(dev, s);
    std::lock_guard<std::mutex> g(ms->mu);
    uint64_t *const launches = &ms->launches;
    // the pending launch: tasks [g0, g0 + its count), `sum_n` winner words so far
    size_t g0 = 0, sum_n = 0;
    auto pk = stg::make_packer<stg::MergeBatchArgs>(~uint64_t(0), [&](stg::MergeBatchArgs &w, uint32_t blocks) -> int {
        const int rc = merge_scratch_ensure(ms.get(), s, sum_n, 0, 1, blocks);
        sum_n = 0;
        if (rc) return rc;
        if (++ms->tag == 0) ms->tag = 1;
        w.tag = ms->tag;
        w.win = ms->win.get();
        w.desc = ms->desc.get();
        w.ctl = ms->bctl.get();
        w.fail = ms->fail.get();
        HIP_TRY(stg::launch_merge_batch(w, blocks, P::opt(L[g0]), s, launches));
        return STG_OK;
    });
    // the pending world > 1 group: tasks [w0, w0 + its count), all of one world;
    // `w_off` elements of dense / marks so far (slices MERGE_WORLD_ALIGN apart),
    // `w_n` the sum of its tensors' n
    size_t w0 = 0, w_off = 0, w_n = 0;
    auto pw = stg::make_packer<stg::MergeWorldArgs>(GRID_MAX, [&](stg::MergeWorldArgs &w, uint32_t blocks) -> int {
        const int world = tasks[w0].world;
        // two tile words per tile: the counts and their prefixes
        const int rc = merge_scratch_ensure(ms.get(), s, w_off, 0, world, 2 * (size_t)blocks, w_off);
        w_off = w_n = 0;
        if (rc) return rc;
        stg::MergeScatterArgs sc{};
        sc.nt = w.nt;
        sc.win = ms->win.get();
        sc.dense = ms->wdense.get();
        sc.mark = ms->wmark.get();
        uint64_t sblocks = 0;
        for (uint32_t q = 0; q < w.nt; ++q) {
            stg::MergeScatterTensor &d = sc.t[q];
            d.m = (uint32_t)tasks[w0 + q].per_rank;
            d.n = w.t[q].n;
            d.off = w.t[q].off;
            d.blk0 = (uint32_t)sblocks;
            sblocks += (2 * (uint64_t)d.m + STG_WG - 1) / STG_WG;  // < 2^25 each
        }
        for (int r = 0; r <= world; ++r) {  // one launch per rank, stream-ordered: the sum's rank order
            sc.rank = (uint32_t)r;
            for (uint32_t q = 0; q < w.nt; ++q) {
                const std::vector<stg::RankStream> &rs = calls[w0 + q].rs;
                stg::MergeScatterTensor &d = sc.t[q];
                d.sidx = r >= 1 ? rs[r - 1].idx : nullptr;
                d.sval = r >= 1 ? rs[r - 1].val : nullptr;
                d.sflag = r >= 1 ? rs[r - 1].flag : 0u;
                d.midx = r < world ? rs[r].idx : nullptr;
                d.mflag = r < world ? rs[r].flag : 0u;
            }
            HIP_TRY(stg::launch_merge_world_scatter(sc, (uint32_t)sblocks, s, launches));
        }
        w.world = (float)world;
        w.tiles = ms->tiles.get();
        w.dense = ms->wdense.get();
        w.mark = ms->wmark.get();
        HIP_TRY(stg::launch_merge_world_emit(w, blocks, P::opt(L[w0]), s, launches));
        return STG_OK;
    });
    for (size_t i = 0; i < ntasks; ++i) {
        const stg_merge_task_t &t = tasks[i];
        int rc;
        // a change of kind closes what is pending: the call's launches keep the tasks' order
        if (fused[i] != 1 && (rc = pk.flush())) return rc;
        if (fused[i] != 2 && (rc = pw.flush())) return rc;
        if (!fused[i]) {  // the per-tensor sequence at its place in the order
            if ((rc = merge_run_locked(calls[i], ms.get(), ncu, nullptr, nullptr, launches))) return rc;
            if ((rc = merge_step<P>(o, L[i], calls[i], launches))) return rc;
            continue;
        }
        if (fused[i] == 2) {
            // (the packer closes at MERGE_BATCH tensors; another world, the cap and a repeated name close here)
            bool close = pw.count() && (tasks[w0].world != t.world || w_n + t.param_len > GROUP_CAP);
            for (size_t q = w0; !close && q < w0 + pw.count(); ++q) close = strcmp(tasks[q].name, t.name) == 0;
            if (close && (rc = pw.flush())) return rc;
            stg::MergeWorldTensor *dp;
            if ((rc = pw.add((t.param_len + stg::MERGE_TILE - 1) / stg::MERGE_TILE, &dp))) return rc;
            if (pw.count() == 1) {
                w0 = i;
                P::common(L[i], pw.table());
            }
            stg::MergeWorldTensor &d = *dp;
            d.out_idx = t.d_out_idx;
            d.out_val = t.d_out_val;
            d.out_count = t.d_out_count;
            d.param = t.d_param;
            d.n = t.param_len;
            d.off = (uint32_t)w_off;
            P::fill(L[i], d);
            w_off += (t.param_len + stg::MERGE_WORLD_ALIGN - 1) / stg::MERGE_WORLD_ALIGN * stg::MERGE_WORLD_ALIGN;
            w_n += t.param_len;
            continue;
        }
        // (the packer closes at MERGE_BATCH tensors; the winner-word cap and a repeated name close here)
        bool close = pk.count() && sum_n + t.param_len > stg::MERGE_BATCH_WIN_CAP;
        for (size_t q = g0; !close && q < g0 + pk.count(); ++q) close = strcmp(tasks[q].name, t.name) == 0;
        if (close && (rc = pk.flush())) return rc;
        stg::MergeTensor *dp;
        if ((rc = pk.add((t.per_rank + stg::MERGE_BATCH_TILE - 1) / stg::MERGE_BATCH_TILE, &dp))) return rc;
        if (pk.count() == 1) {
            g0 = i;
            P::common(L[i], pk.table());
        }
        stg::MergeTensor &d = *dp;
        const stg::RankStream &k = calls[i].rs[0];
        d.idx = k.idx;
        d.val = k.val;
        d.flag = k.flag;
        d.out_idx = t.d_out_idx;
        d.out_val = t.d_out_val;
        d.out_count = t.d_out_count;
        d.param = t.d_param;
        d.m = (uint32_t)t.per_rank;
        d.n = t.param_len;
        d.win0 = (uint32_t)sum_n;
        d.desc0 = d.blk0;
        P::fill(L[i], d);
        sum_n += t.param_len;
    }
    if (const int rc = pk.flush()) return rc;
    return pw.flush();
}

}  // namespace

extern "C" {

int stg_scatter_merge_device(const uint32_t *d_idx, const float *d_val, size_t per_rank, int world, size_t n,
                             float *d_dense, uint8_t *d_mark, uint32_t *d_out_idx, float *d_out_val,
                             uint32_t *d_out_count, void *stream) {
    return scatter_merge(MergeCall{decoded_streams(d_idx, d_val, per_rank, world), false, per_rank, world, n, d_dense,
                                   d_mark, d_out_idx, d_out_val, d_out_count, stream});
}

int stg_scatter_merge_wire_device(const stg_rank_stream_t *ranks, size_t per_rank, int world, size_t n,
                                  float *d_dense, uint8_t *d_mark, uint32_t *d_out_idx, float *d_out_val,
                                  uint32_t *d_out_count, void *stream) {
    return scatter_merge(MergeCall{wire_streams(ranks, world), true, per_rank, world, n, d_dense, d_mark, d_out_idx,
                                   d_out_val, d_out_count, stream});
}

int stg_scatter_merge_check(void *stream) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::shared_ptr<MergeScratch> ms;
    {
        std::lock_guard<std::mutex> g(g_merge_mu);
        auto it = g_merge.find({dev, s});
        if (it == g_merge.end()) return STG_OK;  // no merge on this stream yet
        ms = it->second;
    }
    std::lock_guard<std::mutex> g(ms->mu);
    HIP_TRY(hipStreamSynchronize(s));
    uint32_t f = 0;
    if (ms->fail.get()) HIP_TRY(hipMemcpy(&f, ms->fail.get(), sizeof f, hipMemcpyDeviceToHost));
    if (f) {
        char b[96];
        snprintf(b, sizeof b, "MERGE decompress device failure flags 0x%x (a look-back gave up)", f);
        return fail(STG_ERR_DEVICE, b);
    }
    return STG_OK;
}

int stg_merge_batch_launches(void *stream, uint64_t *out) {
    if (!out) return fail(STG_ERR_INVALID, "null argument");
    *out = 0;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::shared_ptr<MergeScratch> ms;
    {
        std::lock_guard<std::mutex> g(g_merge_mu);
        auto it = g_merge.find({dev, static_cast<hipStream_t>(stream)});
        if (it == g_merge.end()) return STG_OK;  // no merge on this stream yet
        ms = it->second;
    }
    std::lock_guard<std::mutex> g(ms->mu);
    *out = ms->launches;
    return STG_OK;
}

int stg_scatter_merge_release(void *stream) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::shared_ptr<MergeScratch> ms;
    {
        std::lock_guard<std::mutex> g(g_merge_mu);
        auto it = g_merge.find({dev, s});
        if (it == g_merge.end()) return STG_OK;
        ms = std::move(it->second);
        g_merge.erase(it);
    }
    {
        std::lock_guard<std::mutex> g(ms->mu);  // calls already inside finish first
        HIP_TRY(hipStreamSynchronize(s));
    }
    ms.reset();  // freed here, or by the last caller still holding it
    return STG_OK;
}

int stg_sgd_create(int device, float lr, float momentum, float dampening, float weight_decay, int nesterov,
                   int maximize, stg_sgd_t *out) {
    if (!out) return fail(STG_ERR_INVALID, "null argument");
    auto o = std::make_unique<stg_sgd>();
    o->device = device;
    o->lr = lr;
    o->momentum = momentum;
    o->dampening = dampening;
    o->weight_decay = weight_decay;
    o->nesterov = nesterov != 0;
    o->maximize = maximize != 0;
    *out = o.release();
    return STG_OK;
}

int stg_sgd_destroy(stg_sgd_t o) {
    delete o;
    return STG_OK;
}

int stg_sgd_optimize_raw_device(stg_sgd_t o, const char *name, float *d_param, uint32_t param_len, const float *d_grad,
                                const uint32_t *d_idx, uint32_t grad_len, const uint32_t *d_grad_len, void *stream) {
    return optimize_raw<SgdBatch>(o, name, d_param, param_len, d_grad, d_idx, grad_len, d_grad_len, stream);
}

int stg_merge_optimize_sgd_device(stg_sgd_t o, const char *name, float *d_param, uint32_t param_len,
                                  const uint32_t *d_idx, const float *d_val, size_t per_rank, int world,
                                  float *d_dense, uint8_t *d_mark, uint32_t *d_out_idx, float *d_out_val,
                                  uint32_t *d_out_count, void *stream) {
    return merge_optimize<SgdBatch>(o, name, d_param, param_len,
                                    MergeCall{decoded_streams(d_idx, d_val, per_rank, world), false, per_rank, world,
                                        param_len, d_dense, d_mark, d_out_idx, d_out_val, d_out_count, stream});
}

int stg_merge_optimize_sgd_wire_device(stg_sgd_t o, const char *name, float *d_param, uint32_t param_len,
                                       const stg_rank_stream_t *ranks, size_t per_rank, int world, float *d_dense,
                                       uint8_t *d_mark, uint32_t *d_out_idx, float *d_out_val,
                                       uint32_t *d_out_count, void *stream) {
    return merge_optimize<SgdBatch>(o, name, d_param, param_len,
                                    MergeCall{wire_streams(ranks, world), true, per_rank, world, param_len, d_dense, d_mark,
                                        d_out_idx, d_out_val, d_out_count, stream});
}

int stg_sgd_get_momentum(stg_sgd_t o, const char *name, float *host_out, uint32_t len, void *stream) {
    if (!o || !name) return fail(STG_ERR_INVALID, "null argument");
    return sgd_read_back(o, o->mom, name, host_out, len, stream, "no momentum buffer for this name");
}

// The factor table of smart momentum: (float)pow((double)m, (double)d) by the
// host's libm, as sgd.cpp:226 computes it, for d = 0 .. d0, d0 the first d that
// gives 0.f (m < 1: the values fall monotonically, so every later one is 0 too).
constexpr size_t SGD_POW_CAP = size_t(1) << 22;  // entries; m = 0.9999 needs ~1.04 M

int stg_sgd_set_smart_momentum(stg_sgd_t o, int on) {
    if (!o) return fail(STG_ERR_INVALID, "null argument");
    if (!on) {
        std::lock_guard<std::mutex> g(o->mu);
        o->smart = false;
        return STG_OK;
    }
    // momentum 0: the reference has no last-touched array to read (sgd.cpp:43-54);
    // outside (0, 1) every factor trips its range assertion (sgd.cpp:229-232)
    if (!(o->momentum > 0.f && o->momentum < 1.f))
        return fail(STG_ERR_INVALID, "smart momentum needs 0 < momentum < 1");
    std::lock_guard<std::mutex> g(o->mu);
    if (!o->pow_tab.get()) {
        std::vector<float> tab;
        for (;;) {
            const float v = (float)std::pow((double)o->momentum, (double)tab.size());
            tab.push_back(v);
            if (v == 0.f) break;
            if (tab.size() >= SGD_POW_CAP)
                return fail(STG_ERR_UNSUPPORTED, "smart momentum: the factor table of this momentum exceeds 2^22 entries");
        }
        HIP_TRY(hipSetDevice(o->device));
        stg::DevBuf<float> t;  // (exactly tab.size() entries: its capacity is the table's length)
        stg::DevBuf<uint32_t> f;
        HIP_TRY(t.reserve(tab.size(), nullptr, false));
        if (hipMemcpy(t.get(), tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
            f.reserve(1, nullptr, true) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
            return fail(STG_ERR_HIP, "smart momentum: uploading the factor table failed");
        // resident before any launch can name it; never moved or freed before destroy
        o->pow_tab = std::move(t);
        o->fail = std::move(f);
    }
    o->smart = true;
    return STG_OK;
}

int stg_sgd_get_last(stg_sgd_t o, const char *name, uint32_t *host_out, uint32_t len, void *stream) {
    if (!o || !name || (len && !host_out)) return fail(STG_ERR_INVALID, "null argument");
    return sgd_read_back(o, o->last, name, host_out, len, stream, "no smart-momentum state for this name");
}

int stg_sgd_get_iter(stg_sgd_t o, uint32_t *out) {
    if (!o || !out) return fail(STG_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(o->mu);
    *out = o->iter;
    return STG_OK;
}

int stg_sgd_check(stg_sgd_t o, void *stream) {
    if (!o) return fail(STG_ERR_INVALID, "null argument");
    uint32_t *fw = nullptr;
    {
        std::lock_guard<std::mutex> g(o->mu);
        fw = o->fail.get();
    }
    if (!fw) return STG_OK;  // the option was never on: nothing can have failed
    HIP_TRY(hipSetDevice(o->device));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    uint32_t f = 0;
    HIP_TRY(hipMemcpy(&f, fw, sizeof f, hipMemcpyDeviceToHost));
    if (f)
        return fail(STG_ERR_DEVICE, "sgd: a smart-momentum factor was outside [0, 1) (an index repeated within one "
                                    "call); those elements were skipped");
    return STG_OK;
}

int stg_adam_create(int device, float lr, float b1, float b2, float eps, float weight_decay, int amsgrad,
                    int maximize, stg_adam_t *out) {
    if (!out) return fail(STG_ERR_INVALID, "null argument");
    auto o = std::make_unique<stg_adam>();
    o->device = device;
    o->lr = lr;
    o->b1 = b1;
    o->b2 = b2;
    o->eps = eps;
    o->weight_decay = weight_decay;
    o->amsgrad = amsgrad != 0;
    o->maximize = maximize != 0;
    *out = o.release();
    return STG_OK;
}

int stg_adam_destroy(stg_adam_t o) {
    delete o;
    return STG_OK;
}

int stg_adam_optimize_raw_device(stg_adam_t o, const char *name, float *d_param, uint32_t param_len,
                                 const float *d_grad, const uint32_t *d_idx, uint32_t grad_len,
                                 const uint32_t *d_grad_len, void *stream) {
    return optimize_raw<AdamBatch>(o, name, d_param, param_len, d_grad, d_idx, grad_len, d_grad_len, stream);
}

int stg_merge_optimize_adam_device(stg_adam_t o, const char *name, float *d_param, uint32_t param_len,
                                   const uint32_t *d_idx, const float *d_val, size_t per_rank, int world,
                                   float *d_dense, uint8_t *d_mark, uint32_t *d_out_idx, float *d_out_val,
                                   uint32_t *d_out_count, void *stream) {
    return merge_optimize<AdamBatch>(o, name, d_param, param_len,
                                     MergeCall{decoded_streams(d_idx, d_val, per_rank, world), false, per_rank, world,
                                         param_len, d_dense, d_mark, d_out_idx, d_out_val, d_out_count, stream});
}

int stg_merge_optimize_adam_wire_device(stg_adam_t o, const char *name, float *d_param, uint32_t param_len,
                                        const stg_rank_stream_t *ranks, size_t per_rank, int world, float *d_dense,
                                        uint8_t *d_mark, uint32_t *d_out_idx, float *d_out_val,
                                        uint32_t *d_out_count, void *stream) {
    return merge_optimize<AdamBatch>(o, name, d_param, param_len,
                                     MergeCall{wire_streams(ranks, world), true, per_rank, world, param_len, d_dense, d_mark,
                                         d_out_idx, d_out_val, d_out_count, stream});
}

int stg_merge_optimize_sgd_batch_device(stg_sgd_t o, const stg_merge_task_t *tasks, size_t ntasks, void *stream) {
    return merge_optimize_batch<SgdBatch>(o, tasks, ntasks, stream);
}

int stg_merge_optimize_adam_batch_device(stg_adam_t o, const stg_merge_task_t *tasks, size_t ntasks, void *stream) {
    return merge_optimize_batch<AdamBatch>(o, tasks, ntasks, stream);
}

int stg_adam_get_state(stg_adam_t o, const char *name, float *host_m, float *host_v, uint32_t len,
                       float *host_vmax, uint32_t *tick_out, void *stream) {
    if (!o || !name) return fail(STG_ERR_INVALID, "null argument");
    const stg_adam::Name *nm;  // (a name's state never moves or goes before destroy)
    uint32_t tick;
    {
        std::lock_guard<std::mutex> g(o->mu);
        auto it = o->st.find(name);
        if (it == o->st.end()) return fail(STG_ERR_INVALID, "no Adam state for this name");
        nm = &it->second;
        tick = nm->tick;
    }
    HIP_TRY(hipSetDevice(o->device));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    const size_t c = std::min(len, nm->len);
    if (host_m) HIP_TRY(hipMemcpy(host_m, nm->m(), c * sizeof(float), hipMemcpyDeviceToHost));
    if (host_v) HIP_TRY(hipMemcpy(host_v, nm->v(), c * sizeof(float), hipMemcpyDeviceToHost));
    if (host_vmax) HIP_TRY(hipMemcpy(host_vmax, nm->vmax(), sizeof(float), hipMemcpyDeviceToHost));
    if (tick_out) *tick_out = tick;
    return STG_OK;
}

int stg_adam_check(stg_adam_t o, void *stream) {
    if (!o) return fail(STG_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(o->device));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    uint32_t f = 0;
    if (o->fail.get()) HIP_TRY(hipMemcpy(&f, o->fail.get(), sizeof f, hipMemcpyDeviceToHost));
    if (f) return fail(STG_ERR_DEVICE, "adam: amsgrad look-back timed out (a predecessor tile never published)");
    return STG_OK;
}

int stg_gather_slice(uint64_t n, int local_rank, int num_gpus, uint64_t *start, uint64_t *end) {
    if (!start || !end) return fail(STG_ERR_INVALID, "null argument");
    if (num_gpus < 1 || local_rank < 0 || local_rank >= num_gpus) return fail(STG_ERR_INVALID, "bad rank / GPU count");
    *start = (uint64_t)(((int64_t)n * local_rank) / num_gpus);  // cpu_gather.cpp:59-60 (int64 arithmetic)
    *end = (uint64_t)(((int64_t)n * (local_rank + 1)) / num_gpus);
    return STG_OK;
}

int stg_gather_add_device(float *d_grad0, const float *d_residual, const float *const *d_grads, int num_gpus,
                          uint64_t n, int local_rank, void *stream) {
    if (num_gpus < 1 || num_gpus > (int)stg::GATHER_MAX) return fail(STG_ERR_UNSUPPORTED, "num_gpus outside 1..16");
    uint64_t a = 0, b = 0;
    int rc = stg_gather_slice(n, local_rank, num_gpus, &a, &b);
    if (rc) return rc;
    if (a == b) return STG_OK;
    if (!d_grad0 || (num_gpus > 1 && !d_grads)) return fail(STG_ERR_INVALID, "null argument");
    for (int i = 1; i < num_gpus; ++i)
        if (!d_grads[i]) return fail(STG_ERR_INVALID, "null source");
    const stg::GatherArgs g = gather_args(d_grad0, d_residual, d_grads, num_gpus);
    int ncu;
    if (const int rc = device_cus(&ncu)) return rc;
    HIP_TRY(stg::launch_gather_add(g, a, b, ncu, static_cast<hipStream_t>(stream)));
    return STG_OK;
}

int stg_gather_add_typed_device(float *d_grad0, const float *d_residual, const stg_grad_src_t *srcs, int num_gpus,
                                uint64_t n, int local_rank, void *stream) {
    if (num_gpus < 1 || num_gpus > (int)stg::GATHER_MAX) return fail(STG_ERR_UNSUPPORTED, "num_gpus outside 1..16");
    uint64_t a = 0, b = 0;
    int rc = stg_gather_slice(n, local_rank, num_gpus, &a, &b);
    if (rc) return rc;
    stg::GatherArgs g;
    bool typed;
    std::string why;
    if ((rc = typed_gather_args(d_grad0, d_residual, srcs, num_gpus, b - a, &g, &typed, &why))) return fail(rc, why);
    if (a == b) return STG_OK;
    if (!d_grad0) return fail(STG_ERR_INVALID, "null argument");
    int ncu;
    if (const int rc = device_cus(&ncu)) return rc;
    // fp32 in place: the fp32 launcher (g is then what gather_args builds)
    HIP_TRY((typed ? stg::launch_gather_add_typed : stg::launch_gather_add)(g, a, b, ncu, static_cast<hipStream_t>(stream)));
    return STG_OK;
}

int stg_debug_gather_plan(const uint64_t *addrs, const int *dtypes, size_t nstreams, uint64_t n, uint32_t *width,
                          uint32_t *head) {
    if (!addrs || !dtypes || !width || !head || nstreams < 1 || nstreams > stg::GATHER_MAX + 2)
        return fail(STG_ERR_INVALID, "null argument or stream count outside 1..18");
    uintptr_t addr[stg::GATHER_MAX + 2];
    uint32_t esz[stg::GATHER_MAX + 2];
    for (size_t i = 0; i < nstreams; ++i) {
        if (dtypes[i] != STG_DT_F32 && dtypes[i] != STG_DT_BF16 && dtypes[i] != STG_DT_F16)
            return fail(STG_ERR_INVALID, "unknown dtype");
        addr[i] = (uintptr_t)addrs[i];
        esz[i] = dtypes[i] == STG_DT_F32 ? 4u : 2u;
    }
    const stg::GatherPlan p = stg::gather_plan(addr, esz, (uint32_t)nstreams, n, stg::gather_max_width());
    *width = p.width;
    *head = p.head;
    return STG_OK;
}

int stg_wire_flag(uint64_t tensor_numel, int fp16_values) {
    return (tensor_numel < 65536 ? STG_WIRE_U16_IDX : 0) | (fp16_values ? STG_WIRE_F16_VAL : 0);
}

int stg_wire_encode_device(const uint32_t *d_idx, const float *d_val, size_t numel, int flag, void *d_idx_out,
                           void *d_val_out, void *stream) {
    if (flag & ~(STG_WIRE_U16_IDX | STG_WIRE_F16_VAL)) return fail(STG_ERR_INVALID, "unknown wire flag bits");
    if (!numel) return STG_OK;
    if (!d_idx || !d_val || !d_idx_out || !d_val_out) return fail(STG_ERR_INVALID, "null argument");
    int ncu;
    if (const int rc = device_cus(&ncu)) return rc;
    HIP_TRY(stg::launch_wire_encode(d_idx, d_val, numel, (uint32_t)flag, d_idx_out, d_val_out, ncu,
                                    static_cast<hipStream_t>(stream)));
    return STG_OK;
}

int stg_wire_encode_batch_device(const stg_wire_stream_t *streams, size_t nstreams, void *stream) {
    if (nstreams && !streams) return fail(STG_ERR_INVALID, "null stream array");
    for (size_t i = 0; i < nstreams; ++i) {
        const stg_wire_stream_t &w = streams[i];
        if (w.flag & ~(STG_WIRE_U16_IDX | STG_WIRE_F16_VAL)) return fail(STG_ERR_INVALID, "unknown wire flag bits");
        if (w.numel && (!w.d_idx || !w.d_val || !w.d_idx_out || !w.d_val_out))
            return fail(STG_ERR_INVALID, "null argument");
        if (w.numel > (size_t)STG_WG * 0xffffffull) return fail(STG_ERR_UNSUPPORTED, "wire stream too long for a batch");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto b = stream_packer<stg::WireBatch>(GRID_MAX, stg::launch_wire_encode_batch, s);
    for (size_t i = 0; i < nstreams; ++i) {
        const stg_wire_stream_t &w = streams[i];
        if (!w.numel) continue;
        const uint64_t nbk = (w.numel + STG_WG - 1) / STG_WG;
        stg::WireBucket *d;
        if (const int rc = b.add(nbk, &d)) return rc;
        d->idx = w.d_idx;
        d->val = w.d_val;
        d->idx_out = w.d_idx_out;
        d->val_out = w.d_val_out;
        d->n = w.numel;
        d->flag = (uint32_t)w.flag;
    }
    return b.flush();
}

int stg_wire_decode_device(const void *d_idx_in, const void *d_val_in, size_t numel, int flag, uint32_t *d_idx,
                           float *d_val, void *stream) {
    if (flag & ~(STG_WIRE_U16_IDX | STG_WIRE_F16_VAL)) return fail(STG_ERR_INVALID, "unknown wire flag bits");
    if (!numel) return STG_OK;
    if (!d_idx_in || !d_val_in || !d_idx || !d_val) return fail(STG_ERR_INVALID, "null argument");
    int ncu;
    if (const int rc = device_cus(&ncu)) return rc;
    HIP_TRY(stg::launch_wire_decode(d_idx_in, d_val_in, numel, (uint32_t)flag, d_idx, d_val, ncu,
                                    static_cast<hipStream_t>(stream)));
    return STG_OK;
}

int stg_wire_decode_batch_device(const stg_wire_rx_t *streams, size_t nstreams, void *stream) {
    if (nstreams && !streams) return fail(STG_ERR_INVALID, "null stream array");
    for (size_t i = 0; i < nstreams; ++i) {
        const stg_wire_rx_t &w = streams[i];
        if (w.flag & ~(STG_WIRE_U16_IDX | STG_WIRE_F16_VAL)) return fail(STG_ERR_INVALID, "unknown wire flag bits");
        if (w.numel && (!w.d_idx_in || !w.d_val_in || !w.d_idx || !w.d_val))
            return fail(STG_ERR_INVALID, "null argument");
        if (w.numel > (size_t)STG_WG * 0xffffffull) return fail(STG_ERR_UNSUPPORTED, "wire stream too long for a batch");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto b = stream_packer<stg::WireRxBatch>(GRID_MAX, stg::launch_wire_decode_batch, s);
    for (size_t i = 0; i < nstreams; ++i) {
        const stg_wire_rx_t &w = streams[i];
        if (!w.numel) continue;
        const uint64_t nbk = (w.numel + STG_WG - 1) / STG_WG;
        stg::WireRx *d;
        if (const int rc = b.add(nbk, &d)) return rc;
        d->idx_in = w.d_idx_in;
        d->val_in = w.d_val_in;
        d->idx = w.d_idx;
        d->val = w.d_val;
        d->n = w.numel;
        d->flag = (uint32_t)w.flag;
    }
    return b.flush();
}

int stg_param_publish_batch_device(const stg_publish_task_t *tasks, size_t ntasks, void *stream) {
    if (ntasks && !tasks) return fail(STG_ERR_INVALID, "null task array");
    bool any = false;
    for (size_t i = 0; i < ntasks; ++i) {
        const stg_publish_task_t &t = tasks[i];
        auto bad = [&](const std::string &what) {
            return fail(STG_ERR_INVALID, "publish task " + std::to_string(i) + ": " + what);
        };
        if (t.nreplicas < 1 || t.nreplicas > (int)stg::PUBLISH_MAXR) return bad("nreplicas outside 1..16");
        if (t.idx_cap) {
            if (!t.d_param || !t.d_idx || !t.d_count || !t.replicas) return bad("null argument");
            if (!t.param_len) return bad("empty parameter");
            any = true;
        }
        for (int r = 0; t.replicas && r < t.nreplicas; ++r) {
            const stg_replica_t &p = t.replicas[r];
            if (p.dtype != STG_DT_F32 && p.dtype != STG_DT_BF16 && p.dtype != STG_DT_F16)
                return bad("replica " + std::to_string(r) + ": unknown dtype");
            if (t.idx_cap && !p.d_param) return bad("replica " + std::to_string(r) + ": null pointer");
            if (reinterpret_cast<uintptr_t>(p.d_param) & publish_elem_mask(p.dtype))
                return bad("replica " + std::to_string(r) + ": pointer not aligned to its element size");
        }
    }
    if (!any) return STG_OK;
    int ncu;
    if (const int rc = device_cus(&ncu)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool runs = env_int(getenv("STG_DEBUG_PUBLISH_SCALAR"), 0) != 1;  // measurements: the scalar-only kernel
    return publish_pack(
        ntasks, ncu, [&](size_t i) { return tasks[i].idx_cap; },
        [&](size_t i, stg::PublishTask *d) {
            const stg_publish_task_t &t = tasks[i];
            d->param = t.d_param;
            d->idx = t.d_idx;
            d->count = t.d_count;
            d->n = t.param_len;
            d->cap = t.idx_cap;
            d->nrep = (uint32_t)t.nreplicas;
            for (int r = 0; r < t.nreplicas; ++r) {
                d->rep[r] = t.replicas[r].d_param;
                d->dtypes |= (uint32_t)t.replicas[r].dtype << (2 * r);
            }
        },
        [&](stg::PublishBatch &w, uint32_t blocks) -> int {
            HIP_TRY(stg::launch_param_publish_batch(w, blocks, runs, s));
            return STG_OK;
        });
}

int stg_debug_publish_launches(const uint32_t *idx_caps, size_t ntasks, int num_cu) {
    if ((ntasks && !idx_caps) || num_cu < 1) return 0;
    int launches = 0;
    publish_pack(
        ntasks, num_cu, [&](size_t i) { return idx_caps[i]; }, [](size_t, stg::PublishTask *) {},
        [&](stg::PublishBatch &, uint32_t) -> int {
            ++launches;
            return STG_OK;
        });
    return launches;
}

int stg_debug_tv_batch_plan(const uint64_t *n, size_t ntasks, int num_cu, uint32_t *first_range, uint32_t *launch_of) {
    if ((ntasks && (!n || !first_range || !launch_of)) || num_cu < 1) return STG_ERR_INVALID;
    int launches = 0;
    for (size_t i = 0; i < ntasks; ++i) {
        first_range[i] = 0;
        launch_of[i] = 0xffffffffu;  // (an empty task: no launch)
    }
    tv_batch_pack(
        ntasks, num_cu, [&](size_t i) { return n[i]; },
        [&](size_t i, stg::TvBatchTask *d) {
            first_range[i] = d->blk0;
            launch_of[i] = (uint32_t)launches;
        },
        [&](stg::TvBatch &, uint32_t) -> int {
            ++launches;
            return STG_OK;
        },
        [&](size_t i) -> int {
            launch_of[i] = (uint32_t)launches++;
            return STG_OK;
        });
    return launches;
}

int stg_debug_topk_batch_plan(const uint64_t *n, size_t ntasks, int num_cu, uint32_t *first_tile, uint32_t *launch,
                              uint32_t *tile_cap) {
    if (!n || !first_tile || !launch || !tile_cap || num_cu <= 0) return -1;
    *tile_cap = (uint32_t)stg::topk_batch_tile_cap(num_cu);
    int groups = 0;
    for (size_t i = 0; i < ntasks; ++i) {
        first_tile[i] = 0;
        launch[i] = 0xffffffffu;  // (an empty task: no group)
    }
    topk_batch_pack(
        ntasks, num_cu, [&](size_t i) { return n[i]; },
        [&](size_t i, stg::TopkBatchTask *d) {
            first_tile[i] = d->blk0;
            launch[i] = (uint32_t)groups;
        },
        [&](stg::TopkBatch &, uint32_t) -> int {
            ++groups;
            return STG_OK;
        },
        [&](size_t i) -> int {
            launch[i] = (uint32_t)groups++;
            return STG_OK;
        });
    return groups;
}

int stg_synth_fill_device(float *d_dst, size_t n, uint64_t seed, int dist, uint32_t param, void *stream) {
    if (!n) return STG_OK;
    HIP_TRY(stg::launch_synth(d_dst, n, seed, dist, param, static_cast<hipStream_t>(stream)));
    return STG_OK;
}

}  // extern "C"
