/*
 * stg_oracle.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * Clean-room CPU restatement of StellaTrain's gradient-sparsification codec
 * (reference snapshot 2024-08-07, backend/src/compress) plus the caller-side
 * arithmetic (engine/modules/compress.cpp MERGE path), the MERGE decompress
 * (engine/modules/cpu_optimize.cpp) and the scalar sparse-SGD loop
 * (optim/sgd.cpp).  It is the *checker* for the HIP product path in
 * stellatrain_amd/csrc and the "port" CPU baseline in bench.py.  Nothing in
 * the product path may link or call this file.
 *
 * Parity pin: tests/test_oracle_golden.py checks this restatement bit-exactly
 * against golden vectors produced by the reference sources themselves
 * (oracle/_ref, built in place from /root/reference by oracle/Makefile;
 * generator script tests/golden/make_golden.py).
 *
 * Semantics restated here (citations are /root/reference/backend/src/...):
 *   - thresholdv16: compress/thresholdv16.cpp:22-29, 36-54, 57-73, 78-295
 *   - threshold-v : compress/thresholdv.cpp:18-20, 27-37, 40-83, 292-293
 *                   (the AVX-512 path is compiled out under -march=broadwell)
 *   - top-k       : compress/topk.cpp:13-46 (incl. the byte-count memcpy bug)
 *   - MERGE decompress: engine/modules/cpu_optimize.cpp:40-72
 *   - sparse SGD  : optim/sgd.cpp:34-55, 221-263 (scalar path)
 *   - sparse Adam : optim/adam.cpp:19-86 (FMA shapes of the -O3 object code)
 *   - gather-add  : engine/modules/cpu_gather.cpp:59-87 with misc/array_util.h:12-54
 *   - wire format : engine/comm_manager.cpp:486-567 (index / value casts of the
 *                   ZeroMQ ring), flags :573-590, comm_manager.h:24-27
 *
 * The regime-B heap fill deliberately uses std::priority_queue: the
 * reference's tie order among equal block sums *is* libstdc++'s
 * make_heap/pop_heap order, so the oracle reproduces it by construction.
 */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#define ORC_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr uint32_t kLine = 16;  // floats per 64-byte cache line (thresholdv16.cpp:20)

// ---------------------------------------------------------------------------
// Synthetic inputs: integer-only generator, identical in
// numpy (stellatrain_amd/synth.py) and on the device (csrc/synth.hip).
// ---------------------------------------------------------------------------
inline uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// ---------------------------------------------------------------------------
// thresholdv16
// ---------------------------------------------------------------------------

// |x| summed in the AVX tree order of hsum_float_avx (thresholdv16.cpp:57-73):
// h(a) = ((a0+a4)+(a1+a5)) + ((a2+a6)+(a3+a7)); block = h(lo8) + h(hi8).
inline float half_tree(const float *p) {
    const float s04 = std::fabs(p[0]) + std::fabs(p[4]);
    const float s15 = std::fabs(p[1]) + std::fabs(p[5]);
    const float s26 = std::fabs(p[2]) + std::fabs(p[6]);
    const float s37 = std::fabs(p[3]) + std::fabs(p[7]);
    return (s04 + s15) + (s26 + s37);
}
inline float block_tree_sum(const float *p) { return half_tree(p) + half_tree(p + 8); }

// thresholdv16.cpp:36-54: sequential per-block |x| sums, the last partial
// block scaled by 16/(n%16), then the (k/16)-th largest (0-based).
float tv16_first_threshold(const float *src, size_t n, uint32_t k) {
    const size_t nblk = (n + kLine - 1) / kLine;
    size_t bk = k / kLine;
    std::vector<float> bs(nblk, 0.f);
    for (size_t i = 0; i < n; ++i) bs[i / kLine] += std::fabs(src[i]);
    if (n % kLine) bs[nblk - 1] *= static_cast<float>(kLine) / static_cast<float>(n % kLine);
    if (bk >= nblk) bk = nblk - 1;  // reference reads past the end here (k == n); clamp
    std::nth_element(bs.begin(), bs.begin() + bk, bs.end(),
                     [](float a, float b) { return std::fabs(a) > std::fabs(b); });
    return std::fabs(bs[bk]);
}

struct Tv16State {
    float t;
    float inc;
};

struct Tv16 {
    std::mutex mu;
    std::unordered_map<std::string, Tv16State> st;
};

// thresholdv16.cpp:78-295 restated (stage 1 / stage 2 / stage 3 / AIMD / heap).
size_t tv16_compress(Tv16 *h, const std::string &name, const float *src, size_t n, uint32_t k,
                     uint32_t *idx, size_t idx_cap, float *val, int32_t off) {
    float t, inc;
    bool have;
    {
        std::lock_guard<std::mutex> g(h->mu);
        auto it = h->st.find(name);
        have = it != h->st.end();
        if (have) { t = it->second.t; inc = it->second.inc; }
    }
    if (!have) {
        t = tv16_first_threshold(src, n, k);
        inc = static_cast<float>(static_cast<double>(t) * 0.01);
    }

    const uint32_t dst_len = static_cast<uint32_t>(idx_cap);
    const size_t nb = n / kLine;
    const uint32_t tl = static_cast<uint32_t>(n % kLine);
    const uint32_t d16 = dst_len - dst_len % kLine;
    uint32_t cnt = 0;
    size_t j = 0;
    std::vector<std::pair<float, uint32_t>> cand;
    cand.reserve(n / kLine + 1);

    auto emit = [&](size_t pos, uint32_t len) {
        for (uint32_t i = 0; i < len; ++i) {
            idx[cnt + i] = static_cast<uint32_t>(pos + i) + static_cast<uint32_t>(off);
            val[cnt + i] = src[pos + i];
        }
        cnt += len;
    };

    // stage 1: whole lines while at least one whole line of room remains
    for (; j < nb && cnt < d16; ++j) {
        const float s = block_tree_sum(src + j * kLine);
        if (s >= t) emit(j * kLine, kLine);
        else cand.emplace_back(s, static_cast<uint32_t>(j * kLine));
    }
    // stage 2: fewer than 16 slots left; first qualifying line donates a prefix
    bool filled_in_stage2 = false;
    if (j < nb && cnt < dst_len) {
        const uint32_t rem = dst_len - cnt;
        for (; j < nb; ++j) {
            const float s = block_tree_sum(src + j * kLine);
            if (s >= t) { emit(j * kLine, rem); filled_in_stage2 = true; break; }
            cand.emplace_back(s, static_cast<uint32_t>(j * kLine));
        }
    }
    // stage 3: ragged tail, judged on its *signed* sum (thresholdv16.cpp:212-236)
    if (!filled_in_stage2 && tl != 0 && cnt < dst_len) {
        const size_t p0 = nb * kLine;
        const uint32_t rem = dst_len - cnt;
        float s = 0.f;
        for (uint32_t i = 0; i < tl; ++i) s += src[p0 + i];
        if (s * static_cast<float>(kLine) >= t * static_cast<float>(tl)) {
            emit(p0, std::min(rem, tl));
        } else {
            cand.emplace_back(s * static_cast<float>(kLine) / static_cast<float>(tl),
                              static_cast<uint32_t>(p0));
        }
    }

    // AIMD (thresholdv16.cpp:243-259)
    if (cnt < dst_len) t = static_cast<float>(static_cast<double>(t) * 0.99);
    else t = t + inc;
    {
        std::lock_guard<std::mutex> g(h->mu);
        h->st[name] = Tv16State{t, inc};
    }

    // heap fill (thresholdv16.cpp:261-293): libstdc++ priority_queue order
    if (cnt < dst_len) {
        struct Less {
            bool operator()(const std::pair<float, uint32_t> &a, const std::pair<float, uint32_t> &b) const {
                return a.first < b.first;
            }
        };
        std::priority_queue<std::pair<float, uint32_t>, std::vector<std::pair<float, uint32_t>>, Less> q(Less(), cand);
        while (cnt < dst_len && !q.empty()) {
            const uint32_t pos = q.top().second;
            const uint32_t len = std::min(16u, std::min(static_cast<uint32_t>(n - pos), dst_len - cnt));
            emit(pos, len);
            q.pop();
        }
    }
    return cnt;
}

// ---------------------------------------------------------------------------
// threshold-v (naive path: thresholdv.cpp:40-83)
// ---------------------------------------------------------------------------
float tv_first_threshold(const float *src, size_t n, uint32_t k) {
    std::vector<float> c(src, src + n);
    size_t kk = std::min<size_t>(k, n - 1);  // reference reads c[n] when k == n; clamp
    std::nth_element(c.begin(), c.begin() + kk, c.end(),
                     [](float a, float b) { return std::fabs(a) > std::fabs(b); });
    return std::fabs(c[kk]);
}

struct Tv {
    std::mutex mu;
    std::unordered_map<uint64_t, float> st;
};

size_t tv_compress(Tv *h, uint64_t key, const float *src, size_t n, uint32_t k, uint32_t *idx,
                   size_t cap, float *val) {
    float t;
    bool have;
    {
        std::lock_guard<std::mutex> g(h->mu);
        auto it = h->st.find(key);
        have = it != h->st.end();
        if (have) t = it->second;
    }
    if (!have) t = tv_first_threshold(src, n, k);

    size_t cnt = 0;
    float gmax = -1.f;
    for (size_t i = 0; i < n; ++i) {
        const float a = std::fabs(src[i]);
        gmax = (a < gmax) ? gmax : a;  // std::max(a, gmax)
        if (a >= t) {
            if (cnt < cap) { idx[cnt] = static_cast<uint32_t>(i); val[cnt] = src[i]; }
            ++cnt;
        }
    }
    // AIMD; GCC -O3 -march=broadwell contracts the increase into one vfmadd231sd
    if (k > cnt) t = static_cast<float>(static_cast<double>(t) * 0.99);
    else if (k < cnt)
        t = static_cast<float>(std::fma(0.01 * static_cast<double>(cnt) / static_cast<double>(k),
                                         static_cast<double>(gmax), static_cast<double>(t)));
    {
        std::lock_guard<std::mutex> g(h->mu);
        h->st[key] = t;
    }
    return std::min(cnt, cap);
}

// ---------------------------------------------------------------------------
// Sparse SGD, scalar path (optim/sgd.cpp:34-55, 221-263).
// Smart momentum (sgd.cpp:54, 225-232, 258-259): a per-name array of the
// iteration that last touched each element, allocated zeroed with the momentum
// buffer (:46-47) whether or not the option is on.  Where the momentum stands,
// the factor (float)pow((double)m, (double)(iter - last[idx])) stands -- the
// ternary's type is double, stored in a float -- and m itself at iteration 0.
// The reference asserts the factor in [0, 1); nothing is skipped here: an index
// repeated in a call simply sees pow(m, 0) == 1 the second time.  With the
// option on and momentum 0 the reference reads a null array; here the call is
// refused (false, orc_last_error) and changes nothing.
// ---------------------------------------------------------------------------
struct Sgd {
    float lr = 1e-3f, momentum = 0.f, weight_decay = 0.f, dampening = 0.f;
    bool nesterov = false, maximize = false, smart = false;
    uint32_t iter = 0;
    std::mutex mu;
    std::unordered_map<std::string, std::vector<float>> b;
    std::unordered_map<std::string, std::vector<uint32_t>> last;
};

bool sgd_apply(Sgd *o, const std::string &name, float *param, uint32_t param_len, const float *g_in,
               const uint32_t *gidx, uint32_t glen) {
    if (o->smart && o->momentum == 0.f) return false;  // no last-touched array exists
    bool first = false;
    float *pb = nullptr;
    uint32_t *pl = nullptr;
    {
        std::lock_guard<std::mutex> g(o->mu);
        if (o->momentum != 0.f && o->b.find(name) == o->b.end()) {
            o->b[name].assign(param_len, 0.f);
            o->last[name].assign(param_len, 0u);
            first = true;
        }
        if (o->momentum != 0.f) pb = o->b[name].data();
        if (o->smart) pl = o->last[name].data();
    }
    const double lr = o->maximize ? -static_cast<double>(o->lr) : static_cast<double>(o->lr);
    for (uint32_t i = 0; i < glen; ++i) {
        const uint32_t id = gidx[i];
        const float x = param[id];
        float g = g_in[i];
        float m = o->momentum;
        if (o->smart && o->iter != 0)
            m = static_cast<float>(std::pow(static_cast<double>(o->momentum), static_cast<double>(o->iter - pl[id])));
        if (o->weight_decay != 0.f) g = std::fmaf(o->weight_decay, x, g);
        if (o->momentum != 0.f) {
            float bnew;
            if (!first) bnew = std::fmaf(pb[id], m, (1.f - o->dampening) * g);
            else bnew = g;
            if (o->nesterov) g = std::fmaf(m, bnew, g);
            else g = bnew;
            pb[id] = bnew;
        }
        param[id] = static_cast<float>(std::fma(-lr, static_cast<double>(g), static_cast<double>(x)));
        if (o->smart) pl[id] = o->iter;
    }
    o->iter++;
    return true;
}

// ---------------------------------------------------------------------------
// Sparse Adam (optim/adam.cpp:19-86; defaults adam.h:21-23, lr sparse_optimizer.h:30).
// Per-name state: m, v zero-filled arrays of param_len, a float vmax (0) and a
// uint32 tick (1), incremented after every call (adam.cpp:28-35, 81-82).
// Arithmetic as GCC 11 -O3 -march=broadwell emits it (objdump of adam.o):
//   b1pow = pow((double)b1, (double)tick), c1 = 1 - b1pow  (likewise b2)  :42-43,67-68
//   maximize: g = -g; wd != 0: g = fmaf(wd, x, g)           (vfmadd231ss) :56-62
//   mt = fmaf(b1, m, (1-b1)*g)   vt = fmaf(b2, v, ((1-b2)*g)*g)  (float)  :64-65
//   mt_hat = (double)mt / c1     vt_hat = (double)vt / c2                  :67-68
//   amsgrad: vmax = vt_hat > (double)vmax ? (float)vt_hat : vmax  (running over i)
//            x' = (float)(x - lr*mt_hat / (double)(sqrtf(vmax) + eps))     :70-72
//   else:    x' = (float)(x - lr*mt_hat / ((double)eps + sqrt(vt_hat)))    :74
// ---------------------------------------------------------------------------
struct Adam {
    float lr = 1e-3f, b1 = 0.9f, b2 = 0.999f, weight_decay = 0.f, eps = 1e-8f;
    bool amsgrad = false, maximize = false;
    struct St {
        std::vector<float> m, v;
        float vmax = 0.f;
        uint32_t tick = 1;
    };
    std::mutex mu;
    std::unordered_map<std::string, St> st;
};

void adam_apply(Adam *o, const std::string &name, float *param, uint32_t param_len, const float *g_in,
                const uint32_t *gidx, uint32_t glen) {
    Adam::St *s;
    {
        std::lock_guard<std::mutex> g(o->mu);
        auto it = o->st.find(name);
        if (it == o->st.end()) {
            it = o->st.emplace(name, Adam::St()).first;
            it->second.m.assign(param_len, 0.f);
            it->second.v.assign(param_len, 0.f);
        }
        s = &it->second;
    }
    const double c1 = 1.0 - std::pow(static_cast<double>(o->b1), static_cast<double>(s->tick));
    const double c2 = 1.0 - std::pow(static_cast<double>(o->b2), static_cast<double>(s->tick));
    const double lr = o->lr;
    float vmax = s->vmax;
    for (uint32_t i = 0; i < glen; ++i) {
        const uint32_t id = gidx[i];
        const float x = param[id];
        float g = g_in[i];
        if (o->maximize) g = -g;
        if (o->weight_decay != 0.f) g = std::fmaf(o->weight_decay, x, g);
        const float a = (1.f - o->b1) * g;
        const float mt = std::fmaf(o->b1, s->m[id], a);
        const float bq = ((1.f - o->b2) * g) * g;
        const float vt = std::fmaf(o->b2, s->v[id], bq);
        const double num = (static_cast<double>(mt) / c1) * lr;
        const double vt_hat = static_cast<double>(vt) / c2;
        double den;
        if (o->amsgrad) {
            if (vt_hat > static_cast<double>(vmax)) vmax = static_cast<float>(vt_hat);
            den = static_cast<double>(std::sqrt(vmax) + o->eps);
        } else {
            den = static_cast<double>(o->eps) + std::sqrt(vt_hat);
        }
        param[id] = static_cast<float>(static_cast<double>(x) - num / den);
        s->m[id] = mt;
        s->v[id] = vt;
    }
    s->vmax = vmax;
    s->tick++;
}

// ---------------------------------------------------------------------------
// Wire format of the compressed stream (engine/comm_manager.cpp).  queueTx
// (:573-590) sets COMM_FLAG_UINT16_IDX (0x01) when tensor_numel < 65536
// (IDX_COMPRESSION 1, config.h:63) and COMM_FLAG_FP16_VAL (0x02) under
// FP16_COMPRESSION (0 in config.h:64, i.e. compiled out as shipped).  The casts
// run 8-wide SIMD blocks while i + 8 < length, then a scalar tail, and the two
// halves differ (the SIMD path is what the x86 instruction defines):
//   u32->u16 (:509-528): blocks _mm_packs_epi32 = signed saturation of the
//            int32 to int16 (idx >= 32768 -> 0x7FFF); tail (uint16_t) truncation.
//   u16->u32 (:486-505): blocks _mm256_cvtepi16_epi32 = SIGN extension; tail
//            zero extension.
//   f32->f16 (:530-548): blocks _mm256_cvtps_ph(v, 0) = IEEE binary16, round
//            to nearest even; tail `dst[i] = src[i]` with fp16_t = uint16_t
//            (comm_manager.h:27), i.e. GCC's vcvttss2si to int32 (truncation,
//            out of range / NaN -> 0x80000000) stored as the low 16 bits.
//   f16->f32 (:550-567): blocks _mm256_cvtph_ps (exact; a signalling NaN
//            comes out quiet, payload kept); tail the integer value of the
//            uint16 converted to float.
// tests/test_wire_isa_host.py pins all of this to the instructions themselves
// (oracle/isa_wire.cpp) on every binary16 word and rounding boundary.
// ---------------------------------------------------------------------------
size_t wire_simd_end(size_t len) { return len ? 8 * ((len - 1) / 8) : 0; }

uint16_t f32_to_f16_rne(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const uint32_t ex = (u >> 23) & 0xffu;
    uint32_t man = u & 0x7fffffu;
    if (ex == 0xffu) return static_cast<uint16_t>(sign | 0x7c00u | (man ? 0x200u | (man >> 13) : 0u));
    const int e = static_cast<int>(ex) - 127 + 15;
    if (e >= 31) return static_cast<uint16_t>(sign | 0x7c00u);
    if (e <= 0) {  // binary16 subnormal (or zero)
        if (e < -10) return static_cast<uint16_t>(sign);
        man |= 0x800000u;
        const uint32_t shift = static_cast<uint32_t>(14 - e);
        uint32_t h = man >> shift;
        const uint32_t rem = man & ((1u << shift) - 1u), half = 1u << (shift - 1);
        if (rem > half || (rem == half && (h & 1u))) ++h;
        return static_cast<uint16_t>(sign | h);
    }
    uint32_t h = (static_cast<uint32_t>(e) << 10) | (man >> 13);
    const uint32_t rem = man & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;  // may carry into the exponent (-> inf)
    return static_cast<uint16_t>(sign | h);
}

float f16_to_f32(uint16_t h) {
    const uint32_t sign = static_cast<uint32_t>(h & 0x8000u) << 16;
    uint32_t ex = (h >> 10) & 0x1fu, man = h & 0x3ffu, u;
    if (ex == 0x1fu) u = sign | 0x7f800000u | (man ? 0x00400000u | (man << 13) : 0u);  // a NaN widens quiet
    else if (ex) u = sign | ((ex + 112u) << 23) | (man << 13);
    else if (!man) u = sign;
    else {
        int e = -1;
        do { man <<= 1; ++e; } while (!(man & 0x400u));
        u = sign | ((112u - static_cast<uint32_t>(e)) << 23) | ((man & 0x3ffu) << 13);
    }
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

uint16_t f32_to_u16_trunc(float f) {  // vcvttss2si r32 + 16-bit store
    int32_t t = INT32_MIN;
    if (f == f && f > -2147483904.0f && f < 2147483648.0f) t = static_cast<int32_t>(f);
    return static_cast<uint16_t>(static_cast<uint32_t>(t) & 0xffffu);
}

thread_local std::string g_err;

}  // namespace

// ===========================================================================
// C ABI of the oracle (consumed by tests/ and bench.py's cpu_baseline only)
// ===========================================================================

ORC_API void orc_synth_fill(float *dst, size_t n, uint64_t seed, int dist, uint32_t param) {
    // dist 0: D1 Irwin-Hall(4) of 24-bit uniforms, centred, * 2^-24 * 1e-3
    // dist 1: D2 = D1 * 2^-e, e = U{0..8}
    // dist 2: D3 = D1 with zeros; param = zero probability in units of 1e-4
    const double scale = 1e-3 / 16777216.0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t base = seed * 0x100000001B3ull + static_cast<uint64_t>(i) * 4u;
        const uint64_t r0 = splitmix64(base + 0), r1 = splitmix64(base + 1);
        const int64_t v = static_cast<int64_t>(r0 & 0xFFFFFF) + static_cast<int64_t>((r0 >> 24) & 0xFFFFFF) +
                          static_cast<int64_t>(r1 & 0xFFFFFF) + static_cast<int64_t>((r1 >> 24) & 0xFFFFFF) -
                          (int64_t{1} << 25);
        double x = static_cast<double>(v) * scale;
        if (dist == 1) {
            const uint32_t e = static_cast<uint32_t>((r1 >> 48) % 9u);
            x = std::ldexp(x, -static_cast<int>(e));
        } else if (dist == 2) {
            const uint32_t z = static_cast<uint32_t>((r0 >> 48) % 10000u);
            if (z < param) x = 0.0;
        }
        dst[i] = static_cast<float>(x);
    }
}

ORC_API const char *orc_last_error(void) { return g_err.c_str(); }

// --- thresholdv16 ---
ORC_API void *orc_tv16_new(void) { return new Tv16(); }
ORC_API void orc_tv16_free(void *h) { delete static_cast<Tv16 *>(h); }
ORC_API size_t orc_tv16_compress(void *h, const char *name, const float *src, size_t n, uint32_t k,
                                 uint32_t *idx, size_t idx_cap, float *val, int32_t idx_offset) {
    return tv16_compress(static_cast<Tv16 *>(h), name, src, n, k, idx, idx_cap, val, idx_offset);
}
ORC_API int orc_tv16_state(void *h, const char *name, float *t, float *inc) {
    auto *p = static_cast<Tv16 *>(h);
    std::lock_guard<std::mutex> g(p->mu);
    auto it = p->st.find(name);
    if (it == p->st.end()) return -1;
    *t = it->second.t;
    *inc = it->second.inc;
    return 0;
}
ORC_API float orc_tv16_first_threshold(const float *src, size_t n, uint32_t k) {
    return tv16_first_threshold(src, n, k);
}
ORC_API void orc_tv16_block_sums(const float *src, size_t n, float *out) {
    for (size_t j = 0; j < n / kLine; ++j) out[j] = block_tree_sum(src + j * kLine);
}

// --- threshold-v (state keyed by the caller's src pointer in the reference;
//     here the key is explicit so tests can emulate the engine's two buffers) ---
ORC_API void *orc_tv_new(void) { return new Tv(); }
ORC_API void orc_tv_free(void *h) { delete static_cast<Tv *>(h); }
ORC_API size_t orc_tv_compress(void *h, uint64_t key, const float *src, size_t n, uint32_t k,
                               uint32_t *idx, size_t cap, float *val) {
    return tv_compress(static_cast<Tv *>(h), key, src, n, k, idx, cap, val);
}
ORC_API int orc_tv_state(void *h, uint64_t key, float *t) {
    auto *p = static_cast<Tv *>(h);
    std::lock_guard<std::mutex> g(p->mu);
    auto it = p->st.find(key);
    if (it == p->st.end()) return -1;
    *t = it->second;
    return 0;
}
ORC_API float orc_tv_first_threshold(const float *src, size_t n, uint32_t k) {
    return tv_first_threshold(src, n, k);
}

// --- top-k (topk.cpp:28-46).  bug_compat=1 reproduces the byte-count memcpy
//     (only n bytes = n/4 floats survive) and idx = 0..k-1, in libstdc++
//     nth_element partition order; bug_compat=0 is the intended top-k by |x|
//     over the whole bucket with real indices (+idx_offset), index-ordered. ---
ORC_API int64_t orc_topk_compress(const float *src, size_t n, uint32_t k, uint32_t *idx, size_t cap,
                                  float *val, int32_t idx_offset, int bug_compat) {
    if (cap < k) { g_err = "Invalid parameter k"; return -1; }
    if (bug_compat) {
        std::vector<float> c(n, 0.f);
        std::memcpy(c.data(), src, n);  // sic: bytes, not floats (topk.cpp:31)
        std::nth_element(c.begin(), c.begin() + std::min<size_t>(k, n), c.end(),
                         [](float a, float b) { return std::fabs(a) > std::fabs(b); });
        for (uint32_t i = 0; i < k; ++i) { idx[i] = i; val[i] = c[i]; }
        return static_cast<int64_t>(cap);
    }
    std::vector<uint32_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = static_cast<uint32_t>(i);
    // rank by |x| desc, ties by index asc; emit the k winners in index order
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return std::fabs(src[a]) > std::fabs(src[b]); });
    std::vector<uint32_t> win(order.begin(), order.begin() + std::min<size_t>(k, n));
    std::sort(win.begin(), win.end());
    for (size_t i = 0; i < win.size(); ++i) {
        idx[i] = win[i] + static_cast<uint32_t>(idx_offset);
        val[i] = src[win[i]];
    }
    return static_cast<int64_t>(cap);
}

// --- MERGE caller arithmetic (compress.cpp:44,52) and API k (core.cpp:1216) ---
ORC_API int64_t orc_merge_numel(int64_t n, double ratio, int world) {
    // compression_ratio_ is double (core.h:96), world is cast to float, the
    // quotient is stored in a float, and size_t * float is a float product.
    const float kf = static_cast<float>((1 - ratio) / static_cast<float>(world));
    const int64_t lo = std::min<int64_t>(n, 1);
    return std::max<int64_t>(lo, static_cast<int64_t>(static_cast<float>(n) * kf));
}
ORC_API int64_t orc_api_numel(int64_t n, float ratio) {
    return static_cast<int64_t>((1. - static_cast<double>(ratio)) * static_cast<double>(n));
}

// --- MERGE decompress (cpu_optimize.cpp:40-72): per-rank dense scatter
//     (index_put_, no accumulate), rank-order sum, /world, unique union of
//     indices, gather.  Output is sorted by index (the reference's
//     unordered_set order is unspecified; SGD is per-index so order is moot). ---
ORC_API size_t orc_merge_decompress(const uint32_t *idx, const float *val, size_t per_rank, int world,
                                    size_t n, uint32_t *out_idx, float *out_val) {
    std::vector<float> merged(n, 0.f);
    std::vector<float> tmp(n);
    std::vector<char> seen(n, 0);
    for (int r = 0; r < world; ++r) {
        std::fill(tmp.begin(), tmp.end(), 0.f);
        for (size_t i = 0; i < per_rank; ++i) tmp[idx[r * per_rank + i]] = val[r * per_rank + i];
        for (size_t i = 0; i < n; ++i) merged[i] += tmp[i];
        for (size_t i = 0; i < per_rank; ++i) seen[idx[r * per_rank + i]] = 1;
    }
    const float w = static_cast<float>(world);
    size_t m = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!seen[i]) continue;
        out_idx[m] = static_cast<uint32_t>(i);
        out_val[m] = merged[i] / w;
        ++m;
    }
    return m;
}

// --- sparse SGD ---
ORC_API void *orc_sgd_new(float lr, float momentum, float dampening, float weight_decay, int nesterov,
                          int maximize) {
    auto *o = new Sgd();
    o->lr = lr; o->momentum = momentum; o->dampening = dampening; o->weight_decay = weight_decay;
    o->nesterov = nesterov != 0; o->maximize = maximize != 0;
    return o;
}
ORC_API void orc_sgd_free(void *o) { delete static_cast<Sgd *>(o); }
ORC_API int orc_sgd_apply(void *o, const char *name, float *param, uint32_t param_len, const float *g,
                          const uint32_t *gidx, uint32_t glen) {
    if (sgd_apply(static_cast<Sgd *>(o), name, param, param_len, g, gidx, glen)) return 0;
    g_err = "smart_momentum needs momentum != 0";
    return -1;
}
ORC_API void orc_sgd_smart(void *o, int on) { static_cast<Sgd *>(o)->smart = on != 0; }
ORC_API uint32_t orc_sgd_iter(void *o) { return static_cast<Sgd *>(o)->iter; }
ORC_API int orc_sgd_last(void *o, const char *name, uint32_t *out, uint32_t len) {
    auto *p = static_cast<Sgd *>(o);
    std::lock_guard<std::mutex> g(p->mu);
    auto it = p->last.find(name);
    if (it == p->last.end()) return -1;
    std::memcpy(out, it->second.data(), sizeof(uint32_t) * std::min<size_t>(len, it->second.size()));
    return 0;
}
ORC_API int orc_sgd_momentum(void *o, const char *name, float *out, uint32_t len) {
    auto *p = static_cast<Sgd *>(o);
    std::lock_guard<std::mutex> g(p->mu);
    auto it = p->b.find(name);
    if (it == p->b.end()) return -1;
    std::memcpy(out, it->second.data(), sizeof(float) * std::min<size_t>(len, it->second.size()));
    return 0;
}

// --- sparse Adam ---
ORC_API void *orc_adam_new(float lr, float b1, float b2, float eps, float weight_decay, int amsgrad, int maximize) {
    auto *o = new Adam();
    o->lr = lr; o->b1 = b1; o->b2 = b2; o->eps = eps; o->weight_decay = weight_decay;
    o->amsgrad = amsgrad != 0; o->maximize = maximize != 0;
    return o;
}
ORC_API void orc_adam_free(void *o) { delete static_cast<Adam *>(o); }
ORC_API void orc_adam_apply(void *o, const char *name, float *param, uint32_t param_len, const float *g,
                            const uint32_t *gidx, uint32_t glen) {
    adam_apply(static_cast<Adam *>(o), name, param, param_len, g, gidx, glen);
}
ORC_API int orc_adam_state(void *o, const char *name, float *m, float *v, uint32_t len, float *vmax) {
    auto *p = static_cast<Adam *>(o);
    std::lock_guard<std::mutex> g(p->mu);
    auto it = p->st.find(name);
    if (it == p->st.end()) return -1;
    const size_t c = std::min<size_t>(len, it->second.m.size());
    std::memcpy(m, it->second.m.data(), sizeof(float) * c);
    std::memcpy(v, it->second.v.data(), sizeof(float) * c);
    *vmax = it->second.vmax;
    return static_cast<int>(it->second.tick);
}

// --- wire format (engine/comm_manager.cpp) ---
ORC_API uint8_t orc_wire_flag(uint64_t tensor_numel, int fp16_values) {
    return static_cast<uint8_t>((tensor_numel < 65536 ? 0x01 : 0) | (fp16_values ? 0x02 : 0));
}
ORC_API void orc_wire_encode(const uint32_t *idx, const float *val, size_t len, uint8_t flag, void *idx_out,
                             void *val_out) {
    const size_t se = wire_simd_end(len);
    for (size_t i = 0; i < len; ++i) {
        if (flag & 0x01) {
            uint16_t w;
            if (i < se) {
                const int32_t v = static_cast<int32_t>(idx[i]);
                w = static_cast<uint16_t>(v > 32767 ? 32767 : (v < -32768 ? -32768 : v));
            } else {
                w = static_cast<uint16_t>(idx[i]);
            }
            static_cast<uint16_t *>(idx_out)[i] = w;
        } else {
            static_cast<uint32_t *>(idx_out)[i] = idx[i];
        }
        if (flag & 0x02)
            static_cast<uint16_t *>(val_out)[i] = i < se ? f32_to_f16_rne(val[i]) : f32_to_u16_trunc(val[i]);
        else
            static_cast<float *>(val_out)[i] = val[i];
    }
}
ORC_API void orc_wire_decode(const void *idx_in, const void *val_in, size_t len, uint8_t flag, uint32_t *idx,
                             float *val) {
    const size_t se = wire_simd_end(len);
    for (size_t i = 0; i < len; ++i) {
        if (flag & 0x01) {
            const uint16_t w = static_cast<const uint16_t *>(idx_in)[i];
            idx[i] = i < se ? static_cast<uint32_t>(static_cast<int32_t>(static_cast<int16_t>(w))) : w;
        } else {
            idx[i] = static_cast<const uint32_t *>(idx_in)[i];
        }
        if (flag & 0x02) {
            const uint16_t h = static_cast<const uint16_t *>(val_in)[i];
            val[i] = i < se ? f16_to_f32(h) : static_cast<float>(h);
        } else {
            val[i] = static_cast<const float *>(val_in)[i];
        }
    }
}

// --- intra-node gather-add (engine/modules/cpu_gather.cpp:59-87) ---
// Local rank r of N owns [len*r/N, len*(r+1)/N) of grad[0] and adds, in order,
// the residual and grad[1] .. grad[N-1] into it; add_arrays
// (misc/array_util.h:12-54) is a plain per-element dst += src in every path.
ORC_API void orc_gather_slice(int64_t len, int local_rank, int num_gpus, int64_t *start, int64_t *end) {
    *start = (len * local_rank) / num_gpus;
    *end = (len * (local_rank + 1)) / num_gpus;
}
ORC_API void orc_gather_add(float *grad0, const float *resid, const float *const *grads, int num_gpus, int64_t len,
                            int local_rank) {
    int64_t a, b;
    orc_gather_slice(len, local_rank, num_gpus, &a, &b);
    for (int i = 0; i < num_gpus; ++i) {
        const float *src = i == 0 ? resid : grads[i];
        for (int64_t j = a; j < b; ++j) grad0[j] += src[j];
    }
}
