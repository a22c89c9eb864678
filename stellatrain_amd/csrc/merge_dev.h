// merge_dev.h -- per-element device code of the MERGE decompress emission and
// the optimizer steps fused into it, shared by the per-tensor kernels
// (apply.hip) and the batched ones (merge_batch.hip, merge_batch_world.hip):
// one text, so they agree bitwise.  gfx950 only.
#pragma once

#include <algorithm>

#include "ws.h"
#include "wire_dev.h"

namespace stg {

// WIRE: the lane's WP pairs (e % 4 == 0, WP % 4 == 0) of a received stream,
// four at a time (wire_dev.h: an 8-byte load of the 16-bit form where the four
// exist and are aligned, clamped single loads otherwise).
template <uint32_t WP>
__device__ __forceinline__ void wire_idx_wp(const void *idx, uint32_t flag, size_t wend, size_t m, size_t e,
                                            uint32_t (&j)[WP]) {
    static_assert(WP % 4 == 0, "groups of four pairs");
#pragma unroll
    for (uint32_t q = 0; q < WP / 4; ++q) wire_get_idx4(idx, flag, wend, m, e + 4 * q, &j[4 * q]);
}
template <uint32_t WP>
__device__ __forceinline__ void wire_val_wp(const void *val, uint32_t flag, size_t wend, size_t m, size_t e,
                                            float (&v)[WP]) {
    static_assert(WP % 4 == 0, "groups of four pairs");
#pragma unroll
    for (uint32_t q = 0; q < WP / 4; ++q) wire_get_val4(val, flag, wend, m, e + 4 * q, &v[4 * q]);
}

// The lane's WP pairs e .. e+WP-1: their indices, and which of them win (bit b).
// Every load is issued before any is used -- the index loads together, then
// the winner words (clamped addresses, results masked) -- two round trips per
// lane instead of 2 WP dependent ones.
template <uint32_t WP, bool WIRE = false>
__device__ __forceinline__ uint32_t win_keep_t(const uint32_t *__restrict__ idx, size_t m, size_t n,
                                               const uint32_t *__restrict__ win, size_t e, uint32_t (&j)[WP],
                                               uint32_t flag = 0, size_t wend = 0) {
    if (WIRE) {
        wire_idx_wp<WP>(idx, flag, wend, m, e, j);
    } else if (WP % 4 == 0 && e + WP <= m && (reinterpret_cast<uintptr_t>(idx + e) & 15u) == 0) {
        const uint4 *p = reinterpret_cast<const uint4 *>(idx + e);
#pragma unroll
        for (uint32_t q = 0; q < WP / 4; ++q) {
            const uint4 v = p[q];
            j[4 * q] = v.x; j[4 * q + 1] = v.y; j[4 * q + 2] = v.z; j[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (uint32_t b = 0; b < WP; ++b) j[b] = idx[std::min<size_t>(e + b, m - 1)];
    }
    uint32_t w[WP];
#pragma unroll
    for (uint32_t b = 0; b < WP; ++b) w[b] = win[j[b] < n ? j[b] : 0u];
    uint32_t keep = 0;
#pragma unroll
    for (uint32_t b = 0; b < WP; ++b)
        if (e + b < m && j[b] < n && w[b] == (uint32_t)(e + b) + 1u) keep |= 1u << b;
    return keep;
}

// SGD::optimize_raw on one element (optim/sgd.cpp:34-263, scalar path), with
// param[id] = x and mom[id] = m loaded by the caller: the same expression as
// sgd_apply, so a step fused into the emission agrees with it bitwise.
//
// SMART (smart momentum, sgd.cpp:225-232, 258-259): `f` stands where the
// momentum stands, f = sgd_factor(a, last[id]); an element whose factor is
// outside [0, 1) -- the reference's assertion: the index was already touched
// in this call -- is skipped and flagged.
template <bool SMART>
__device__ __forceinline__ float sgd_factor(const SgdLaunch &a, uint32_t last) {
    if (!SMART || a.iter == 0) return a.momentum;
    const uint32_t d = a.iter - last;
    return a.pow_tab[d < a.pow_len ? d : a.pow_len - 1];  // past the table: its last entry, 0
}

template <bool SMART>
__device__ __forceinline__ void sgd_step(const SgdLaunch &a, uint32_t id, float g, float x, float m, float f,
                                         uint32_t last) {
    if (SMART && a.iter != 0 && last == a.iter) {
        g_or(a.fail, SGD_FAIL_FACTOR);
        return;
    }
    if (a.weight_decay != 0.f) g = fmaf(a.weight_decay, x, g);
    if (a.mom) {
        const float b = a.first ? g : fmaf(m, f, (1.0f - a.dampening) * g);
        g = a.nesterov ? fmaf(f, b, g) : b;
        a.mom[id] = b;
    }
    a.param[id] = (float)fma(-a.lr, (double)g, (double)x);
    if (SMART) a.last[id] = a.iter;
}

// Adam::optimize_raw on one element (optim/adam.cpp:19-86, no amsgrad), with
// param[id] = x, m[id] = m0, v[id] = v0 loaded by the caller: the expressions of
// adam_elem / adam_apply below, so a fused step agrees with them bitwise.
__device__ __forceinline__ void adam_step(const AdamLaunch &a, uint32_t id, float g, float x, float m0, float v0) {
    if (a.maximize) g = -g;
    if (a.weight_decay != 0.f) g = fmaf(a.weight_decay, x, g);
    const float mt = fmaf(a.b1, m0, (1.f - a.b1) * g);
    const float vt = fmaf(a.b2, v0, ((1.f - a.b2) * g) * g);
    const double num = ((double)mt / a.c1) * a.lr;
    const double vt_hat = (double)vt / a.c2;
    a.param[id] = (float)((double)x - num / ((double)a.eps + sqrt(vt_hat)));
    a.m[id] = mt;
    a.v[id] = vt;
}

// One emitted pair's optimizer step in a batched launch: sgd_step / adam_step
// on the launch structure rebuilt from the handle-wide scalars of the launch's
// table `w` (w.sgd / w.adam) and the tensor's fields `d` (param, n, s0, s1, u:
// MergeTensor, MergeWorldTensor).  OPT: 0 = SGD, 1 = SGD with smart momentum,
// 2 = Adam (no amsgrad).
template <int OPT>
struct Step;
template <>
struct Step<2> {
    AdamLaunch a;
    template <class W, class D>
    __device__ __forceinline__ Step(const W &w, const D &d) : a(w.adam) {
        a.param = d.param;
        a.param_len = d.n;
        a.m = d.s0;
        a.v = static_cast<float *>(d.s1);
        a.c1 = d.u.adam.c1;
        a.c2 = d.u.adam.c2;
    }
    __device__ __forceinline__ void load(uint32_t id, float &x, float &m, float &v, uint32_t &l) const {
        x = a.param[id];
        m = a.m[id];
        v = a.v[id];
        l = 0u;
    }
    __device__ __forceinline__ void factors(float &, uint32_t) const {}
    __device__ __forceinline__ void step(uint32_t id, float g, float x, float m, float v, uint32_t) const {
        adam_step(a, id, g, x, m, v);
    }
};
template <int OPT>
struct Step {
    static constexpr bool SMART = OPT == 1;
    SgdLaunch a;
    template <class W, class D>
    __device__ __forceinline__ Step(const W &w, const D &d) : a(w.sgd) {
        a.param = d.param;
        a.param_len = d.n;
        a.mom = d.s0;
        a.last = static_cast<uint32_t *>(d.s1);
        a.iter = d.u.sgd.iter;
        a.first = d.u.sgd.first != 0;
    }
    __device__ __forceinline__ void load(uint32_t id, float &x, float &m, float &, uint32_t &l) const {
        x = a.param[id];
        m = a.mom ? a.mom[id] : 0.f;
        l = SMART ? a.last[id] : 0u;
    }
    // SMART: the winners' factors, gathered from the table together (else the momentum)
    __device__ __forceinline__ void factors(float &f, uint32_t l) const { f = sgd_factor<SMART>(a, l); }
    __device__ __forceinline__ void step(uint32_t id, float g, float x, float m, float f, uint32_t l) const {
        sgd_step<SMART>(a, id, g, x, m, f, l);
    }
};

// world > 1: a lane's 16 mark bytes at e (one 16-byte load where all exist;
// the array starts 16-byte aligned and e % 16 == 0), and how many bytes of a
// word of them are set.
__device__ __forceinline__ uint32_t nz_bytes(uint32_t w) {
    uint32_t c = 0;
    c += (w & 0xffu) != 0;
    c += (w & 0xff00u) != 0;
    c += (w & 0xff0000u) != 0;
    c += (w & 0xff000000u) != 0;
    return c;
}

__device__ __forceinline__ uint4 load_marks(const uint8_t *mark, size_t n, size_t e) {
    if (e + 16 <= n) return *reinterpret_cast<const uint4 *>(mark + e);
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t b = 0; b < 16; ++b)
        if (e + b < n) w[b >> 2] |= (uint32_t)mark[e + b] << (8 * (b & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace stg
