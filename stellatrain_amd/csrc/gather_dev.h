// gather_dev.h -- the per-lane body of the intra-node gather-add, shared by
// gather.hip and send_batch.hip (gfx950 only).
//
// ModuleCpuGather::run (engine/modules/cpu_gather.cpp:59-87) per element:
//   acc = term0; if residual: acc += residual[e]; for s = 1 .. N-1: acc +=
//   widen(src[s][e]); dst[e] = acc
// A is GatherArgs or SendGather (ws.h: dst, resid, src[], nsrc, dtypes).
// The fp32 in-place form (gather_elem<false>; its float4 lane is written out
// in the two fp32 kernels): every source is float, term0 is dst[e], a.src[0]
// and a.dtypes are not looked at.  The typed form (gather_lane,
// gather_elem<true>) reads source s as the STG_DT_* type in bits 2 s, 2 s + 1
// of a.dtypes -- a kernel-argument word, so the type switch is a wave-uniform
// branch, not a table load -- and takes term0 from a.src[0] when that is not
// null (dst is then write-only).
// Widening is exact: bf16 is bits << 16, fp16 is v_cvt_f32_f16 in the default
// mode (subnormals kept, -0 keeps its sign, a NaN stays a NaN) -- the values
// wire_dev.h's f16_to_f32 gives on every non-NaN word.
#pragma once

#include <stdint.h>

#include "common.h"

namespace stg {

typedef float gd_f4v __attribute__((ext_vector_type(4)));
typedef uint32_t gd_u4v __attribute__((ext_vector_type(4)));
typedef uint32_t gd_u2v __attribute__((ext_vector_type(2)));

constexpr uint32_t GATHER_F32 = 0, GATHER_BF16 = 1, GATHER_F16 = 2;  // = STG_DT_*

// the 16-bit word h (bits above 15 clear) of type dt != GATHER_F32 as a float
__device__ __forceinline__ float gather_widen16(uint32_t dt, uint32_t h) {
    if (dt == GATHER_BF16) return u2f(h << 16);
    return (float)__builtin_bit_cast(_Float16, (uint16_t)h);
}

__device__ __forceinline__ float gather_load1(const void *p, uint32_t dt, size_t e) {
    if (dt == GATHER_F32) return static_cast<const float *>(p)[e];
    return gather_widen16(dt, static_cast<const uint16_t *>(p)[e]);
}

// One element, every pointer at any element-aligned address.
template <bool TYPED, class A>
__device__ __forceinline__ void gather_elem(const A &a, size_t e) {
    float acc = TYPED && a.src[0] ? gather_load1(a.src[0], a.dtypes & 3u, e) : a.dst[e];
    if (a.resid) acc += a.resid[e];
    for (uint32_t s = 1; s < a.nsrc; ++s)
        acc += TYPED ? gather_load1(a.src[s], (a.dtypes >> (2 * s)) & 3u, e) : static_cast<const float *>(a.src[s])[e];
    a.dst[e] = acc;
}

// W consecutive elements of a source as loaded: W floats, or W 16-bit words in
// the first W / 2 dwords.  Nontemporal: a source is read once.
template <uint32_t W>
__device__ __forceinline__ void gather_load_raw(const void *p, uint32_t dt, size_t e, uint32_t (&w)[W]) {
    if (dt == GATHER_F32) {
        const gd_u4v *q = reinterpret_cast<const gd_u4v *>(static_cast<const float *>(p) + e);
#pragma unroll
        for (uint32_t j = 0; j < W / 4; ++j) {
            const gd_u4v v = __builtin_nontemporal_load(q + j);
            w[4 * j] = v.x, w[4 * j + 1] = v.y, w[4 * j + 2] = v.z, w[4 * j + 3] = v.w;
        }
    } else if (W == 8) {
        const gd_u4v v = __builtin_nontemporal_load(reinterpret_cast<const gd_u4v *>(static_cast<const uint16_t *>(p) + e));
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
        const gd_u2v v = __builtin_nontemporal_load(reinterpret_cast<const gd_u2v *>(static_cast<const uint16_t *>(p) + e));
        w[0] = v.x, w[1] = v.y;
    }
}

template <uint32_t W>
__device__ __forceinline__ void gather_add_raw(float (&acc)[W], uint32_t dt, const uint32_t (&w)[W], bool first) {
#pragma unroll
    for (uint32_t j = 0; j < W; ++j) {
        const float x = dt == GATHER_F32 ? u2f(w[j]) : gather_widen16(dt, (w[j / 2] >> (16 * (j & 1u))) & 0xffffu);
        acc[j] = first ? x : acc[j] + x;
    }
}

// The typed lane, W = 4 or 8 consecutive elements from e on: dst, the residual
// and every fp32 source 16-byte aligned there, every 16-bit source 2 W bytes
// aligned.  MAXS >= a.nsrc.  Every stream's vector is loaded before any is
// added (a loop of load-then-add waited for each load in turn), then the sum
// runs in the reference's order.
template <uint32_t MAXS, uint32_t W, class A>
__device__ __forceinline__ void gather_lane(const A &a, size_t e) {
    static_assert(W == 4 || W == 8, "one or two float4 per fp32 stream");
    uint32_t x[MAXS][W];
    float acc[W], r[W];
    const bool t0 = a.src[0] != nullptr;
    if (t0) {
        gather_load_raw<W>(a.src[0], a.dtypes & 3u, e, x[0]);
    } else {
#pragma unroll
        for (uint32_t j = 0; j < W / 4; ++j) {
            const gd_f4v v = *reinterpret_cast<const gd_f4v *>(a.dst + e + 4 * j);
            acc[4 * j] = v.x, acc[4 * j + 1] = v.y, acc[4 * j + 2] = v.z, acc[4 * j + 3] = v.w;
        }
    }
    if (a.resid) {
#pragma unroll
        for (uint32_t j = 0; j < W / 4; ++j) {
            const gd_f4v v = __builtin_nontemporal_load(reinterpret_cast<const gd_f4v *>(a.resid + e + 4 * j));
            r[4 * j] = v.x, r[4 * j + 1] = v.y, r[4 * j + 2] = v.z, r[4 * j + 3] = v.w;
        }
    }
#pragma unroll
    for (uint32_t s = 1; s < MAXS; ++s)
        if (s < a.nsrc) gather_load_raw<W>(a.src[s], (a.dtypes >> (2 * s)) & 3u, e, x[s]);
    if (t0) gather_add_raw<W>(acc, a.dtypes & 3u, x[0], true);
    if (a.resid) {
#pragma unroll
        for (uint32_t j = 0; j < W; ++j) acc[j] += r[j];
    }
#pragma unroll
    for (uint32_t s = 1; s < MAXS; ++s)
        if (s < a.nsrc) gather_add_raw<W>(acc, (a.dtypes >> (2 * s)) & 3u, x[s], false);
#pragma unroll
    for (uint32_t j = 0; j < W / 4; ++j)
        *reinterpret_cast<gd_f4v *>(a.dst + e + 4 * j) = gd_f4v{acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]};
}

}  // namespace stg
