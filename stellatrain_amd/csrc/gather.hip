// gather.hip -- intra-node gather-add before the codec (gfx950).
//
// ModuleCpuGather::run (engine/modules/cpu_gather.cpp:59-87): local rank r of
// N owns the slice [len*r/N, len*(r+1)/N) of grad[0] and adds into it, in
// order, the residual and grad[1] .. grad[N-1] with add_arrays
// (misc/array_util.h:12-54, a plain per-element dst += src).  Here the N - 1
// sources are device pointers -- this GPU's buffers or peers' over xGMI (P2P
// enabled or IPC-mapped) -- and the whole chain is one pass: each element is
// read once from every source, summed in the reference's order in a register
// and stored once, instead of N read-modify-write passes over dst.
//
// Bound: HBM (or xGMI for peer sources); algorithmic bytes per element
// 4 (dst) + 4 (residual) + 4 (N - 1) + 4 (store).  float4 lanes when every
// slice pointer shares one 16-byte phase (the head elements go scalar),
// nontemporal loads of the sources.
//
// The typed launcher takes bf16 / fp16 sources (a 16-bit model replica's
// gradients) and widens them in the load: 2 (N - 1) source bytes per element
// instead of the 10 (N - 1) of a cast to an fp32 temporary and its re-read.
// With the first term typed too (src[0]) dst is only stored: 4 (store) + 4
// (residual) + 2 N.  Lane groups of 8 or 4 elements by ws.h's GatherPlan.
#include <algorithm>
#include <cstdlib>

#include "ws.h"
#include "gather_dev.h"

namespace stg {

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

// MAXS >= nsrc: every source's float4 is loaded before any is added (a
// runtime-length loop of load-then-add waited for each load in turn), then
// the sum runs in the reference's order: dst, residual, grad[1], ...
// (Written out here and in send_batch.hip's gather_add_batch, not a function
// of gather_dev.h: through one, the MAXS = 8 kernels take 174 VGPRs, not 42.)
template <uint32_t MAXS>
__global__ void __launch_bounds__(STG_WG) gather_add_vec(GatherArgs a, size_t v0, size_t nv) {
    const size_t stride = (size_t)gridDim.x * STG_WG;
    for (size_t i = (size_t)blockIdx.x * STG_WG + threadIdx.x; i < nv; i += stride) {
        const size_t e = v0 + 4 * i;
        f4v x[MAXS];
        f4v acc = *reinterpret_cast<const f4v *>(a.dst + e);
        const f4v r = a.resid ? __builtin_nontemporal_load(reinterpret_cast<const f4v *>(a.resid + e)) : f4v{0, 0, 0, 0};
#pragma unroll
        for (uint32_t s = 1; s < MAXS; ++s)
            if (s < a.nsrc)
                x[s] = __builtin_nontemporal_load(reinterpret_cast<const f4v *>(static_cast<const float *>(a.src[s]) + e));
        if (a.resid) acc += r;
#pragma unroll
        for (uint32_t s = 1; s < MAXS; ++s)
            if (s < a.nsrc) acc += x[s];
        *reinterpret_cast<f4v *>(a.dst + e) = acc;
    }
}

__global__ void __launch_bounds__(STG_WG) gather_add_scalar(GatherArgs a, size_t b0, size_t b1) {
    const size_t stride = (size_t)gridDim.x * STG_WG;
    for (size_t e = b0 + (size_t)blockIdx.x * STG_WG + threadIdx.x; e < b1; e += stride) gather_elem<false>(a, e);
}

// The typed forms: sources of the STG_DT_* types in a.dtypes, the first term
// from a.src[0] when given.  W elements per lane group (ws.h GatherPlan).
template <uint32_t MAXS, uint32_t W>
__global__ void __launch_bounds__(STG_WG) gather_add_typed_vec(GatherArgs a, size_t v0, size_t nv) {
    const size_t stride = (size_t)gridDim.x * STG_WG;
    for (size_t i = (size_t)blockIdx.x * STG_WG + threadIdx.x; i < nv; i += stride)
        gather_lane<MAXS, W>(a, v0 + W * i);
}

__global__ void __launch_bounds__(STG_WG) gather_add_typed_scalar(GatherArgs a, size_t b0, size_t b1) {
    const size_t stride = (size_t)gridDim.x * STG_WG;
    for (size_t e = b0 + (size_t)blockIdx.x * STG_WG + threadIdx.x; e < b1; e += stride) gather_elem<true>(a, e);
}

template <uint32_t W>
void launch_typed_vec(const GatherArgs &a, size_t v0, size_t nv, uint32_t blocks, hipStream_t s) {
    if (a.nsrc <= 4) gather_add_typed_vec<4, W><<<blocks, STG_WG, 0, s>>>(a, v0, nv);
    else if (a.nsrc <= 8) gather_add_typed_vec<8, W><<<blocks, STG_WG, 0, s>>>(a, v0, nv);
    else gather_add_typed_vec<GATHER_MAX, W><<<blocks, STG_WG, 0, s>>>(a, v0, nv);
}

}  // namespace

hipError_t launch_gather_add(const GatherArgs &a, size_t start, size_t end, int num_cu, hipStream_t s) {
    if (end <= start) return hipSuccess;
    // the 16-byte phase of the slice start must agree across every pointer
    auto phase = [&](const void *p) { return (reinterpret_cast<uintptr_t>(static_cast<const float *>(p) + start) & 15u); };
    const uintptr_t ph = phase(a.dst);
    bool vec = (ph & 3u) == 0;
    if (a.resid) vec &= phase(a.resid) == ph;
    for (uint32_t i = 1; i < a.nsrc; ++i) vec &= phase(a.src[i]) == ph;
    size_t head = vec ? std::min<size_t>(end - start, ((16u - ph) & 15u) / 4u) : end - start;
    const size_t v0 = start + head, nv = vec ? (end - v0) / 4 : 0, vt = v0 + 4 * nv;
    const uint32_t cap = (uint32_t)num_cu * 8;
    if (nv) {
        const uint32_t blocks = (uint32_t)std::max<size_t>(1, std::min<size_t>((nv + STG_WG - 1) / STG_WG, cap));
        if (a.nsrc <= 4) gather_add_vec<4><<<blocks, STG_WG, 0, s>>>(a, v0, nv);
        else if (a.nsrc <= 8) gather_add_vec<8><<<blocks, STG_WG, 0, s>>>(a, v0, nv);
        else gather_add_vec<GATHER_MAX><<<blocks, STG_WG, 0, s>>>(a, v0, nv);
    }
    if (head) {
        const uint32_t blocks = (uint32_t)std::max<size_t>(1, std::min<size_t>((head + STG_WG - 1) / STG_WG, cap));
        gather_add_scalar<<<blocks, STG_WG, 0, s>>>(a, start, start + head);
    }
    if (vec && end > vt) gather_add_scalar<<<1, STG_WG, 0, s>>>(a, vt, end);
    return hipGetLastError();
}

uint32_t gather_max_width() {
    static const uint32_t w = [] {
        const char *e = getenv("STG_DEBUG_GATHER_WIDTH");
        return e && atoi(e) == 4 ? 4u : 8u;
    }();
    return w;
}

GatherPlan gather_plan_of(const GatherArgs &a, size_t start, size_t end) {
    uintptr_t addr[GATHER_MAX + 2];
    uint32_t esz[GATHER_MAX + 2], ns = 0;
    auto add = [&](const void *p, uint32_t dt) {
        esz[ns] = dt == GATHER_F32 ? 4u : 2u;
        addr[ns] = reinterpret_cast<uintptr_t>(p) + (uintptr_t)esz[ns] * start;
        ++ns;
    };
    add(a.dst, GATHER_F32);
    if (a.resid) add(a.resid, GATHER_F32);
    for (uint32_t i = a.src[0] ? 0 : 1; i < a.nsrc; ++i) add(a.src[i], (a.dtypes >> (2 * i)) & 3u);
    return gather_plan(addr, esz, ns, end - start, gather_max_width());
}

hipError_t launch_gather_add_typed(const GatherArgs &a, size_t start, size_t end, int num_cu, hipStream_t s) {
    if (end <= start) return hipSuccess;
    const GatherPlan p = gather_plan_of(a, start, end);
    const size_t head = p.width ? p.head : end - start;
    const size_t v0 = start + head, nv = p.width ? (end - v0) / p.width : 0, vt = v0 + p.width * nv;
    const uint32_t cap = (uint32_t)num_cu * 8;
    if (nv) {
        const uint32_t blocks = (uint32_t)std::max<size_t>(1, std::min<size_t>((nv + STG_WG - 1) / STG_WG, cap));
        if (p.width == 8) launch_typed_vec<8>(a, v0, nv, blocks, s);
        else launch_typed_vec<4>(a, v0, nv, blocks, s);
    }
    if (head) {
        const uint32_t blocks = (uint32_t)std::max<size_t>(1, std::min<size_t>((head + STG_WG - 1) / STG_WG, cap));
        gather_add_typed_scalar<<<blocks, STG_WG, 0, s>>>(a, start, start + head);
    }
    if (p.width && end > vt) gather_add_typed_scalar<<<1, STG_WG, 0, s>>>(a, vt, end);
    return hipGetLastError();
}

}  // namespace stg
