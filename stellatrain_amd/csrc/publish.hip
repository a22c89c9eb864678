// publish.hip -- hands a step's changed parameters to the node's model
// replicas (gfx950): the device form of ModuleH2DCopy::run
// (engine/modules/h2d_copy.cpp:31-56, gpu_param_tensor.copy_(cpu_param_tensor)
// per GPU of the node).
//
// The sparse steps write the parameter only at the indices of the merged
// stream (sgd.cpp:221-260, adam.cpp:19-86; weight decay too is applied to the
// touched elements), and leave those indices and their count on the device.
// So a replica is brought up to date by k element stores, not n:
//   replica_r[j] = cvt_r(param[j])   for j = idx[i], i < *count, j < n
// and no other element of a replica is stored to, not even with its old
// value (peers may be reading theirs).
//
// Up to PUBLISH_BATCH tasks share a launch; workgroups are dealt to the tasks
// by host-computed first-workgroup offsets (blk0), as in wire_encode_batch.
// The grid is sized from the slots the index buffer holds; a workgroup whose
// tile starts at or past the count read on the device leaves at once, and a
// count above the slots (0xffffffff: a merge that failed) publishes nothing.
// Plain streaming code: no atomics, nothing waits on another workgroup, no
// LDS, every loop bound fixed at launch.
//
// A lane owns PUBLISH_WP = 4 consecutive stream slots: one 16-byte index load
// where the buffer's phase allows, four gathers of param[j], all issued
// before the first store, then the stores of every replica.  The streams are
// not random -- thresholdv16 emits aligned lines of 16 consecutive indices and
// the world > 1 union is index-ascending with runs at any phase -- and a lone
// dword store costs about six times a dwordx4 store per byte, a 2-byte store
// twelve.  So (RUNS) a lane whose four indices are consecutive stores them as
// one 4-element word where the replica's ADDRESS (replicas are only
// element-aligned) is aligned to it, as two 2-element words where it is
// aligned to those, and else as element, 2-element word, element; a lane
// without such a run still pairs slots 0-1 and 2-3 where they are consecutive
// and the address is aligned.  A wide store covers published elements only.
//
// Bounds: 4 bytes of index and one 4-byte gather per pair, R stores; latency-
// and store-issue-bound like the emission kernels, far below HBM rate.
#include "ws.h"

namespace stg {

namespace {

typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef uint32_t u2v __attribute__((ext_vector_type(2)));
typedef uint32_t u4v __attribute__((ext_vector_type(4)));

// float -> bf16 bits, round to nearest even; a NaN keeps its sign and top
// payload bits and is made quiet; overflow reaches inf through the carry
__device__ __forceinline__ uint16_t to_bf16(float f) {
    const uint32_t u = f2u(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
// float -> fp16 bits: v_cvt_f16_f32 in the default mode (round to nearest
// even, subnormal results kept, overflow to inf, NaN stays NaN)
__device__ __forceinline__ uint16_t to_f16(float f) {
    const _Float16 h = (_Float16)f;
    return __builtin_bit_cast(uint16_t, h);
}

// In the stores below bit u of `ok` says slot u is published; p01 / p23 that
// the two slots are published and hold consecutive indices; run4 that all
// four do.
template <class T>
__device__ __forceinline__ uint32_t phase_of(const T *p) {
    return (uint32_t)(reinterpret_cast<uintptr_t>(p) / sizeof(T)) & 3u;  // in elements; replicas are element-aligned
}

__device__ __forceinline__ void pair_f32(float *rep, uint32_t ja, uint32_t jb, float xa, float xb, bool a, bool b,
                                         bool p) {
    if (p && !(phase_of(rep + ja) & 1u)) {
        *reinterpret_cast<f2v *>(rep + ja) = f2v{xa, xb};
        return;
    }
    if (a) rep[ja] = xa;
    if (b) rep[jb] = xb;
}

__device__ __forceinline__ void store_f32(float *rep, const uint32_t (&j)[PUBLISH_WP], const float (&x)[PUBLISH_WP],
                                          uint32_t ok, bool run4, bool p01, bool p23) {
    if (run4) {
        float *p = rep + j[0];
        const uint32_t ph = phase_of(p);
        if (ph == 0) {
            *reinterpret_cast<f4v *>(p) = f4v{x[0], x[1], x[2], x[3]};
        } else if (ph == 2) {
            *reinterpret_cast<f2v *>(p) = f2v{x[0], x[1]};
            *reinterpret_cast<f2v *>(p + 2) = f2v{x[2], x[3]};
        } else {
            p[0] = x[0];
            *reinterpret_cast<f2v *>(p + 1) = f2v{x[1], x[2]};
            p[3] = x[3];
        }
        return;
    }
    pair_f32(rep, j[0], j[1], x[0], x[1], ok & 1u, ok & 2u, p01);
    pair_f32(rep, j[2], j[3], x[2], x[3], ok & 4u, ok & 8u, p23);
}

__device__ __forceinline__ uint32_t pack2(uint16_t lo, uint16_t hi) { return (uint32_t)lo | ((uint32_t)hi << 16); }

__device__ __forceinline__ void pair_h16(uint16_t *rep, uint32_t ja, uint32_t jb, uint16_t xa, uint16_t xb, bool a,
                                         bool b, bool p) {
    if (p && !(phase_of(rep + ja) & 1u)) {
        *reinterpret_cast<uint32_t *>(rep + ja) = pack2(xa, xb);
        return;
    }
    if (a) rep[ja] = xa;
    if (b) rep[jb] = xb;
}

__device__ __forceinline__ void store_h16(uint16_t *rep, const uint32_t (&j)[PUBLISH_WP],
                                          const uint16_t (&x)[PUBLISH_WP], uint32_t ok, bool run4, bool p01, bool p23) {
    if (run4) {
        uint16_t *p = rep + j[0];
        const uint32_t ph = phase_of(p);
        if (ph == 0) {
            *reinterpret_cast<u2v *>(p) = u2v{pack2(x[0], x[1]), pack2(x[2], x[3])};
        } else if (ph == 2) {
            *reinterpret_cast<uint32_t *>(p) = pack2(x[0], x[1]);
            *reinterpret_cast<uint32_t *>(p + 2) = pack2(x[2], x[3]);
        } else {
            p[0] = x[0];
            *reinterpret_cast<uint32_t *>(p + 1) = pack2(x[1], x[2]);
            p[3] = x[3];
        }
        return;
    }
    pair_h16(rep, j[0], j[1], x[0], x[1], ok & 1u, ok & 2u, p01);
    pair_h16(rep, j[2], j[3], x[2], x[3], ok & 4u, ok & 8u, p23);
}

template <bool RUNS>
__global__ void __launch_bounds__(STG_WG) param_publish_batch(PublishBatch w) {
    const PublishTask &a = w.t[batch_item(w.t, w.nt)];
    const uint32_t wb = blockIdx.x - a.blk0;
    const uint64_t c = *a.count;
    if (c > a.cap) return;  // a failed merge's count (POISON_COUNT), or one the buffer cannot hold
    const uint64_t s0 = (uint64_t)wb * PUBLISH_TILE + threadIdx.x * PUBLISH_WP;
    if (s0 >= c) return;

    uint32_t j[PUBLISH_WP];
    if (s0 + PUBLISH_WP <= c && !(reinterpret_cast<uintptr_t>(a.idx) & 15u)) {
        const u4v q = *reinterpret_cast<const u4v *>(a.idx + s0);
        j[0] = q.x, j[1] = q.y, j[2] = q.z, j[3] = q.w;
    } else {
#pragma unroll
        for (uint32_t u = 0; u < PUBLISH_WP; ++u) j[u] = s0 + u < c ? a.idx[s0 + u] : 0xffffffffu;
    }
    uint32_t ok = 0;
    float x[PUBLISH_WP];
#pragma unroll
    for (uint32_t u = 0; u < PUBLISH_WP; ++u) {
        const bool v = s0 + u < c && j[u] < a.n;  // an index >= n is skipped, as the merge drops it
        ok |= (uint32_t)v << u;
        x[u] = v ? a.param[j[u]] : 0.f;
    }
    if (!ok) return;
    const bool p01 = RUNS && (ok & 3u) == 3u && j[1] == j[0] + 1;
    const bool p23 = RUNS && (ok & 12u) == 12u && j[3] == j[2] + 1;
    const bool run4 = p01 && p23 && j[2] == j[1] + 1;
    uint16_t xb[PUBLISH_WP], xh[PUBLISH_WP];
#pragma unroll
    for (uint32_t u = 0; u < PUBLISH_WP; ++u) {
        xb[u] = to_bf16(x[u]);
        xh[u] = to_f16(x[u]);
    }
#pragma unroll 4
    for (uint32_t r = 0; r < a.nrep; ++r) {
        const uint32_t dt = (a.dtypes >> (2 * r)) & 3u;
        if (dt == PUBLISH_F32) {
            store_f32(static_cast<float *>(a.rep[r]), j, x, ok, run4, p01, p23);
        } else {
            uint16_t xr[PUBLISH_WP];
#pragma unroll
            for (uint32_t u = 0; u < PUBLISH_WP; ++u) xr[u] = dt == PUBLISH_BF16 ? xb[u] : xh[u];
            store_h16(static_cast<uint16_t *>(a.rep[r]), j, xr, ok, run4, p01, p23);
        }
    }
}

}  // namespace

hipError_t launch_param_publish_batch(const PublishBatch &w, uint32_t blocks, bool runs, hipStream_t s) {
    if (!w.nt || !blocks) return hipSuccess;
    if (runs) param_publish_batch<true><<<blocks, STG_WG, 0, s>>>(w);
    else param_publish_batch<false><<<blocks, STG_WG, 0, s>>>(w);
    return hipGetLastError();
}

}  // namespace stg
