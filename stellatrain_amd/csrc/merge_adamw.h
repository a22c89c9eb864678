// merge_adamw.h -- the dense AdamW step fused into a MERGE decompress
// (merge_adamw.hip): its kernel tables and launchers.
#pragma once

#include "merge_grad.h"

namespace stg {

// The step's constants, rounded once on the host from doubles.
struct AdamwHyper {
    float decay;       // 1 - lr * weight_decay (decoupled)
    float wd;          // weight_decay (coupled: g += wd * x)
    float beta1, omb1; // omb1 = 1 - beta1
    float beta2, omb2;
    float bc2s;        // sqrt(1 - beta2^step)
    float eps;
    float ss;          // lr / (1 - beta1^step)
    uint32_t decoupled;
};

// One tensor's arrays.  The fp32 arrays (m, v and master, or param where it is
// fp32) are 4-byte aligned and congruent mod 16; a 16-bit param is 2-byte aligned.
struct AdamwTensor {
    void *param;       // n elements of the launch's type
    float *master;     // null: param is read; else the fp32 master, param = cvt(master')
    float *m, *v;
};

// One tensor's step over the scratch launch_sparse_bucketing has filled.
struct AdamwArgs {
    SparseScratch sc;  // sc.cnt null: per_rank == 0, every tile is empty and nothing of the scratch is read
    AdamwTensor t;
    uint64_t n;
    uint32_t world;
    uint32_t ntiles;   // ceil(n / TB_TILE): the grid
    uint32_t cap;      // world * per_rank: record slots
    uint32_t lcap;     // entries of list
    float fworld;
    AdamwHyper h;
};
// The step (one launch): dtype GRAD_* of t.param; a master needs a 16-bit dtype.  a.ntiles >= 1.
hipError_t launch_adamw_dense(const AdamwArgs &a, int dtype, hipStream_t s);

// A group's step over the scratch launch_sparse_batch_bucketing has filled:
// tensor q owns the virtual tiles [blk0_q, blk0_q + ceil(n_q / TB_TILE)).
struct AdamwBatchTensor {
    AdamwTensor t;
    uint32_t n;
    uint32_t blk0;
    uint32_t dtype;    // GRAD_*
    uint32_t pad;
};
struct AdamwBatchArgs {
    AdamwBatchTensor t[MERGE_BATCH];
    SparseScratch sc;
    uint32_t nt, world;
    uint32_t ntiles;   // the group's tiles: the grid
    uint32_t cap;      // the group's pairs: record slots
    uint32_t lcap;
    float fworld;
    AdamwHyper h;
};
static_assert(sizeof(AdamwBatchArgs) <= 1024, "kernel arguments: stay well under 4 KiB");
hipError_t launch_adamw_dense_batch(const AdamwBatchArgs &a, hipStream_t s);

}  // namespace stg
