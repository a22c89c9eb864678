// merge_grad.h -- the dense typed gradient of a MERGE decompress
// (merge_grad.hip): its kernel tables and launchers.
#pragma once

#include "merge_sparse_batch.h"

namespace stg {

constexpr uint32_t GRAD_F32 = 0, GRAD_BF16 = 1, GRAD_F16 = 2;  // = STG_DT_*

// One tensor's emission over the scratch launch_sparse_bucketing has filled.
struct GradArgs {
    SparseScratch sc;  // sc.cnt null: per_rank == 0, every tile is empty and nothing of the scratch is read
    void *grad;        // n elements of the launch's type, element-aligned
    uint64_t n;
    uint32_t world;
    uint32_t ntiles;   // ceil(n / TB_TILE): the grid
    uint32_t cap;      // world * per_rank: record slots
    uint32_t lcap;     // entries of list
    float fworld;
};
// The emission (one launch): dtype GRAD_*; accumulate: grad += merged at union
// indices only, else every element of [0, n) is stored once.  a.ntiles >= 1.
hipError_t launch_grad_dense(const GradArgs &a, int dtype, bool accumulate, hipStream_t s);

// A group's emission over the scratch launch_sparse_batch_bucketing has filled:
// tensor q owns the virtual tiles [blk0_q, blk0_q + ceil(n_q / TB_TILE)).
struct GradBatchTensor {
    void *grad;
    uint32_t n;
    uint32_t blk0;
    uint32_t dtype;       // GRAD_*
    uint32_t accumulate;
};
struct GradBatchArgs {
    GradBatchTensor t[MERGE_BATCH];
    SparseScratch sc;
    uint32_t nt, world;
    uint32_t ntiles;   // the group's tiles: the grid
    uint32_t cap;      // the group's pairs: record slots
    uint32_t lcap;
    float fworld;
};
static_assert(sizeof(GradBatchArgs) <= 1024, "kernel arguments: stay well under 4 KiB");
hipError_t launch_grad_dense_batch(const GradBatchArgs &a, hipStream_t s);

}  // namespace stg
