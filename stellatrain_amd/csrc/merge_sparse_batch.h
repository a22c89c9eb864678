// merge_sparse_batch.h -- the sparse MERGE decompress + optimizer step of a
// group of tensors in shared launches (merge_sparse_batch.hip): the group's
// caps, its by-value kernel tables and its launcher.
#pragma once

#include "merge_sparse.h"

namespace stg {

// A group is up to MERGE_BATCH consecutive tensors of one world laid side by
// side in one virtual tile space: tensor q owns the tiles [tile0_q, tile0_q +
// ceil(n_q / TB_TILE)).  Counters, tile list, records and union counts are those
// of one sparse call over that space (SparseScratch, sized by sparse_sizes'
// formula with the group's sums), so a group closes before
constexpr uint32_t SB_TILE_CAP = 1u << 16;  // ... its tiles would pass this: the one-workgroup scans stay at 16 rounds
constexpr uint32_t SB_PAIR_CAP = 1u << 21;  // ... its pairs (world * the sum of per_rank) would: 24 MiB of records
constexpr uint32_t SB_RANKS = 4;            // rank streams of every tensor one bucketing launch reads

// The bucketing launches' table: per tensor SB_RANKS streams by value.
struct SparseBucketTensor {
    RankStream r[SB_RANKS];
    uint32_t n, per_rank;
    uint32_t tile0;
    uint32_t bpr;      // workgroups per rank: ceil(per_rank / TB_PAIRS)
    uint32_t blk0;     // first workgroup of this tensor: bpr per rank of the launch
    uint32_t pad;
};
struct SparseBucketArgs {
    SparseBucketTensor t[MERGE_BATCH];
    SparseScratch sc;
    uint32_t nt, world;
    uint32_t r0;       // the rank of r[0]
    uint32_t cap;      // record slots of the group
};

// The scans' and the tile kernels' table: a tensor's outputs and the fields of
// its step (Step<OPT>, merge_dev.h), as MergeWorldTensor carries them.
struct SparseBatchTensor {
    uint32_t *out_idx;
    float *out_val;
    uint32_t *out_count;
    float *param;
    float *s0;
    void *s1;
    union {
        struct { double c1, c2; } adam;
        struct { uint32_t iter, first; } sgd;
    } u;
    uint32_t n;
    uint32_t blk0;     // tile0: the tensor's first tile in the group's tile space
    uint32_t ocap;     // world * per_rank: the slots of its output
    uint32_t pad;
};
struct SparseBatchArgs {
    SparseBatchTensor t[MERGE_BATCH];
    SparseScratch sc;
    uint32_t nt, world;
    uint32_t ntiles;   // the group's tiles
    uint32_t cap;      // the group's pairs: record slots
    uint32_t lcap;     // entries of list / ucnt
    float fworld;
    SgdLaunch sgd;     // the handle-wide scalars (per-tensor fields unset), opt 0 / 1
    AdamLaunch adam;   // ... opt 2
};
static_assert(sizeof(SparseBucketArgs) <= 3072 && sizeof(SparseBatchArgs) <= 3072,
              "kernel arguments: stay under 4 KiB");

// Launches of one group: two bucketing passes of ceil(world / SB_RANKS) each,
// the scan, the per-tile union counts, their segmented scan, the emission.
inline uint32_t sparse_batch_launches(uint32_t world) { return 4 + 2 * ((world + SB_RANKS - 1) / SB_RANKS); }

// One group (w.nt >= 1 tensors, every per_rank >= 1, w.world <= TB_RANKS).
// ranks[q] holds tensor q's w.world host entries; opt as launch_merge_world_emit's.
hipError_t launch_merge_sparse_batch(const SparseBatchArgs &w, const RankStream *const *ranks, int opt, int num_cu,
                                     hipStream_t s, uint64_t *launches = nullptr);
// Its bucketing launches (count, scan, place) alone, for an emission of another
// kind (merge_grad.hip): reads w.sc, nt, world, ntiles, cap, lcap and per tensor
// n, blk0 and ocap.
hipError_t launch_sparse_batch_bucketing(const SparseBatchArgs &w, const RankStream *const *ranks, hipStream_t s,
                                         uint64_t *launches = nullptr);

}  // namespace stg
