// merge_sparse.h -- the tile-bucketed sparse MERGE decompress (merge_sparse.hip):
// its constants, the layout of its scratch and its launcher.
#pragma once

#include <stddef.h>

#include "ws.h"

namespace stg {

// A tile is TB_TILE consecutive indices, merged densely in one workgroup's
// LDS: a float sum and an election word per index and a mark byte, 36 KiB of
// the CU's 160 KiB, so four workgroups share a CU.
constexpr uint32_t TB_TILE_SHIFT = 12;
constexpr uint32_t TB_TILE = 1u << TB_TILE_SHIFT;
static_assert(TB_TILE == 16 * STG_WG, "the emission: 16 indices per lane");
constexpr uint32_t TB_RANKS = 64;           // rank streams one bucketing launch reads (its table travels by value)
constexpr uint32_t TB_CACHE = 4;            // records of a tile a lane holds in registers (1,024 per workgroup)
constexpr uint32_t TB_PAIRS = 4 * STG_WG;   // pairs of one rank per bucketing workgroup
constexpr uint32_t FAIL_MERGE_SPARSE = 16u; // the scratch's fail word: counters, offsets or counts disagreed

struct SparseCtl {
    uint32_t ntl;      // non-empty tiles of the call (entries of `list`)
    uint32_t kept;     // pairs with index < n
    uint32_t pad[2];
};

// The scratch of one call, all in the (device, stream) MergeScratch:
//   cnt   world words per tile, tile-major: pairs of (tile, rank); zero between
//         calls.  The scan turns a non-empty tile's words into the segments'
//         first record slots, the placement advances each to its segment's end,
//         the emission zeroes them;
//   list  the non-empty tiles in ascending order: {tile, first record slot};
//   ucnt  per listed tile its union size, then (tb_tscan) the exclusive prefix;
//   rec   per kept pair {position in its rank, index within the tile}, and
//   rval  its value: a tile's segments back to back in rank order.
struct SparseScratch {
    uint32_t *cnt;
    uint2 *list;
    uint32_t *ucnt;
    uint2 *rec;
    float *rval;
    SparseCtl *ctl;
    uint32_t *fail;
};

// Host arithmetic of the sizes: tiles = ceil(n / TB_TILE), pairs = world *
// per_rank, list = min(tiles, pairs).
struct SparseSizes {
    size_t tiles, pairs, list;
    size_t bytes(int world) const {
        return 4 * (size_t)world * tiles + 12 * list + 12 * pairs + sizeof(SparseCtl);
    }
};
inline SparseSizes sparse_sizes(size_t per_rank, int world, size_t n) {
    SparseSizes z;
    z.tiles = (n + TB_TILE - 1) / TB_TILE;
    z.pairs = (size_t)world * per_rank;
    z.list = std::min(z.tiles, z.pairs);
    return z;
}

struct SparseRanks {
    RankStream r[TB_RANKS];
    uint32_t nr;       // streams in this launch
    uint32_t r0;       // the rank of r[0]
};
struct SparseArgs {
    SparseScratch sc;
    uint64_t n;
    uint32_t world, per_rank;
    uint32_t ntiles;   // ceil(n / TB_TILE)
    uint32_t cap;      // world * per_rank: record slots, and slots of the output
    uint32_t lcap;     // entries of list / ucnt
    float fworld;
    // the output and, for a fused step, the tensor's optimizer fields as the
    // batched world > 1 emission carries them (Step<OPT>, merge_dev.h)
    MergeWorldTensor t;
    SgdLaunch sgd;
    AdamLaunch adam;
};
static_assert(sizeof(SparseRanks) + sizeof(SparseArgs) <= 3072, "kernel arguments: stay under 4 KiB");

// The six launches of one call (per_rank >= 1): count, scan, place, per-tile
// union counts, their scan, emission.  opt: -1 = no step, else as
// launch_merge_world_emit's.  `ranks` holds a.world host entries.
hipError_t launch_merge_sparse(const RankStream *ranks, const SparseArgs &a, int opt, int num_cu, hipStream_t s);
// Its first three (count, scan, place) alone, for an emission of another kind
// (merge_grad.hip): reads a.sc, n, world, per_rank, ntiles, cap and lcap.
hipError_t launch_sparse_bucketing(const RankStream *ranks, const SparseArgs &a, hipStream_t s);

}  // namespace stg
