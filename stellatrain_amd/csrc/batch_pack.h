// batch_pack.h -- the host side of a batched launch's table: items dealt
// consecutive runs of workgroups, a launch closed when the table is full or
// its grid would pass a limit.  (The device side is batch_item, common.h.)
//
// Table is one of ws.h's by-value kernel tables: an array `t` of items with a
// `blk0` (the item's first workgroup) and a count `nt`.  `launch` is called as
// launch(table, workgroups) -> int (0 = ok) for every non-empty table.
#pragma once

#include <stdint.h>

#include <type_traits>
#include <utility>

namespace stg {

template <class Table, class Launch>
class BatchPacker {
public:
    using Item = typename std::remove_extent<decltype(Table::t)>::type;
    static constexpr uint32_t CAP = std::extent<decltype(Table::t)>::value;

    // limit: workgroups one launch may have; an item with more runs alone
    BatchPacker(uint64_t limit, Launch launch) : limit_(limit), launch_(std::move(launch)) {}

    // The slot of the next item, of nbk workgroups, with blk0 set.  Closes the
    // pending launch first when the table is full, or is not empty and would
    // pass the limit; a launch that fails comes back with *slot = nullptr.
    int add(uint64_t nbk, Item **slot) {
        *slot = nullptr;
        if (tab_.nt == CAP || (tab_.nt && blocks_ + nbk > limit_))
            if (const int rc = flush()) return rc;
        Item &d = tab_.t[tab_.nt++];
        d.blk0 = (uint32_t)blocks_;
        blocks_ += nbk;
        *slot = &d;
        return 0;
    }

    // Launches what is pending (nothing: no call) and starts an empty table.
    int flush() {
        const int rc = tab_.nt ? launch_(tab_, (uint32_t)blocks_) : 0;
        tab_ = Table{};
        blocks_ = 0;
        return rc;
    }

    Table &table() { return tab_; }
    uint32_t count() const { return tab_.nt; }
    uint64_t blocks() const { return blocks_; }

private:
    Table tab_{};
    uint64_t blocks_ = 0;
    uint64_t limit_;
    Launch launch_;
};

template <class Table, class Launch>
BatchPacker<Table, Launch> make_packer(uint64_t limit, Launch launch) {
    return BatchPacker<Table, Launch>(limit, std::move(launch));
}

}  // namespace stg
