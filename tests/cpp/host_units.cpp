// host_units.cpp -- the host layer's two small building blocks without a GPU:
// DevBuf (csrc/devbuf.h) and BatchPacker (csrc/batch_pack.h) against a fake
// allocator.  Builds with a host compiler and no HIP library:
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include host_units.cpp
// (tests/test_host_units.py adds -fsanitize=address,undefined and runs it).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../stellatrain_amd/csrc/batch_pack.h"
#include "../../stellatrain_amd/csrc/devbuf.h"

// ---- the five HIP calls DevBuf makes, on host memory ----
namespace fake {
std::map<void *, size_t> live;  // block -> bytes
int allocs = 0;                 // hipMalloc calls so far
int fail_at = 0;                // the k-th hipMalloc from now fails (0: none)
int syncs = 0, memsets = 0;
size_t last_bytes = 0;
}  // namespace fake

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) {
    ++fake::allocs;
    if (fake::fail_at && --fake::fail_at == 0) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = malloc(bytes ? bytes : 1);
    memset(*p, 0xab, bytes);  // recycled memory is never zero
    fake::live[*p] = bytes;
    fake::last_bytes = bytes;
    return hipSuccess;
}
hipError_t hipFree(void *p) {
    if (!p) return hipSuccess;
    if (!fake::live.erase(p)) {
        fprintf(stderr, "hipFree of a block that is not live\n");
        abort();
    }
    free(p);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *p, int v, size_t bytes, hipStream_t) {
    ++fake::memsets;
    auto it = fake::live.find(p);
    if (it == fake::live.end() || bytes > it->second) {
        fprintf(stderr, "hipMemsetAsync outside a live block\n");
        abort();
    }
    memset(p, v, bytes);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
    ++fake::syncs;
    return hipSuccess;
}
const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake error"; }
}

static int g_failed = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            ++g_failed;                                                  \
        }                                                                \
    } while (0)

template <typename T>
static bool sound(const stg::DevBuf<T> &b) {  // the invariant, and the capacity is really backed
    if ((b.get() == nullptr) != (b.cap() == 0)) return false;
    if (!b.get()) return true;
    auto it = fake::live.find(b.get());
    return it != fake::live.end() && it->second == b.cap() * sizeof(T);
}

static bool all_bytes(const void *p, size_t n, unsigned char v) {
    const unsigned char *c = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; ++i)
        if (c[i] != v) return false;
    return true;
}

static void devbuf_cases() {
    {
        stg::DevBuf<uint32_t> b;
        bool fresh = false;
        CHECK(sound(b) && b.cap() == 0);
        // growth to max(need, 1.5 x cap); the wait comes with every reallocation
        CHECK(b.reserve(100, nullptr, false, &fresh) == hipSuccess && fresh && b.cap() == 100 && sound(b));
        CHECK(fake::syncs == 1);
        CHECK(b.reserve(101, nullptr, false, &fresh) == hipSuccess && fresh && b.cap() == 150 && sound(b));
        CHECK(b.reserve(1000, nullptr, false, &fresh) == hipSuccess && fresh && b.cap() == 1000 && sound(b));
        CHECK(fake::syncs == 3 && fake::live.size() == 1);
        // need <= cap: no call at all
        const int a0 = fake::allocs, s0 = fake::syncs;
        uint32_t *p0 = b.get();
        CHECK(b.reserve(1000, nullptr, true, &fresh) == hipSuccess && !fresh && b.get() == p0);
        CHECK(b.reserve(1, nullptr, true, &fresh) == hipSuccess && !fresh && b.get() == p0);
        CHECK(fake::allocs == a0 && fake::syncs == s0 && fake::memsets == 0);
        // zeroing covers the whole new capacity, not the need
        CHECK(b.reserve(1001, nullptr, true, &fresh) == hipSuccess && fresh && b.cap() == 1500);
        CHECK(fake::memsets == 1 && all_bytes(b.get(), 1500 * sizeof(uint32_t), 0));
        // a cap on growth
        CHECK(b.reserve(1600, nullptr, false, &fresh, 1700) == hipSuccess && b.cap() == 1700 && sound(b));
        // and not zeroed unless asked (the fake hands out 0xab)
        CHECK(all_bytes(b.get(), 1700 * sizeof(uint32_t), 0xab));
    }
    CHECK(fake::live.empty());  // nothing live after destruction

    {   // a failed allocation: empty buffer, the error, and the next reserve allocates again
        stg::DevBuf<float> b;
        bool fresh = true;
        CHECK(b.reserve(10, nullptr, true) == hipSuccess);
        fake::fail_at = 1;
        CHECK(b.reserve(20, nullptr, true, &fresh) == hipErrorOutOfMemory);
        CHECK(!fresh && b.get() == nullptr && b.cap() == 0 && sound(b) && fake::live.empty());
        // (today's defect: a call that fits the remembered capacity returned OK on a null pointer)
        CHECK(b.reserve(5, nullptr, true, &fresh) == hipSuccess && fresh && b.get() && b.cap() == 5 && sound(b));
        CHECK(all_bytes(b.get(), 5 * sizeof(float), 0));
    }
    CHECK(fake::live.empty());

    {   // a pair sized together: the second allocation fails, neither keeps a capacity its pointer does not back
        stg::DevBuf<uint32_t> pos;
        stg::DevBuf<float> val;
        CHECK(pos.reserve(64, nullptr, false) == hipSuccess && val.reserve(64, nullptr, false) == hipSuccess);
        fake::fail_at = 2;
        hipError_t e = pos.reserve(200, nullptr, false);
        if (e == hipSuccess) e = val.reserve(200, nullptr, false);
        CHECK(e == hipErrorOutOfMemory);
        CHECK(sound(pos) && pos.cap() == 200);
        CHECK(sound(val) && val.cap() == 0 && val.get() == nullptr);
        // the next sizing of the pair brings both to the need, whatever each one held
        e = pos.reserve(150, nullptr, false);
        if (e == hipSuccess) e = val.reserve(150, nullptr, false);
        CHECK(e == hipSuccess && sound(pos) && sound(val) && pos.cap() == 200 && val.cap() == 150);
    }
    CHECK(fake::live.empty());

    {   // moves leave the source empty and free nothing twice
        stg::DevBuf<uint64_t> a;
        CHECK(a.reserve(8, nullptr, false) == hipSuccess);
        uint64_t *p = a.get();
        stg::DevBuf<uint64_t> b(std::move(a));
        CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == p && b.cap() == 8 && sound(b));
        stg::DevBuf<uint64_t> c;
        CHECK(c.reserve(4, nullptr, false) == hipSuccess);
        c = std::move(b);  // c's old block goes
        CHECK(b.get() == nullptr && b.cap() == 0 && c.get() == p && sound(c) && fake::live.size() == 1);
        std::vector<stg::DevBuf<uint64_t>> v;
        v.push_back(std::move(c));
        v.emplace_back();
        CHECK(v[0].get() == p && fake::live.size() == 1);
    }
    CHECK(fake::live.empty());
}

// ---- the packer ----
struct Item {
    int id;
    uint32_t blk0;
};
struct Table {
    Item t[16];
    uint32_t nt;
};
struct Launched {
    std::vector<Item> items;
    uint32_t blocks;
};

static void packer_cases() {
    std::vector<Launched> out;
    int fail_with = 0;
    const auto launch = [&](Table &w, uint32_t blocks) -> int {
        out.push_back(Launched{std::vector<Item>(w.t, w.t + w.nt), blocks});
        return fail_with;
    };
    const auto put = [](auto &pk, int id, uint64_t nbk) {
        Item *d = nullptr;
        const int rc = pk.add(nbk, &d);
        if (rc == 0) d->id = id;
        else CHECK(d == nullptr);
        return rc;
    };
    {   // 17 items at capacity 16: launches of 16 and 1, blk0 restarting at 0
        auto pk = stg::make_packer<Table>(0x7fffffffull, launch);
        for (int i = 0; i < 17; ++i) CHECK(put(pk, i, 3) == 0);
        CHECK(out.size() == 1 && pk.count() == 1 && pk.blocks() == 3);
        CHECK(pk.flush() == 0 && out.size() == 2);
        CHECK(out[0].items.size() == 16 && out[0].blocks == 48 && out[1].items.size() == 1 && out[1].blocks == 3);
        for (int i = 0; i < 16; ++i) CHECK(out[0].items[i].id == i && out[0].items[i].blk0 == 3u * i);
        CHECK(out[1].items[0].id == 16 && out[1].items[0].blk0 == 0);
        // a flush of an empty table launches nothing
        CHECK(pk.flush() == 0 && out.size() == 2 && pk.count() == 0 && pk.blocks() == 0);
    }
    out.clear();
    {   // the workgroup limit closes a non-empty table early; an item larger than the limit runs alone
        auto pk = stg::make_packer<Table>(10, launch);
        CHECK(put(pk, 0, 4) == 0 && put(pk, 1, 6) == 0);  // 10: not past the limit
        CHECK(out.empty());
        CHECK(put(pk, 2, 1) == 0);  // 11 would pass it
        CHECK(out.size() == 1 && out[0].items.size() == 2 && out[0].blocks == 10);
        CHECK(put(pk, 3, 25) == 0);  // larger than the limit: closes {2}, then sits alone ...
        CHECK(out.size() == 2 && out[1].items.size() == 1 && out[1].items[0].id == 2 && out[1].blocks == 1);
        CHECK(put(pk, 4, 1) == 0);  // ... and is closed by the next item
        CHECK(out.size() == 3 && out[2].items.size() == 1 && out[2].items[0].id == 3 && out[2].blocks == 25 &&
              out[2].items[0].blk0 == 0);
        // an empty table takes an item larger than the limit without a launch
        CHECK(pk.flush() == 0 && out.size() == 4);
        CHECK(put(pk, 5, 11) == 0 && out.size() == 4 && pk.count() == 1);
        // a forced close
        CHECK(pk.flush() == 0 && out.size() == 5 && out[4].items[0].id == 5 && out[4].blocks == 11);
        CHECK(put(pk, 6, 2) == 0 && pk.count() == 1 && pk.table().t[0].blk0 == 0);
        CHECK(pk.flush() == 0 && out.size() == 6);
    }
    out.clear();
    {   // a failing launch: its code comes back, and nothing is launched after it
        auto pk = stg::make_packer<Table>(0x7fffffffull, launch);
        for (int i = 0; i < 16; ++i) CHECK(put(pk, i, 1) == 0);
        fail_with = -7;
        CHECK(put(pk, 16, 1) == -7);
        CHECK(out.size() == 1 && pk.count() == 0);
        CHECK(pk.flush() == 0 && out.size() == 1);  // the failed table is gone, not sent again
        CHECK(put(pk, 17, 1) == 0);
        CHECK(pk.flush() == -7 && out.size() == 2);
        fail_with = 0;
    }
}

int main() {
    devbuf_cases();
    packer_cases();
    if (g_failed) {
        fprintf(stderr, "host_units: %d check(s) failed\n", g_failed);
        return 1;
    }
    printf("host_units: ok\n");
    return 0;
}
