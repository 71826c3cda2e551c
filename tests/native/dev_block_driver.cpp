// Stand-alone driver of rlao_amd/csrc/dev_block.hpp for tests/test_dev_block_host.py: the owner of libaoenv's device memory on host
// memory, with an allocator that counts, can be told to fail its n-th allocation, and notices a free of what it did not hand out.
// Prints one "name value..." line per answer; the Python test asserts them.  Plain C++, no GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>

#include "dev_block.hpp"

namespace {

struct HostMem {
    static std::set<void*> live;
    static int calls, frees, bad_frees, fail_at;       // fail_at: the number of the alloc call that fails (0: none)
    static bool alloc(void** p, size_t bytes) {
        if (++calls == fail_at) return false;
        *p = std::aligned_alloc(ao::kDevAlign, bytes);  // (a block's total is a multiple of the alignment)
        if (!*p) return false;
        std::memset(*p, 0xAB, bytes);
        live.insert(*p);
        return true;
    }
    static void free(void* p) {
        if (!live.erase(p)) { ++bad_frees; return; }
        ++frees;
        std::free(p);
    }
    static bool zero(void* p, size_t bytes) { std::memset(p, 0, bytes); return true; }
    static bool copy_in(void* dst, const void* src, size_t bytes) { std::memcpy(dst, src, bytes); return true; }
};
std::set<void*> HostMem::live;
int HostMem::calls = 0, HostMem::frees = 0, HostMem::bad_frees = 0, HostMem::fail_at = 0;

using Block = ao::DevBlock<HostMem>;
void fail_next() { HostMem::fail_at = HostMem::calls + 1; }
int n_live() { return (int)HostMem::live.size(); }
size_t count_not(const void* p, size_t n, unsigned char v) {
    size_t c = 0;
    for (size_t i = 0; i < n; ++i) c += static_cast<const unsigned char*>(p)[i] != v;
    return c;
}

// a feature record as env.hip keeps them: a block, plain pointers into it set once, plain configuration
struct Rec {
    bool set = false;
    int K = 0;
    Block mem;
    void* a = nullptr;
    void* b = nullptr;
};

void layout() {
    const ao::DevLayout l = ao::dev_layout({0, 1, 255, 256, 257});
    std::printf("layout_offsets");
    for (int k = 0; k < l.n; ++k) l.off[k] == ao::kDevNoPart ? std::printf(" null") : std::printf(" %zu", l.off[k]);
    std::printf("\nlayout_total %zu\n", l.total);
    Block b;
    const int rc = b.alloc({0, 1, 255, 256, 257}, false);
    std::printf("parts_rc %d calls %d live %d\n", rc, HostMem::calls, n_live());
    std::printf("parts_from_base");
    const char* base = static_cast<const char*>(b.part(1));
    for (int k = 0; k < 5; ++k) b.part(k) ? std::printf(" %td", static_cast<const char*>(b.part(k)) - base) : std::printf(" null");
    std::printf("\nparts_outside %d %d\n", b.part(-1) == nullptr, b.part(5) == nullptr);
    std::printf("base_misaligned %zu\n", (size_t)((uintptr_t)b.part(1) % ao::kDevAlign));
    const int calls = HostMem::calls;
    Block z;
    const int rz = z.alloc({0, 0, 0}, true);
    std::printf("zeros_only rc %d allocations %d live_block %d part0_null %d\n", rz, HostMem::calls - calls, (bool)z, z.part(0) == nullptr);
}

void zeroing() {
    Block a, b;
    a.alloc({0, 1, 255, 256, 257}, true);
    b.alloc({0, 1, 255, 256, 257}, false);
    std::printf("zeroed_nonzero_bytes %zu\n", count_not(a.part(1), 1280, 0));
    std::printf("unzeroed_touched_bytes %zu\n", count_not(b.part(1), 1280, 0xAB));
}

void uploads() {
    Block b;
    b.alloc({0, 8, 300}, true);
    const char src[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    const int ok = b.upload(1, src, 8), too_long = b.upload(1, src, 9), absent = b.upload(0, src, 1), none = b.upload(0, src, 0);
    std::printf("upload ok %d too_long %d absent %d empty %d arrived %d next_part_untouched %zu\n", ok, too_long, absent, none,
                std::memcmp(b.part(1), src, 8) == 0, count_not(b.part(2), 300, 0));
}

void failures() {
    const int live0 = n_live();
    Block b;
    fail_next();
    const int rc = b.alloc({64, 64}, true);
    std::printf("failed_alloc rc %d empty %d part0_null %d live_delta %d\n", rc, !b, b.part(0) == nullptr, n_live() - live0);
    b.alloc({16}, true);
    static_cast<char*>(b.part(0))[3] = 77;
    void* held = b.part(0);
    const int frees = HostMem::frees;
    fail_next();
    const int rc2 = b.alloc({4096, 4096}, false);
    std::printf("failed_replacement rc %d same_block %d data_intact %d frees %d live_delta %d\n", rc2, b.part(0) == held,
                static_cast<char*>(b.part(0))[3] == 77, HostMem::frees - frees, n_live() - live0);
    const int rc3 = b.alloc({4096, 4096}, false);
    std::printf("replacement rc %d old_freed %d frees %d live_delta %d\n", rc3, HostMem::live.count(held) == 0, HostMem::frees - frees,
                n_live() - live0);
}

void frees() {
    int f0 = HostMem::frees;
    {
        Block a;
        a.alloc({100}, false);
        void* p = a.part(0);
        Block b(std::move(a));
        std::printf("move_construct frees %d source_empty %d dest_holds %d", HostMem::frees - f0, !a && a.part(0) == nullptr, b.part(0) == p);
    }
    std::printf(" frees_after_scope %d\n", HostMem::frees - f0);
    f0 = HostMem::frees;
    {
        Block a, b;
        a.alloc({100}, false);
        b.alloc({200}, false);
        void *pa = a.part(0), *pb = b.part(0);
        b = std::move(a);
        std::printf("move_assign frees %d target_old_freed %d target_holds_source %d source_empty %d", HostMem::frees - f0,
                    HostMem::live.count(pb) == 0, b.part(0) == pa && HostMem::live.count(pa) == 1, !a);
    }
    std::printf(" frees_after_scope %d\n", HostMem::frees - f0);
    f0 = HostMem::frees;
    {
        Block a;
        a.alloc({100}, false);
        void* p = a.part(0);
        Block& same = a;
        a = std::move(same);
        std::printf("self_move_assign frees %d still_holds %d", HostMem::frees - f0, a.part(0) == p && HostMem::live.count(p) == 1);
    }
    std::printf(" frees_after_scope %d\n", HostMem::frees - f0);
    f0 = HostMem::frees;
    {
        Block a;
        a.alloc({100}, false);
        a.reset();
        a.reset();
        std::printf("reset_twice frees %d empty %d", HostMem::frees - f0, !a);
    }
    std::printf(" frees_after_scope %d\n", HostMem::frees - f0);
}

void record_swap() {
    const int live0 = n_live(), f0 = HostMem::frees;
    Rec rec;
    rec.mem.alloc({32, 0, 32}, true);
    rec.a = rec.mem.part(0);
    rec.b = rec.mem.part(2);
    rec.K = 3;
    rec.set = true;
    void* first = rec.a;
    {
        Rec local;                                         // built whole, then moved in: what a failed build leaves is `rec` as it was
        local.mem.alloc({64, 64, 0}, true);
        local.a = local.mem.part(0);
        local.b = local.mem.part(1);
        local.K = 7;
        local.set = true;
        void* second = local.a;
        rec = std::move(local);
        std::printf("record_move frees %d old_freed %d holds_new %d K %d set %d local_block_empty %d", HostMem::frees - f0,
                    HostMem::live.count(first) == 0, rec.a == second && rec.mem.part(0) == second && rec.b == rec.mem.part(1), rec.K, rec.set,
                    !local.mem);
    }
    std::printf(" frees_after_scope %d live_delta %d\n", HostMem::frees - f0, n_live() - live0);
    rec = Rec{};
    std::printf("record_clear frees %d live_delta %d set %d K %d pointers_null %d block_empty %d\n", HostMem::frees - f0, n_live() - live0, rec.set,
                rec.K, rec.a == nullptr && rec.b == nullptr, !rec.mem);
}

}  // namespace

int main() {
    layout();
    zeroing();
    uploads();
    failures();
    frees();
    record_swap();
    std::printf("exit live %d bad_frees %d allocations %zu frees %d\n", n_live(), HostMem::bad_frees,
                (size_t)HostMem::calls - 2 /* the two refused */, HostMem::frees);
    return n_live() == 0 && HostMem::bad_frees == 0 ? 0 : 1;
}
