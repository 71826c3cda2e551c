// The one owner of libaoenv's device memory: a move-only block of ONE allocation, carved into parts that each start on a 256-byte
// boundary.  Host only, plain C++: the primitives (allocate, free, zero, copy in) come from the policy type `Mem`, so the library
// (HipMem, env.hip) and the stand-alone driver tests/native/dev_block_driver.cpp (host memory, a counting allocator) share this code.
//
// Mem has four static functions: bool alloc(void** p, size_t bytes), void free(void* p), bool zero(void* p, size_t bytes) and
// bool copy_in(void* dst, const void* src, size_t bytes); true = done, and a failure leaves no error pending.
//
// A block is freed where its owner goes away or is assigned over, with kernels that read it possibly still queued: the device free
// (hipFree) waits for the device before it releases memory, and the whole library relies on that.  A stream-ordered or pooled free
// must not take its place here; nothing else (pools, reference counts) belongs in this file either.
#pragma once
#include <cstddef>
#include <initializer_list>

namespace ao {

constexpr size_t kDevAlign = 256;                    // every part's alignment inside its block
constexpr int kDevMaxParts = 12;
constexpr size_t kDevNoPart = ~(size_t)0;            // offset of a part of zero bytes: it has no address

struct DevLayout {
    int n = 0;
    size_t off[kDevMaxParts] = {};                   // kDevNoPart for an empty part
    size_t size[kDevMaxParts] = {};
    size_t total = 0;                                // 0: nothing to allocate
};

// part sizes in bytes -> offsets and the total; an empty part takes no room (more than kDevMaxParts sizes: the rest is ignored)
inline DevLayout dev_layout(std::initializer_list<size_t> sizes) {
    DevLayout l;
    for (size_t b : sizes) {
        if (l.n == kDevMaxParts) break;
        l.size[l.n] = b;
        l.off[l.n++] = b ? l.total : kDevNoPart;
        l.total += (b + kDevAlign - 1) & ~(kDevAlign - 1);
    }
    return l;
}

template <class Mem>
class DevBlock {
    void* base_ = nullptr;
    DevLayout lay_;
    void take(DevBlock& o) { base_ = o.base_; lay_ = o.lay_; o.base_ = nullptr; o.lay_ = DevLayout{}; }

public:
    DevBlock() = default;
    DevBlock(const DevBlock&) = delete;
    DevBlock& operator=(const DevBlock&) = delete;
    DevBlock(DevBlock&& o) noexcept { take(o); }
    DevBlock& operator=(DevBlock&& o) noexcept { if (this != &o) { reset(); take(o); } return *this; }
    ~DevBlock() { reset(); }

    // One allocation for the parts, zeroed whole if asked.  0, or 1 when there is no memory (the caller words the message): the
    // block is then what it was before the call -- empty, or the live block that was to be replaced.  On success a block held
    // before is freed.
    int alloc(std::initializer_list<size_t> sizes, bool zero) {
        const DevLayout l = dev_layout(sizes);
        void* p = nullptr;
        if (l.total) {
            if (!Mem::alloc(&p, l.total)) return 1;
            if (zero && !Mem::zero(p, l.total)) { Mem::free(p); return 1; }
        }
        reset();
        base_ = p;
        lay_ = l;
        return 0;
    }
    void reset() {
        if (base_) Mem::free(base_);
        base_ = nullptr;
        lay_ = DevLayout{};
    }
    explicit operator bool() const { return base_ != nullptr; }
    void* part(int k) const {
        if (!base_ || k < 0 || k >= lay_.n || lay_.off[k] == kDevNoPart) return nullptr;
        return static_cast<char*>(base_) + lay_.off[k];
    }
    // host memory into the front of part k: 0, or 1 (the part is absent or shorter than `bytes`, or the copy failed)
    int upload(int k, const void* src, size_t bytes) {
        void* dst = part(k);
        if (bytes == 0) return 0;
        if (!dst || bytes > lay_.size[k]) return 1;
        return Mem::copy_in(dst, src, bytes) ? 0 : 1;
    }
};

}  // namespace ao
