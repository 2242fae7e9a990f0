// ctx_mem.hpp -- who owns device memory: the allocations a context (or a preprocess plan) keeps, and the scratch a call borrows.
// Plain C++17, no HIP: the host compiler alone builds it (tests/ctx_mem_check.cpp drives it with a counting malloc that can fail).
//
// Both pieces take an allocator policy A with static  int A::alloc(void** p, size_t bytes)  (0: success) and  void A::free(void* p).
// The library's policy wraps the device allocator (HipMem, vbmf_hip.hip) and is the only place that names it.
//
//   MemOwner<A>    one member of vbmf_ctx and of vbmf_prep.  The fields stay plain typed pointers (kernels take them as arguments); the
//                  owner records the address of every field it has filled and frees each exactly once.  A new buffer acquires, and
//                  that is all: release_all() -- the whole of vbmf_destroy's device-memory part -- finds it.
//   Scratch<A, T>  a buffer that lives as long as a call: freed on every path out of the scope, early returns and HIPCHK / TRY included.
//
// Neither fills what it allocates.  A fill is work on a stream and the stream matters (see the call sites), so it stays there.
#pragma once

#include <cstddef>
#include <vector>

namespace vbmf {

constexpr int MEM_SLOT_BUSY = -1;      // acquire() into a slot that already holds a buffer: refused, the buffer is untouched

template <class A>
class MemOwner {
    struct Rec {
        void* slot;                    // address of the caller's typed pointer field
        void (*clear)(void* slot);     // nulls it as the type it has
        void* ptr;
        size_t bytes;
    };
    std::vector<Rec> recs_;

    template <class T>
    static void clear_as(void* slot) { *static_cast<T**>(slot) = nullptr; }
    void drop(const Rec& r) {
        A::free(r.ptr);
        r.clear(r.slot);
    }

public:
    MemOwner() = default;
    MemOwner(const MemOwner&) = delete;
    MemOwner& operator=(const MemOwner&) = delete;
    ~MemOwner() { release_all(); }

    // allocate into an empty slot and record it; on failure the slot stays null and the policy's code comes back
    template <class T>
    int acquire(T*& slot, size_t bytes) {
        if (slot) return MEM_SLOT_BUSY;
        void* p = nullptr;
        const int rc = A::alloc(&p, bytes);
        if (rc != 0) return rc;
        slot = static_cast<T*>(p);
        recs_.push_back(Rec{&slot, &clear_as<T>, p, bytes});
        return 0;
    }
    // free what the slot holds (if anything), then allocate the new size; on failure the slot is null.  The caller decides when:
    // the one buffer that grows, c->bags, is only ever regrown to a larger size.
    template <class T>
    int regrow(T*& slot, size_t bytes) {
        for (size_t i = 0; i < recs_.size(); ++i)
            if (recs_[i].slot == &slot) {
                drop(recs_[i]);
                recs_.erase(recs_.begin() + (std::ptrdiff_t)i);
                break;
            }
        return acquire(slot, bytes);
    }
    // all-or-nothing groups: rollback(m) frees everything acquired since m = mark() and nulls those slots
    size_t mark() const { return recs_.size(); }
    void rollback(size_t m) {
        while (recs_.size() > m) {
            drop(recs_.back());
            recs_.pop_back();
        }
    }
    void release_all() { rollback(0); }

    size_t live() const { return recs_.size(); }
    size_t live_bytes() const {
        size_t n = 0;
        for (const Rec& r : recs_) n += r.bytes;
        return n;
    }
};

template <class A, class T>
class Scratch {
    T* p_ = nullptr;

public:
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { reset(); }

    int alloc(size_t bytes) {
        if (p_) return MEM_SLOT_BUSY;
        void* p = nullptr;
        const int rc = A::alloc(&p, bytes);
        if (rc == 0) p_ = static_cast<T*>(p);
        return rc;
    }
    void reset() {
        if (p_) A::free(p_);
        p_ = nullptr;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
};

}  // namespace vbmf
