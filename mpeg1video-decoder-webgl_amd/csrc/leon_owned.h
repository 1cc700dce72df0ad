// leon_owned.h -- owning types for what the host code gets from the runtime and must give back: device and pinned memory,
// streams, events.  Plain C++17 with no HIP include: how to get and give back is a policy (the production ones stand in
// leon_hip.cpp beside big_alloc; tests/native/owned_check.cpp has a counting one that fails on demand).
//
// All types are move-only.  A destructor gives back what the object owns, once; a moved-from object is empty.
//
// A memory policy:   static void* get(size_t bytes, tag...);     nullptr: refused
//                    static void give(void* p);
//                    static constexpr bool kHostAddressable;     reserve() may memcpy between two of its buffers
// A handle policy:   using type = ...;                           a pointer-like handle, type{} = none
//                    static type create(args...);                type{}: refused
//                    static void destroy(type h);
//
// RESOURCES MADE TOGETHER AT FIRST USE (a device ring and its pinned twin, a stream and its events) are built in locals and
// move-assigned into their members only when all of them exist:
//
//     if (!d->ring) {
//         Ring ring; Pinned twin;
//         if (!ring.alloc(n) || !twin.alloc(n)) return fail(...);      // the locals' destructors undo what was made
//         d->ring = std::move(ring); d->twin = std::move(twin);        // all or none: `!d->ring` speaks for the group
//     }
//
// so that a failure half way never leaves a member set whose partner is not (Mirror::alloc is this idiom for a pair).
#pragma once

#include <cassert>
#include <cstddef>
#include <cstring>
#include <utility>

namespace leon_owned {

// ---- capacities of the buffers that grow to a high-water mark and never shrink ------------------------------------------
// what a buffer asked for `need` (bytes or elements: the caller's unit) is allocated at: exactly that, half again or twice
// that, and `at_least`
enum class Grow { Exact, Half, Twice };
constexpr size_t cap_for(size_t need, Grow g, size_t at_least = 0)
{
    const size_t cap = g == Grow::Exact ? need : g == Grow::Half ? need + need / 2 : need * 2;
    return cap > at_least ? cap : at_least;
}

// ---- memory ---------------------------------------------------------------------------------------------------------------
template <class Mem, class T = char>
class Buffer {
public:
    Buffer() = default;
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    Buffer(Buffer&& o) noexcept : p_(o.p_), bytes_(o.bytes_), owned_(o.owned_) { o.forget(); }
    Buffer& operator=(Buffer&& o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_; bytes_ = o.bytes_; owned_ = o.owned_;
            o.forget();
        }
        return *this;
    }
    ~Buffer() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }       // reads like the pointer it holds: d->ring + at, kernel arguments, memcpy
    T* operator->() const { return p_; }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }

    void reset()
    {
        if (p_ && owned_) Mem::give(p_);
        forget();
    }
    // gives up ownership: the caller frees it (a borrowed view is simply forgotten)
    T* release()
    {
        T* p = p_;
        forget();
        return p;
    }
    // `bytes` of memory for an EMPTY buffer; false (and still empty): refused, or not empty
    template <class... Tag> bool alloc(size_t bytes, Tag... tag)
    {
        if (p_) return false;
        p_ = static_cast<T*>(Mem::get(bytes, tag...));
        if (!p_) return false;
        bytes_ = bytes;
        owned_ = true;
        return true;
    }
    // a view of memory somebody else owns (a piece of a slab): never given back
    void borrow(T* p, size_t bytes)
    {
        reset();
        p_ = p; bytes_ = bytes; owned_ = false;
    }
    // Grow, never shrink: at least `need` bytes.  A buffer that has them stays as it is; else `cap` bytes are allocated FIRST
    // and the old buffer is given back only then -- false leaves pointer, size and contents as they were.  The new buffer's
    // contents are undefined but for the first `preserve` bytes (host-addressable memory only), copied from the old one.  A
    // borrowed view that grows becomes an owned buffer; its lender keeps the old memory.
    template <class... Tag> bool reserve(size_t need, size_t cap, size_t preserve = 0, Tag... tag)
    {
        if (need <= bytes_) return true;
        assert(cap >= need && (preserve == 0 || Mem::kHostAddressable));
        T* p = static_cast<T*>(Mem::get(cap, tag...));
        if (!p) return false;
        if (preserve && p_) std::memcpy(p, p_, preserve < bytes_ ? preserve : bytes_);
        reset();
        p_ = p; bytes_ = cap; owned_ = true;
        return true;
    }

private:
    void forget() { p_ = nullptr; bytes_ = 0; owned_ = false; }
    T* p_ = nullptr;
    size_t bytes_ = 0;
    bool owned_ = false;
};

// A pinned host array and its device twin of the same element count: both or neither.
template <class HostMem, class DevMem, class T = char>
class Mirror {
public:
    T* host() const { return host_.get(); }
    T* dev() const { return dev_.get(); }
    size_t count() const { return host_.bytes() / sizeof(T); }
    explicit operator bool() const { return (bool)host_; }
    void reset() { host_.reset(); dev_.reset(); }
    // n elements each, for an EMPTY mirror; false: it is still empty
    bool alloc(size_t n)
    {
        if (host_) return false;
        Buffer<HostMem, T> h;
        Buffer<DevMem, T> d;
        if (!d.alloc(n * sizeof(T)) || !h.alloc(n * sizeof(T))) return false;
        host_ = std::move(h);
        dev_ = std::move(d);
        return true;
    }
    // at least `need` elements, allocated at `cap`: the new pair first, the old one given back then; contents are dropped
    bool reserve(size_t need, size_t cap)
    {
        if (need <= count()) return true;
        Mirror m;
        if (!m.alloc(cap)) return false;
        *this = std::move(m);
        return true;
    }

private:
    Buffer<HostMem, T> host_;
    Buffer<DevMem, T> dev_;
};

// ---- streams and events -----------------------------------------------------------------------------------------------------
template <class Traits>
class Handle {
public:
    using type = typename Traits::type;
    Handle() = default;
    Handle(const Handle&) = delete;
    Handle& operator=(const Handle&) = delete;
    Handle(Handle&& o) noexcept : h_(o.h_), owned_(o.owned_) { o.forget(); }
    Handle& operator=(Handle&& o) noexcept
    {
        if (this != &o) {
            reset();
            h_ = o.h_; owned_ = o.owned_;
            o.forget();
        }
        return *this;
    }
    ~Handle() { reset(); }

    type get() const { return h_; }
    operator type() const { return h_; }
    explicit operator bool() const { return h_ != type{}; }
    void reset()
    {
        if (h_ != type{} && owned_) Traits::destroy(h_);
        forget();
    }
    // for an EMPTY handle; false: refused (or not empty), and it is as it was
    template <class... A> bool create(A... a)
    {
        if (h_ != type{}) return false;
        h_ = Traits::create(a...);
        owned_ = h_ != type{};
        return owned_;
    }
    // somebody else's (the caller's stream): used, never destroyed
    void borrow(type h)
    {
        reset();
        h_ = h; owned_ = false;
    }

private:
    void forget() { h_ = type{}; owned_ = false; }
    type h_{};
    bool owned_ = false;
};

}  // namespace leon_owned
