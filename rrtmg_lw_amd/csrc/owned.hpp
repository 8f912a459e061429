// Ownership of the driver's GPU resources (driver.hip: device and pinned buffers, streams, events, graphs), free of HIP so that a
// stand-alone host program can exercise it over counting traits (tests/cpp/owned_check.cpp).  A Traits names the handle type (its
// value-initialised value means "none") and how one is released - `static int release(handle)`, 0 or an error code - and, for
// buffers, acquired: `static int acquire(handle *, size_t bytes)`.
#pragma once
#include <cstddef>
#include <new>
#include <utility>

namespace owned {

// One handle, released exactly once: by reset(), by a move-assignment over it, or by the destructor.
template <class Traits>
class Owned {
public:
    using handle = typename Traits::handle;
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : h_(o.h_) { o.h_ = handle{}; }
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) { (void)reset(); h_ = o.h_; o.h_ = handle{}; }
        return *this;
    }
    ~Owned() { (void)reset(); }
    // releases what is held, if anything; the owner is empty afterwards whatever release() answers
    int reset()
    {
        if (!h_) return 0;
        const handle h = h_;
        h_ = handle{};
        return Traits::release(h);
    }
    handle get() const { return h_; }
    explicit operator bool() const { return h_ != handle{}; }
    // where a create call writes its result - hipStreamCreate(s.slot()); a handle still held is released first
    handle *slot() { (void)reset(); return &h_; }

private:
    handle h_{};
};

// An Owned buffer and its capacity in bytes.  How much to allocate is the caller's policy (reserve's `want`).
template <class Traits>
class GrowBuf {
public:
    using handle = typename Traits::handle;
    GrowBuf() = default;
    GrowBuf(GrowBuf &&o) noexcept : own_(std::move(o.own_)), cap_(o.cap_) { o.cap_ = 0; }
    GrowBuf &operator=(GrowBuf &&o) noexcept
    {
        if (this != &o) { own_ = std::move(o.own_); cap_ = o.cap_; o.cap_ = 0; }
        return *this;
    }
    // Room for `need` bytes: nothing happens when the capacity suffices; otherwise the old buffer is released FIRST and `want` (>= need)
    // bytes are allocated.  A failed release or allocation leaves the buffer empty with capacity 0 and hands the traits' code back.
    int reserve(size_t need, size_t want)
    {
        if (cap_ >= need) return 0;
        if (const int rc = reset()) return rc;
        handle h{};
        if (const int rc = Traits::acquire(&h, want)) return rc;
        *own_.slot() = h;
        cap_ = want;
        return 0;
    }
    int reset() { cap_ = 0; return own_.reset(); }
    size_t bytes() const { return cap_; }
    handle get() const { return own_.get(); }
    template <class T> T *as() const { return static_cast<T *>(own_.get()); }
    explicit operator bool() const { return (bool)own_; }

private:
    Owned<Traits> own_;
    size_t cap_ = 0;
};

// A T that is constructed and never destroyed: for globals whose members' release functions must not run from static destructors at
// process exit (the runtime they would call into may be gone by then).  Whoever owns the T releases its contents explicitly.
template <class T>
class NoDestroy {
public:
    template <class... A> explicit NoDestroy(A &&...a) { new (buf_) T(std::forward<A>(a)...); }
    NoDestroy(const NoDestroy &) = delete;
    NoDestroy &operator=(const NoDestroy &) = delete;
    T &get() { return *std::launder(reinterpret_cast<T *>(buf_)); }

private:
    alignas(T) unsigned char buf_[sizeof(T)];
};

}   // namespace owned
