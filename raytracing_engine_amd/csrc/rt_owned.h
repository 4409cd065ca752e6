// rt_owned.h — the move-only owner of one handle: everything a context holds that is not plain memory of its own (events, streams,
// pinned memory, child contexts, frame slots, the communicator) is a member of this type, instantiated in rt_internal.h.
// Host code only (no HIP), so that it is tested without a GPU (tests/native/owned_check.cpp).
#pragma once

namespace rt {

// Owns handle h from the moment it is given it until it is destroyed, reset, moved from or released; Destroy(h) runs exactly once for
// a handle that is not released.  The empty value is H{} (a null pointer for every handle of the library) and is never destroyed.
template <class H, void (*Destroy)(H)>
class Owned {
   public:
    Owned() = default;
    explicit Owned(H h) : h_(h) {}
    Owned(Owned&& o) noexcept : h_(o.release()) {}
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) reset(o.release());
        return *this;
    }
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { reset(); }

    H get() const { return h_; }
    explicit operator bool() const { return h_ != H{}; }
    void reset(H h = H{}) {  // what it held goes first
        if (h_ != H{}) Destroy(h_);
        h_ = h;
    }
    H release() {  // the caller's from now on
        H h = h_;
        h_ = H{};
        return h;
    }

   private:
    H h_{};
};

}  // namespace rt
