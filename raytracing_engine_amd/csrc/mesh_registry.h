// mesh_registry.h — which host-built meshes are resident, so that contexts given the same mesh share one copy.
// Host code only (no HIP): the key of a mesh and a process-wide table of weak references, both tested without a GPU
// (tests/native/mesh_registry_check.cpp).
#pragma once
#include <cstdint>
#include <cstring>
#include <iterator>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>

namespace rt {

// Everything that decides what a host build puts on the device.  The parameters are compared as they are; the arrays are
// represented by two 64-bit hashes of every byte, so two different meshes with equal parameters are taken for one only if
// both hashes collide at once (about 2^-128 per pair of meshes for hashes that behave as independent random functions).
struct MeshKey {
    int device = -1;
    uint32_t n_tris = 0, levels = 0, chunks = 0;
    uint32_t builder = 0;  // the builder's own constants (SAH triangle cost, depth cap): two libraries in one process never share
    uint64_t h1 = 0, h2 = 0;
    bool operator<(const MeshKey& o) const {
        return std::tie(device, n_tris, levels, chunks, builder, h1, h2) < std::tie(o.device, o.n_tris, o.levels, o.chunks, o.builder, o.h1, o.h2);
    }
    bool operator==(const MeshKey& o) const { return !(*this < o) && !(o < *this); }
};

// Two hashes of one byte stream in one pass over it, each four interleaved lanes of 64-bit words (a 32-byte stripe per step) so the
// multiplies of a lane overlap with the other lanes'.  h1 has xxHash64's round (add, rotate, multiply), h2 MurmurHash3's
// (multiply, rotate, multiply, xor, rotate, multiply-add), with their own constants and seeds; both rounds are one-to-one in the
// word they take in, so inputs that differ in one word leave different lane states.  add() takes one whole array: its lanes
// start from the running state, and its length goes into it, so neither the order nor the split of the arrays can be confused.
class MeshHasher {
  public:
    void add(const void* data, size_t bytes) {
        const unsigned char* p = static_cast<const unsigned char*>(data);
        uint64_t a[4], b[4];
        for (int i = 0; i < 4; i++) {
            a[i] = s1_ + kLaneSeed[i];
            b[i] = fmix(s2_ ^ kLaneSeed[3 - i]);
        }
        size_t left = bytes;
        for (; left >= 32; left -= 32, p += 32) {
            uint64_t w[4];
            std::memcpy(w, p, 32);
            stripe(a, b, w);
        }
        if (left) {  // the tail, zero-filled: the length below tells it from a stream that ends in zeros
            uint64_t w[4] = {0, 0, 0, 0};
            std::memcpy(w, p, left);
            stripe(a, b, w);
        }
        for (int i = 0; i < 4; i++) {
            s1_ = (s1_ ^ round1(0, a[i])) * kP1 + kP4;
            s2_ = fmix(s2_ ^ b[i]) + kLaneSeed[i];
        }
        s1_ = avalanche1(s1_ + (uint64_t)bytes);
        s2_ = fmix(s2_ ^ ((uint64_t)bytes * kC1));
    }
    uint64_t h1() const { return s1_; }
    uint64_t h2() const { return s2_; }

  private:
    static constexpr uint64_t kP1 = 0x9E3779B185EBCA87ull, kP2 = 0xC2B2AE3D27D4EB4Full, kP3 = 0x165667B19E3779F9ull, kP4 = 0x85EBCA77C2B2AE63ull;
    static constexpr uint64_t kC1 = 0x87C37B91114253D5ull, kC2 = 0x4CF5AD432745937Full;
    static constexpr uint64_t kLaneSeed[4] = {0x243F6A8885A308D3ull, 0x13198A2E03707344ull, 0xA4093822299F31D0ull, 0x082EFA98EC4E6C89ull};
    static uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
    static uint64_t round1(uint64_t acc, uint64_t w) { return rotl(acc + w * kP2, 31) * kP1; }
    static uint64_t round2(uint64_t h, uint64_t w) {
        w *= kC1;
        w = rotl(w, 31);
        w *= kC2;
        return rotl(h ^ w, 27) * 5u + 0x52DCE729u;
    }
    static uint64_t avalanche1(uint64_t h) {
        h ^= h >> 33;
        h *= kP2;
        h ^= h >> 29;
        h *= kP3;
        return h ^ (h >> 32);
    }
    static uint64_t fmix(uint64_t k) {
        k ^= k >> 33;
        k *= 0xFF51AFD7ED558CCDull;
        k ^= k >> 33;
        k *= 0xC4CEB9FE1A85EC53ull;
        return k ^ (k >> 33);
    }
    static void stripe(uint64_t a[4], uint64_t b[4], const uint64_t w[4]) {
        for (int i = 0; i < 4; i++) {
            a[i] = round1(a[i], w[i]);
            b[i] = round2(b[i], w[i]);
        }
    }
    uint64_t s1_ = 0x452821E638D01377ull, s2_ = 0xBE5466CF34E90C6Cull;
};

inline MeshKey mesh_key(int device, const float* verts, const float* albedo, const float* emission, uint32_t n_tris, uint32_t levels, uint32_t chunks,
                        uint32_t builder) {
    MeshHasher h;
    h.add(verts, (size_t)n_tris * 36);
    h.add(albedo, (size_t)n_tris * 12);
    h.add(emission, (size_t)n_tris * 12);
    MeshKey k;
    k.device = device;
    k.n_tris = n_tris;
    k.levels = levels;
    k.chunks = levels == 2u ? chunks : 0u;  // a single-level build does not read it
    k.builder = builder;
    k.h1 = h.h1();
    k.h2 = h.h2();
    return k;
}

// Key -> weak reference to what is resident under it.  The table never keeps a mesh alive: an entry whose mesh has gone is
// dropped by the next call.  Counting and un-listing happen under the table's mutex, and so does every step that turns a weak
// reference into a strong one, so "this is the only holder" stays true once un-listed.
template <class T>
class WeakRegistry {
  public:
    std::shared_ptr<T> find(const MeshKey& k) {
        std::lock_guard<std::mutex> g(mu_);
        purge();
        auto it = map_.find(k);
        return it == map_.end() ? nullptr : it->second.lock();
    }
    // lists v under k unless a live mesh is listed there already (two threads that built the same mesh: both keep theirs)
    void insert(const MeshKey& k, const std::shared_ptr<T>& v) {
        std::lock_guard<std::mutex> g(mu_);
        purge();
        map_.emplace(k, v);
    }
    long holders(const std::shared_ptr<T>& v) {
        std::lock_guard<std::mutex> g(mu_);
        return v ? v.use_count() : 0;
    }
    // Before a holder writes into v.  true: others hold it too (it stays listed, the caller writes into a copy of its own);
    // false: the caller is the only holder and v is no longer listed, so it stays the only one
    bool shared_or_unlist(const std::shared_ptr<T>& v) {
        std::lock_guard<std::mutex> g(mu_);
        if (v.use_count() > 1) return true;
        for (auto it = map_.begin(); it != map_.end();)
            it = (!it->second.owner_before(v) && !v.owner_before(it->second)) ? map_.erase(it) : std::next(it);
        return false;
    }
    size_t size() {
        std::lock_guard<std::mutex> g(mu_);
        purge();
        return map_.size();
    }

  private:
    void purge() {
        for (auto it = map_.begin(); it != map_.end();) it = it->second.expired() ? map_.erase(it) : std::next(it);
    }
    std::mutex mu_;
    std::map<MeshKey, std::weak_ptr<T>> map_;
};

}  // namespace rt
