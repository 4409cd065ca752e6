// mesh_registry_check.cpp — host test of csrc/mesh_registry.h (tests/test_mesh_registry_host.py): the key of a mesh reacts to every
// input, and the table of resident meshes shares, forgets and un-lists as DESIGN.md §6.12 says, also with threads.  Prints OK.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <thread>
#include <vector>

#include "../../raytracing_engine_amd/csrc/mesh_registry.h"

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                 \
        }                                                             \
    } while (0)

struct Mesh {
    int payload = 0;
};

static rt::MeshKey key_of(const std::vector<float>& v, const std::vector<float>& a, const std::vector<float>& e, uint32_t n, int device = 0, uint32_t levels = 1,
                          uint32_t chunks = 64, uint32_t builder = 7) {
    return rt::mesh_key(device, v.data(), a.data(), e.data(), n, levels, chunks, builder);
}

int main() {
    // ---- the key --------------------------------------------------------------------------------------------------------
    for (uint32_t n : {1u, 2u, 3u, 7u, 8u, 9u, 100u, 4097u}) {  // array sizes around the 32-byte stripe
        std::mt19937 rng(n);
        std::uniform_real_distribution<float> u(-1.0f, 1.0f);
        std::vector<float> v(9 * (size_t)n + 9), a(3 * (size_t)n + 3), e(3 * (size_t)n + 3);
        for (float& x : v) x = u(rng);
        for (float& x : a) x = u(rng);
        for (float& x : e) x = 0.0f;
        const rt::MeshKey k = key_of(v, a, e, n);
        CHECK(k == key_of(v, a, e, n));
        std::vector<float> v2 = v, a2 = a, e2 = e;  // equal bytes at other addresses
        CHECK(k == key_of(v2, a2, e2, n));
        std::set<std::pair<uint64_t, uint64_t>> seen{{k.h1, k.h2}};
        std::set<uint64_t> seen1{k.h1}, seen2{k.h2};
        size_t variants = 1;
        auto differs = [&](const rt::MeshKey& o) {
            variants++;
            seen.insert({o.h1, o.h2});
            seen1.insert(o.h1);
            seen2.insert(o.h2);
            return !(o == k);
        };
        // every single float of every array, changed in its last bit and in its sign
        for (int which = 0; which < 3; which++) {
            std::vector<float>& arr = which == 0 ? v2 : which == 1 ? a2 : e2;
            const size_t used = (which == 0 ? 9 : 3) * (size_t)n;
            for (size_t i = 0; i < used; i += (used > 600 ? 37 : 1)) {
                const float keep = arr[i];
                uint32_t bits;
                std::memcpy(&bits, &keep, 4);
                bits ^= 1u;
                std::memcpy(&arr[i], &bits, 4);
                CHECK(differs(key_of(v2, a2, e2, n)));
                bits ^= 0x80000001u;  // the sign alone: -0.0 is not 0.0 here
                std::memcpy(&arr[i], &bits, 4);
                CHECK(differs(key_of(v2, a2, e2, n)));
                arr[i] = keep;
            }
            // floats past the arrays' used part are not read
            arr[used] += 1.0f;
            CHECK(k == key_of(v2, a2, e2, n));
            arr[used] = (which == 0 ? v : which == 1 ? a : e)[used];
        }
        CHECK(seen.size() == variants && seen1.size() == variants && seen2.size() == variants);  // each hash alone told them all apart
        // parameters
        CHECK(!(k == key_of(v, a, e, n, 1)));
        CHECK(!(k == key_of(v, a, e, n, 0, 2)));
        CHECK(k == key_of(v, a, e, n, 0, 1, 32));  // a single-level build does not read the chunk count
        CHECK(!(key_of(v, a, e, n, 0, 2, 64) == key_of(v, a, e, n, 0, 2, 32)));
        CHECK(!(k == key_of(v, a, e, n, 0, 1, 64, 8)));
        if (n > 1) CHECK(!(k == key_of(v, a, e, n - 1)));
        // a value that moves from the end of one array to the start of the next is another mesh
        if (n == 1) {
            std::vector<float> va(9, 0.0f), aa(3, 0.0f), ea(3, 0.0f), vb = va, ab = aa;
            va[8] = 1.0f;
            ab[0] = 1.0f;
            CHECK(!(key_of(va, aa, ea, 1) == key_of(vb, ab, ea, 1)));
        }
    }

    // ---- the table -------------------------------------------------------------------------------------------------------
    {
        rt::WeakRegistry<Mesh> reg;
        rt::MeshKey k1, k2;
        k1.h1 = 1;
        k2.h1 = 2;
        CHECK(!reg.find(k1));
        auto m1 = std::make_shared<Mesh>();
        CHECK(reg.holders(m1) == 1 && reg.holders(nullptr) == 0);
        reg.insert(k1, m1);
        CHECK(reg.holders(m1) == 1);  // the table holds no strong reference
        auto s = reg.find(k1);
        CHECK(s == m1 && reg.holders(m1) == 2 && !reg.find(k2));
        auto other = std::make_shared<Mesh>();
        reg.insert(k1, other);  // a live mesh is listed there: it stays
        CHECK(reg.find(k1) == m1);
        CHECK(reg.shared_or_unlist(m1));  // two holders: stays listed
        CHECK(reg.find(k1) == m1);
        s.reset();
        CHECK(!reg.shared_or_unlist(m1));  // sole holder: un-listed
        CHECK(!reg.find(k1) && reg.size() == 0);
        CHECK(!reg.shared_or_unlist(other));  // never listed: nothing to do
        reg.insert(k1, m1);
        reg.insert(k2, other);
        CHECK(reg.size() == 2);
        m1.reset();  // the mesh dies with its last holder, the entry with it
        CHECK(!reg.find(k1) && reg.size() == 1 && reg.find(k2) == other);
        reg.insert(k1, other);  // a dead entry does not block a new one
        CHECK(reg.find(k1) == other);
    }
    {
        // threads: each either finds the mesh of its key or builds and lists one; now and then a holder "writes" (shared_or_unlist,
        // then a change of its payload only if it is the sole holder).  A mesh found in the table must never have been written.
        rt::WeakRegistry<Mesh> reg;
        std::atomic<int> bad{0}, found{0}, built{0};
        std::vector<std::thread> th;
        for (int t = 0; t < 8; t++)
            th.emplace_back([&, t] {
                std::mt19937 rng(t);
                for (int i = 0; i < 20000; i++) {
                    rt::MeshKey k;
                    k.h1 = rng() % 4;
                    std::shared_ptr<Mesh> m = reg.find(k);
                    if (m) {
                        found++;
                        if (m->payload != 0) bad++;
                    } else {
                        m = std::make_shared<Mesh>();
                        built++;
                        reg.insert(k, m);
                    }
                    if (rng() % 3 == 0 && !reg.shared_or_unlist(m)) m->payload = 1;
                    if (reg.holders(m) < 1) bad++;
                }
            });
        for (auto& x : th) x.join();
        CHECK(bad == 0 && found > 0 && built > 0);
        CHECK(reg.size() == 0);
    }
    std::printf("OK\n");
    return 0;
}
