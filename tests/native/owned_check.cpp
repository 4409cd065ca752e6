// owned_check.cpp — host test of csrc/rt_owned.h (tests/test_owned_host.py): the owner of every event, stream and buffer of a context,
// instantiated for a fake handle (an index into a table, 0 = empty) whose destroy function counts.  A handle is destroyed exactly once,
// never twice, and the empty value never.  Prints OK.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../raytracing_engine_amd/csrc/rt_owned.h"

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                 \
        }                                                             \
    } while (0)

using Handle = int;
static std::vector<int> g_destroyed{0};  // per handle; entry 0 is the empty value's and stays 0
static long g_calls = 0;

static Handle create() {
    g_destroyed.push_back(0);
    return (Handle)g_destroyed.size() - 1;
}

static void destroy(Handle h) {
    g_calls++;
    if (h <= 0 || (size_t)h >= g_destroyed.size() || g_destroyed[(size_t)h] != 0) {
        std::printf("FAIL destroy(%d): %s\n", h, h == 0 ? "the empty value" : h < 0 || (size_t)h >= g_destroyed.size() ? "never created" : "a second time");
        std::exit(1);
    }
    g_destroyed[(size_t)h] = 1;
}

using Owner = rt::Owned<Handle, destroy>;

static int count(Handle h) { return g_destroyed[(size_t)h]; }

int main() {
    {  // exactly once, at scope end
        const Handle h = create();
        {
            Owner a(h);
            CHECK(a && a.get() == h && count(h) == 0);
        }
        CHECK(count(h) == 1);
    }
    {  // empty by default; reset() on an empty owner calls nothing
        const long before = g_calls;
        {
            Owner a;
            CHECK(!a && a.get() == 0);
            a.reset();
            CHECK(!a);
        }
        CHECK(g_calls == before);
    }
    {  // a moved-from owner is empty and destroys nothing
        const Handle h = create();
        {
            Owner a(h);
            Owner b(std::move(a));
            CHECK(!a && a.get() == 0 && b.get() == h && count(h) == 0);
            const long before = g_calls;
            a.reset();
            CHECK(g_calls == before);
        }
        CHECK(count(h) == 1);
    }
    {  // move assignment onto a full owner destroys the old handle once and takes the new one
        const Handle h1 = create(), h2 = create();
        {
            Owner a(h1), b(h2);
            a = std::move(b);
            CHECK(count(h1) == 1 && count(h2) == 0 && a.get() == h2 && !b);
        }
        CHECK(count(h1) == 1 && count(h2) == 1);
    }
    {  // self-move-assignment leaves the handle alive and owned
        const Handle h = create();
        {
            Owner a(h);
            Owner& same = a;
            a = std::move(same);
            CHECK(a.get() == h && count(h) == 0);
        }
        CHECK(count(h) == 1);
    }
    {  // reset(h) destroys the old handle before it holds h
        const Handle h1 = create(), h2 = create();
        {
            Owner a(h1);
            a.reset(h2);
            CHECK(count(h1) == 1 && count(h2) == 0 && a.get() == h2);
            a.reset();
            CHECK(count(h2) == 1 && !a);
        }
        CHECK(count(h1) == 1 && count(h2) == 1);
    }
    {  // release() hands the handle out and the owner no longer destroys it
        const Handle h = create();
        {
            Owner a(h);
            CHECK(a.release() == h && !a);
        }
        CHECK(count(h) == 0);
        destroy(h);  // the caller's
    }
    {  // a vector grown from capacity 1 moves its owners many times: 1000 live handles, each destroyed once by clear()
        std::vector<Owner> pool;
        pool.reserve(1);
        std::vector<Handle> made;
        for (int i = 0; i < 1000; i++) {
            made.push_back(create());
            pool.emplace_back(made.back());
        }
        CHECK(pool.size() == 1000);
        for (int i = 0; i < 1000; i++) CHECK(pool[(size_t)i].get() == made[(size_t)i] && count(made[(size_t)i]) == 0);
        pool.clear();
        for (Handle h : made) CHECK(count(h) == 1);
    }
    {  // an array of owners reset in a loop, as a context's members are, and then destroyed
        Handle made[11];
        {
            Owner ev[11];
            for (int i = 0; i < 11; i++) ev[i].reset(made[i] = create());
            for (Owner& e : ev) e.reset();
            for (Handle h : made) CHECK(count(h) == 1);
        }
        for (Handle h : made) CHECK(count(h) == 1);
    }
    // every handle that was created has been destroyed exactly once (destroy() itself refuses a second time), the empty value never
    CHECK(g_destroyed[0] == 0);
    for (size_t h = 1; h < g_destroyed.size(); h++) CHECK(g_destroyed[h] == 1);
    CHECK(g_calls == (long)g_destroyed.size() - 1);
    std::printf("OK %zu handles\n", g_destroyed.size() - 1);
    return 0;
}
