// host_parallel.h — the one thread helper of the host BVH builders (bvh_build.cpp, bvh_two_level.cpp).  Internal.
#pragma once
#include <sched.h>

#include <algorithm>
#include <cstddef>
#include <exception>
#include <system_error>
#include <thread>
#include <vector>

namespace rt {

// CPUs this process may run on (the GPU boxes grant a slice of the machine), at most 32
inline int host_threads() {
    cpu_set_t set;
    int n = 1;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
    return std::min(std::max(n, 1), 32);
}

// fn(i) for i in [0, n) on up to `threads` threads (contiguous chunks; fn must only touch item i's data).
// Nothing escapes a worker thread: an exception inside fn is carried back and rethrown here after every
// thread has been joined, and chunks whose thread could not be created (std::system_error: thread or
// process limit of the box) run on the calling thread, so the result never depends on how many started.
template <typename F>
void parallel_for(size_t n, int threads, size_t kMinPerThread, F fn) {
    const size_t want = std::min<size_t>((size_t)std::max(threads, 1), (n + kMinPerThread - 1) / kMinPerThread);
    if (want <= 1) {
        for (size_t i = 0; i < n; i++) fn(i);
        return;
    }
    std::vector<std::thread> pool;
    pool.reserve(want - 1);
    std::vector<std::exception_ptr> errs(want);
    const size_t chunk = (n + want - 1) / want;
    auto run = [&](size_t t) noexcept {
        try {
            for (size_t i = t * chunk; i < std::min(n, (t + 1) * chunk); i++) fn(i);
        } catch (...) {
            errs[t] = std::current_exception();
        }
    };
    for (size_t t = 1; t < want; t++) {
        try {
            pool.emplace_back(run, t);
        } catch (const std::system_error&) {
            break;
        }
    }
    run(0);
    for (size_t t = pool.size() + 1; t < want; t++) run(t);
    for (auto& th : pool) th.join();
    for (auto& e : errs)
        if (e) std::rethrow_exception(e);
}

}  // namespace rt
