// pt_launch.h — path B, host side: what the launchers of more than one unit share.
#pragma once
#include "rt_internal.h"

#include <type_traits>

namespace rt {

// Call f with v as a compile-time constant (std::integral_constant): the launchers' way from run-time switches to template arguments.
template <class F>
static void with_bool(bool v, F&& f) {
    if (v) f(std::true_type{});
    else f(std::false_type{});
}

static inline bool valid_stack_cfg(const StackCfg& sk, uint32_t grid) { return sk.lds_cap >= 1 && sk.lds_cap <= 160 && (size_t)grid * 256u <= sk.spill_stride; }
static inline size_t stack_lds_bytes(const StackCfg& sk) { return (size_t)sk.lds_cap * 256 * sizeof(unsigned long long); }

// The persistent query kernels share one signature and one launch: 256 threads, the stacks' LDS, c->stream.  A launcher chooses the
// instantiation (with_bool) and hands it over.
template <class Query>
using QueryKernel = void (*)(const PtScene, const Query, uint32_t*, unsigned long long*, const StackCfg, uint32_t);
template <class Query>
static int launch_query(Ctx* c, QueryKernel<Query> kernel, const PtScene& sc, const Query& q, uint32_t* head, unsigned long long* stats, uint32_t grid, const StackCfg& sk,
                        uint32_t refill_min) {
    if (!valid_stack_cfg(sk, grid)) return c->fail(RT_ERR_INVALID, "bad traversal stack configuration");
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), stack_lds_bytes(sk), c->stream, sc, q, head, stats, sk, refill_min);
    RT_HIP(c, hipGetLastError());
    return RT_OK;
}

}  // namespace rt
