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

}  // namespace rt
