// csr_lane.hpp — the compiled instantiations of the one-lane-per-receiver CSR kernels of rules
// WEIGHTED and PUSHSUM (k_round_weighted, k_round_pushsum): one width list, one selection.
// Both kernels read the same well / avell arrays, so they share their widths by construction.
#pragma once

#include <type_traits>

#include "engine.hpp"

namespace acs {

// The width list: calls f(integral_constant<int, D>) for the compiled width D == d; false, with f
// not called, when d is not one.
template <typename F>
bool csr_lane_width(uint32_t d, F&& f) {
    auto at = [&](auto w) {
        if (d != (uint32_t)w()) return false;
        f(w);
        return true;
    };
    return at(std::integral_constant<int, 4>()) || at(std::integral_constant<int, 8>()) ||
           at(std::integral_constant<int, 16>()) || at(std::integral_constant<int, 32>());
}

// the padded degrees with a compiled per-lane kernel (create.hip asks this for both rules)
inline bool csr_lane_fast_supported(uint32_t d) {
    return csr_lane_width(d, [](auto) {});
}

// Calls f(integral_constant<int, D>, VT(), bool_constant<SCHED>) for the handle's instantiation:
// D = a.d, VT = float where a.f32 and else double, SCHED = the handle has a link schedule (a.avell).
// False, with f not called, when a.d is not a compiled width.
template <typename F>
bool csr_lane_select(const RoundArgs& a, F&& f) {
    return csr_lane_width(a.d, [&](auto d) {
        if (a.avell && a.f32)
            f(d, float(), std::true_type());
        else if (a.avell)
            f(d, double(), std::true_type());
        else if (a.f32)
            f(d, float(), std::false_type());
        else
            f(d, double(), std::false_type());
    });
}

}  // namespace acs
