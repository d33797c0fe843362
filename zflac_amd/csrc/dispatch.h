// dispatch.h -- a run-time value picks a template argument: the launch_* functions of the .hip
// units turn (dtype, layout, ...) into a kernel instantiation with these, one nested call per
// parameter, instead of a switch per parameter and unit. Host code.
//
//   dispatch<A, B, C>(v, f)       f(std::integral_constant<.., X>{}) for the X of the list that v
//                                 equals; hipErrorInvalidValue if it equals none
//   dispatch_else<A, B, Z>(v, f)  the same, with the list's last entry for every other value
// f is a generic lambda that returns hipError_t; every entry of the list instantiates it.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/zflac_hip.h"

namespace zflac {

template <auto V, auto... Rest, typename T, typename F>
hipError_t dispatch(T v, F&& f) {
    if (v == (T)V) return f(std::integral_constant<decltype(V), V>{});
    if constexpr (sizeof...(Rest) != 0) return dispatch<Rest...>(v, f);
    else return hipErrorInvalidValue;
}

template <auto V, auto... Rest, typename T, typename F>
hipError_t dispatch_else(T v, F&& f) {
    if constexpr (sizeof...(Rest) != 0) {
        if (v != (T)V) return dispatch_else<Rest...>(v, f);
    }
    return f(std::integral_constant<decltype(V), V>{});
}

// The float dtypes of a dense tensor: F32, F16, BF16, else invalid
template <typename F>
hipError_t dispatch_float(int dtype, F&& f) {
    return dispatch<ZFLAC_EXPORT_F32, ZFLAC_EXPORT_F16, ZFLAC_EXPORT_BF16>(dtype, f);
}

}  // namespace zflac
