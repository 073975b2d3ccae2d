// dispatch.h -- a runtime value into a compile-time constant.  Plain C++17, no HIP: the launch layer (sgpu_runtime.hip) picks
// its __global__ template instantiations through it, and a host compiler can test it (tests/test_dispatch.py).
//
//   among<V0, V1, ...>(v, f)   f(std::integral_constant<int, Vk>{}) for the listed Vk == v; for a v that is not listed f is not
//                              called and the result is value-initialised (nullptr for a kernel pointer: no kernel, never another one)
//   with_bool(b, f)            f(std::true_type{}) or f(std::false_type{})
//
// f is a generic lambda and the calls nest:
//   among<1, 2, 4>(lanes, [&](auto G) { return with_bool(halo, [&](auto H) -> Fn { return kernel<G(), H()>; }); });
// f returns the same type for every listed value.  That type is deduced from the FIRST LISTED value, never from a value
// outside the list: deducing it would instantiate f -- and the kernel it names -- for that value too.
#pragma once
#include <type_traits>

namespace dispatch {

template <int V0, int... Vs, class F>
auto among(int v, F &&f) {
    using R = decltype(f(std::integral_constant<int, V0>{}));
    R r{};
    const auto hit = [&](auto c) { return v == c() && (r = f(c), true); };
    (void)(hit(std::integral_constant<int, V0>{}) || ... || hit(std::integral_constant<int, Vs>{}));
    return r;
}

template <class F>
auto with_bool(bool b, F &&f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

}   // namespace dispatch
