// Runtime int -> compile-time constant, for picking a kernel instantiation:
//   pick_range<2, 11>(K, [&](auto K_) -> kernel_t { return kernel<K_()>; })
// calls the generic lambda with std::integral_constant<int, V> for the V of the set that equals the
// runtime value, and returns nullptr (no call) for a value outside the set.
#pragma once
#include <type_traits>
#include <utility>

namespace nfx {

template <int... Vs, class F>
auto pick_of(int v, F f) {  // v in the explicit list Vs...
    std::common_type_t<decltype(f(std::integral_constant<int, Vs>{}))...> r = nullptr;
    (void)((v == Vs && (r = f(std::integral_constant<int, Vs>{}), true)) || ...);
    return r;
}

template <int Lo, int... Is, class F>
auto pick_offset(int v, F f, std::integer_sequence<int, Is...>) {
    return pick_of<(Lo + Is)...>(v, f);
}

template <int Lo, int Hi, class F>
auto pick_range(int v, F f) {  // v in Lo..Hi, both ends included
    return pick_offset<Lo>(v, f, std::make_integer_sequence<int, Hi - Lo + 1>{});
}

}  // namespace nfx
