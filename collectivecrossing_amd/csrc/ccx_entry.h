// ccx_entry.h -- what the `extern "C"` entries of the C-ABI layer share around their launches: the alignment test of their
// pointer arguments and the step from run-time flags to a kernel's template parameters.  Host code, plain C++17: no HIP
// header is needed to compile it (tests/entry_host.cpp does so with the host compiler).  ccx_internal.h includes it.
#pragma once
#include <cstdint>
#include <type_traits>

namespace ccxi {

// True when any of the pointers has a bit below `bytes` (a power of two) set.  A null pointer contributes nothing: an
// `*_or_null` argument goes in as it is.
template <class... More>
inline bool misaligned(unsigned bytes, const void* p, const More*... more) {
    return ((reinterpret_cast<uintptr_t>(p) | ... | reinterpret_cast<uintptr_t>(static_cast<const void*>(more))) &
            (uintptr_t)(bytes - 1u)) != 0;
}

// Calls f exactly once, with one std::true_type / std::false_type per flag, in the flags' order:
//     with_flags([&](auto mask, auto ent) { hipLaunchKernelGGL((kernel<decltype(mask)::value, decltype(ent)::value>), ...); },
//                masks_or_null != nullptr, entropy_or_null != nullptr);
// A flag cannot reach another parameter than the one written next to it, and the launch line is written once.  Every
// combination of the flags instantiates f's body: a combination that is never launched is kept out of the build by an
// `if constexpr` around the launch.
// with_flags returns what f returns (an entry whose launch needs a checked call first hands its code back through it).
template <class F>
inline decltype(auto) with_flags(F&& f) {
    return f();
}
template <class F, class... Rest>
inline decltype(auto) with_flags(F&& f, bool flag, Rest... rest) {
    static_assert((std::is_same_v<Rest, bool> && ...), "with_flags takes bools: write `p != nullptr` for a pointer");
    if (flag) return with_flags([&](auto... tail) -> decltype(auto) { return f(std::true_type{}, tail...); }, rest...);
    return with_flags([&](auto... tail) -> decltype(auto) { return f(std::false_type{}, tail...); }, rest...);
}

}  // namespace ccxi
