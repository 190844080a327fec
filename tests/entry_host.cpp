// The host helpers of csrc/ccx_entry.h -- the very header every `extern "C"` entry uses -- behind a C interface for
// tests/test_entry_host.py.  Compiled with a plain host C++17 compiler: the header needs no HIP include.
#include <cstdint>

#include "ccx_entry.h"

namespace {

// what the functor received, as bits (argument i true -> bit i), and how often it ran
struct Seen {
    int calls = 0;
    unsigned bits = 0;
    int count = 0;
};

template <class... T>
void note(Seen& s, T... flag) {
    ++s.calls;
    s.count = (int)sizeof...(T);
    unsigned i = 0;
    ((s.bits |= (decltype(flag)::value ? 1u : 0u) << i++), ...);
}

bool bit(unsigned bits, int i) { return ((bits >> i) & 1u) != 0; }

}  // namespace

extern "C" {

// with_flags over n = 1..4 flags taken from the low bits of `bits`: out = {calls, received bits, received count, returned value}
void host_with_flags(int n, unsigned bits, int* out) {
    Seen s;
    int ret = -1;
    switch (n) {
        case 1: ret = ccxi::with_flags([&](auto a) { note(s, a); return 11; }, bit(bits, 0)); break;
        case 2: ret = ccxi::with_flags([&](auto a, auto b) { note(s, a, b); return 12; }, bit(bits, 0), bit(bits, 1)); break;
        case 3:
            ret = ccxi::with_flags([&](auto a, auto b, auto c) { note(s, a, b, c); return 13; }, bit(bits, 0), bit(bits, 1), bit(bits, 2));
            break;
        case 4:
            ret = ccxi::with_flags([&](auto a, auto b, auto c, auto d) { note(s, a, b, c, d); return 14; }, bit(bits, 0), bit(bits, 1),
                                   bit(bits, 2), bit(bits, 3));
            break;
    }
    out[0] = s.calls, out[1] = (int)s.bits, out[2] = s.count, out[3] = ret;
}

// the flags reach the functor as TYPES: a combination shut out with `if constexpr` runs nothing (the entries keep kernels that
// are never launched out of the build this way).  Returns how often the body behind the `if constexpr` ran.
int host_with_flags_excluding_both_false(int a, int b) {
    int ran = 0;
    ccxi::with_flags([&](auto x, auto y) {
        if constexpr (decltype(x)::value || decltype(y)::value) ++ran;
    }, a != 0, b != 0);
    return ran;
}

// the addresses are never dereferenced; the three parameters have the pointer types the entries mix
int host_misaligned1(unsigned bytes, uintptr_t a) { return ccxi::misaligned(bytes, reinterpret_cast<const void*>(a)) ? 1 : 0; }
int host_misaligned3(unsigned bytes, uintptr_t a, uintptr_t b, uintptr_t c) {
    return ccxi::misaligned(bytes, reinterpret_cast<const float*>(a), reinterpret_cast<uint8_t*>(b), reinterpret_cast<void*>(c)) ? 1 : 0;
}

}  // extern "C"
