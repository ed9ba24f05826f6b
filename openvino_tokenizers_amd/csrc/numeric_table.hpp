// numeric_table.hpp -- host side of NumericToString's float path: the table of 128-bit powers of ten the kernel multiplies by
// (numeric_kernels.hpp).  Plain C++ (no HIP): exact big-integer arithmetic on 32-bit limbs, run once per process.
//
// Entry p (kNumPow10Min <= p <= kNumPow10Max) holds t = floor(10^p / 2^te), te = floor(p * log2(10)) - 127, so that
// 2^127 <= t < 2^128 and t * 2^te <= 10^p < (t + 1) * 2^te; the entry is exact (t * 2^te == 10^p) for 0 <= p <= kNumPow10ExactMax.
// The kernel computes te with num_pow10_exp(); the builder checks that formula against the exact bit lengths for every entry.
#pragma once

#include <stdint.h>

#include <vector>

namespace ovtk {

struct NumPow10 {
    unsigned long long hi, lo;
};
constexpr int kNumPow10Min = -305, kNumPow10Max = 331;   // 5 - X for X in -326..310: every decimal exponent of a double, one to spare each way
constexpr int kNumPow10ExactMax = 55;                    // 5^55 < 2^128 < 5^56
constexpr int num_pow10_exp(int p) { return ((p * 1741647) >> 19) - 127; }   // floor(p * log2(10)) - 127 for |p| <= 340 (checked below)

namespace numtab {

using Big = std::vector<uint32_t>;   // little-endian limbs, no leading zero limb (zero: empty)

inline void mul_small(Big& a, uint32_t m) {
    uint64_t carry = 0;
    for (uint32_t& w : a) {
        const uint64_t t = uint64_t(w) * m + carry;
        w = uint32_t(t);
        carry = t >> 32;
    }
    if (carry) a.push_back(uint32_t(carry));
}
inline void div_small(Big& a, uint32_t d) {   // a = floor(a / d)
    uint64_t rem = 0;
    for (size_t i = a.size(); i-- > 0;) {
        const uint64_t t = (rem << 32) | a[i];
        a[i] = uint32_t(t / d);
        rem = t % d;
    }
    while (!a.empty() && a.back() == 0) a.pop_back();
}
inline int bit_length(const Big& a) {
    if (a.empty()) return 0;
    int top = 0;
    for (uint32_t w = a.back(); w; w >>= 1) ++top;
    return int(a.size() - 1) * 32 + top;
}
inline int bit_at(const Big& a, int k) { return k >= 0 && size_t(k >> 5) < a.size() ? int((a[size_t(k >> 5)] >> (k & 31)) & 1u) : 0; }
// bits [from, from + 128) of a (bits below 0 read as 0)
inline NumPow10 bits128(const Big& a, int from) {
    NumPow10 r{0, 0};
    for (int k = 0; k < 64; ++k) {
        r.lo |= (unsigned long long)bit_at(a, from + k) << k;
        r.hi |= (unsigned long long)bit_at(a, from + 64 + k) << k;
    }
    return r;
}
inline Big pow5(int q) {
    Big a{1u};
    for (; q >= 13; q -= 13) mul_small(a, 1220703125u);   // 5^13
    for (; q > 0; --q) mul_small(a, 5u);
    return a;
}

}  // namespace numtab

// -> false if num_pow10_exp() disagrees with an exact exponent (it does not: the check is what makes the formula safe to use)
inline bool build_num_pow10_table(std::vector<NumPow10>& out) {
    using namespace numtab;
    out.assign(size_t(kNumPow10Max - kNumPow10Min + 1), NumPow10{0, 0});
    for (int p = kNumPow10Min; p <= kNumPow10Max; ++p) {
        NumPow10 t;
        int te;
        if (p >= 0) {   // 10^p = 5^p * 2^p: the top 128 bits of 5^p (all of them while they fit)
            const Big b = pow5(p);
            const int bl = bit_length(b);
            t = bits128(b, bl - 128);
            te = bl - 128 + p;
        } else {        // 10^p = 2^p / 5^q: floor(2^(bl + 127) / 5^q) has exactly 128 bits (5^q is no power of two)
            const int q = -p, bl = bit_length(pow5(q));
            Big num(size_t((bl + 127) / 32 + 1), 0u);
            num.back() = 1u << ((bl + 127) & 31);
            int left = q;
            for (; left >= 13; left -= 13) div_small(num, 1220703125u);   // floor(floor(x / a) / b) == floor(x / (a * b))
            for (; left > 0; --left) div_small(num, 5u);
            if (bit_length(num) != 128) return false;
            t = bits128(num, 0);
            te = -(bl + 127) + p;
        }
        if (!(t.hi >> 63) || te != num_pow10_exp(p)) return false;
        out[size_t(p - kNumPow10Min)] = t;
    }
    return true;
}

}  // namespace ovtk
