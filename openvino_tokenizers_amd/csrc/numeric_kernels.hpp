// numeric_kernels.hpp -- NumericToString (reference: src/numeric_to_string.cpp:18-92): std::to_string for the integer types,
// `ostream << x` (glibc's %g, precision 6, "C" locale) for f32 / f64, "true" / "false" for boolean.
//
// count (a lane per element: the text's length) -> scan (scan_kernels.hpp: begins / ends) -> write (a lane formats its element
// again, straight into the wave's LDS stretch; the wave stores the stretch with aligned dword stores).  One formatter serves both
// passes: it puts its bytes into a `Text` that either drops them (count) or is the lane's place in LDS (write), so the two passes
// cannot disagree about a length.
//
// %g with precision 6 needs the six significant decimal digits of the EXACT binary value, rounded half to even, and the choice
// between fixed and exponent form is made after that rounding.  value = m * 2^e (m normalised to 64 bits).  With X the decimal
// exponent (estimated from the binary one, corrected when the digits show it was one off) the digits are round(m * 2^e * 10^p),
// p = 5 - X.  10^p comes from a table of 128-bit approximations t * 2^te <= 10^p < (t + 1) * 2^te (numeric_table.hpp): the
// 192-bit product P = m * t is at most 2^64 below the true product, i.e. less than one unit of its middle limb.  The integer part
// and the fraction sit in the top limb and the middle limb; the rounding is decided unless the fraction lies within that unit of
// one half.  For 0 <= p <= 55 the table entry is exact and so is P: ties are seen directly.  What is left -- an inexact entry
// and a fraction in the band, which is where every true tie with p < 0 lands (1234565 -> 123456.5) -- goes to num_exact_cmp():
// the comparison of m * 2^e * 10^p with N + 1/2 in exact big-integer arithmetic on 32-bit limbs (5^330 * 2^64 has 831 bits).
// OVTK_NUM2STR_EXACT=1 (api_numeric.cpp) sends every finite non-zero element there; the result is the same.
#pragma once

#include "device_common.hpp"
#include "numeric_table.hpp"
#include "scan_kernels.hpp"

namespace ovtk {

using nu64 = unsigned long long;

constexpr int kNumMaxText = 20;                                            // "-9223372036854775808", "18446744073709551615"
constexpr int kNumStageWords = (kWave * kNumMaxText + 3 + 3) / 4 + 1;      // a wave's stretch, shifted by the output's misalignment

__device__ __forceinline__ nu64 num_mulhi(nu64 a, nu64 b) {
#ifdef OVTK_SIMT_EMULATOR
    return nu64((static_cast<unsigned __int128>(a) * b) >> 64);
#else
    return __umul64hi(a, b);
#endif
}

// Where a formatter's bytes go.
struct NumNoText {
    __device__ __forceinline__ void put(int, uint32_t) const {}
};
struct NumLdsText {
    uint8_t* at;
    __device__ __forceinline__ void put(int k, uint32_t c) const { at[k] = uint8_t(c); }
};

// ------------------------------------------------------------------------------------------------ integers
__device__ __forceinline__ int num_digits32(uint32_t v) {
    static constexpr uint32_t kPow[10] = {1u, 10u, 100u, 1000u, 10000u, 100000u, 1000000u, 10000000u, 100000000u, 1000000000u};
    const int t = ((32 - __clz(v | 1u)) * 1233) >> 12;   // floor(bit length * log10(2)): the digit count or one less
    return t + ((v | 1u) >= kPow[t] ? 1 : 0);   // (| 1: zero has one digit; no power of ten above 1 is odd)
}
__device__ __forceinline__ int num_digits64(nu64 v) {
    static constexpr nu64 kPow[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull,
                                      10000000000ull, 100000000000ull, 1000000000000ull, 10000000000000ull, 100000000000000ull,
                                      1000000000000000ull, 10000000000000000ull, 100000000000000000ull, 1000000000000000000ull,
                                      10000000000000000000ull};
    const int t = ((64 - __clzll(v | 1ull)) * 1233) >> 12;
    return t + ((v | 1ull) >= kPow[t] ? 1 : 0);
}
// `take` digits of chunk, least significant first, ending in front of `pos`; two per division by 100 (a multiply-shift: 32 bits)
template <class Text>
__device__ __forceinline__ int num_put_chunk(uint32_t chunk, int take, int pos, Text& out) {
    for (int j = 0; j < take; j += 2) {
        const uint32_t q = chunk / 100u, r = chunk - q * 100u, tens = (r * 205u) >> 11;   // r / 10 for r < 100
        chunk = q;
        out.put(--pos, '0' + (r - tens * 10u));
        if (j + 1 < take) out.put(--pos, '0' + tens);
    }
    return pos;
}
template <class Text>
__device__ __forceinline__ int num_put_u32(bool neg, uint32_t v, Text& out) {
    const int nd = num_digits32(v), len = (neg ? 1 : 0) + nd;
    if (neg) out.put(0, '-');
    int pos = len;
    if (nd > 8) {
        const uint32_t q = v / 100000000u;
        pos = num_put_chunk(v - q * 100000000u, 8, pos, out);
        v = q;
    }
    num_put_chunk(v, nd > 8 ? nd - 8 : nd, pos, out);
    return len;
}
// v / 10^8 as a multiply-shift: ceil(2^90 / 10^8) = 0xABCC77118461CEFD, whose excess over 2^90 / 10^8 times 2^64 stays below 2^90
__device__ __forceinline__ nu64 num_div1e8(nu64 v) { return num_mulhi(v, 0xABCC77118461CEFDull) >> 26; }
template <class Text>
__device__ __forceinline__ int num_put_u64(bool neg, nu64 v, Text& out) {
    if (!(v >> 32)) return num_put_u32(neg, uint32_t(v), out);
    const int nd = num_digits64(v), len = (neg ? 1 : 0) + nd;   // 10..20 digits
    if (neg) out.put(0, '-');
    int pos = len, left = nd;
    nu64 q = num_div1e8(v);
    pos = num_put_chunk(uint32_t(v - q * 100000000ull), 8, pos, out);
    left -= 8;
    if (left > 8) {
        const nu64 q2 = num_div1e8(q);
        pos = num_put_chunk(uint32_t(q - q2 * 100000000ull), 8, pos, out);
        left -= 8;
        q = q2;
    }
    num_put_chunk(uint32_t(q), left, pos, out);
    return len;
}

// ------------------------------------------------------------------------------------------------ floats
// sign(a * 5^k - s * 2^shift), a and s non-zero, 0 <= k <= 331: exact.
static __device__ __attribute__((noinline)) int num_exact_cmp(nu64 a, int k, nu64 s, int shift) {
    static constexpr uint32_t kPow5[14] = {1u, 5u, 25u, 125u, 625u, 3125u, 15625u, 78125u, 390625u, 1953125u, 9765625u, 48828125u, 244140625u, 1220703125u};
    constexpr int kLimbs = 28;   // 64 + 769 bits and a carry
    uint32_t w[kLimbs];
    int n = 2;
    w[0] = uint32_t(a);
    w[1] = uint32_t(a >> 32);
    while (k > 0) {
        const int step = k < 13 ? k : 13;
        const uint32_t mul = kPow5[step];
        nu64 carry = 0;
        for (int i = 0; i < n; ++i) {
            const nu64 t = nu64(w[i]) * mul + carry;
            w[i] = uint32_t(t);
            carry = t >> 32;
        }
        if (carry && n < kLimbs) w[n++] = uint32_t(carry);
        k -= step;
    }
    while (n > 1 && w[n - 1] == 0) --n;
    const int bits_big = 32 * (n - 1) + (32 - __clz(w[n - 1]));
    const int bits_s = 64 - __clzll(s) + shift;
    if (bits_big != bits_s) return bits_big > bits_s ? 1 : -1;
    // the same bit length: the top 64 bits of each, left-aligned; below them s * 2^shift has zeros only
    nu64 top;
    bool rest = false;
    if (bits_big <= 64) {
        top = (nu64(w[0]) | (n > 1 ? nu64(w[1]) << 32 : 0ull)) << (64 - bits_big);
    } else {
        const int from = bits_big - 64, i = from >> 5, r = from & 31;
        const nu64 lo = nu64(w[i]) | (nu64(w[i + 1]) << 32);
        const nu64 hi = (r && i + 2 < n) ? w[i + 2] : 0u;
        top = r ? (lo >> r) | (hi << (64 - r)) : lo;
        for (int j = 0; j < i; ++j) rest = rest || w[j] != 0;
        if (r) rest = rest || (w[i] & ((1u << r) - 1u)) != 0;
    }
    const nu64 top_s = s << __clzll(s);
    if (top != top_s) return top > top_s ? 1 : -1;
    return rest ? 1 : 0;
}

struct NumDec6 {
    uint32_t digits;   // 100000 .. 999999
    int exp10;         // the value rounds to digits * 10^(exp10 - 5)
};
// m * 2^e (m != 0) -> its six significant digits, round half to even on the exact value.
__device__ __forceinline__ NumDec6 num_round6(nu64 m, int e, const NumPow10* tab, bool force_exact) {
    const int lz = __clzll(m);
    const nu64 m64 = m << lz;
    const int e2 = e - lz;
    int x = ((e2 + 63) * 78913) >> 18;   // floor(floor(log2 v) * log10(2)) (exact for |.| <= 1650): floor(log10 v) or one less
    uint32_t n6 = 0;
    for (int round = 0; round < 2; ++round) {   // (two where the estimate was one short)
        const int p = 5 - x;
        const NumPow10 t = tab[p - kNumPow10Min];
        // P = m64 * t, 192 bits: p2:p1:p0
        const nu64 p0 = m64 * t.lo, ll_hi = num_mulhi(m64, t.lo);
        const nu64 hh_lo = m64 * t.hi, hh_hi = num_mulhi(m64, t.hi);
        const nu64 p1 = ll_hi + hh_lo, p2 = hh_hi + (p1 < ll_hi ? 1ull : 0ull);
        const int sh = -(e2 + num_pow10_exp(p)) - 128;   // 39..49: the binary point inside p2
        n6 = uint32_t(p2 >> sh);
        // The estimate is never above floor(log10 v) (10^x <= 2^floor(log2 v) <= v), and P is a lower bound: n6 >= 10^6 proves that
        // x is one short.  n6 = 99999 happens too: v an exact power of ten under a truncated entry, P just below 100000 -- the
        // fraction is all ones there and the rounding below makes it 100000.
        if (n6 >= 1000000u) {
            ++x;
            continue;
        }
        const nu64 frac = p2 & ((1ull << sh) - 1ull), half = 1ull << (sh - 1);
        int up;   // 0 down, 1 up, 2 a tie
        bool decided = true;
        if (p >= 0 && p <= kNumPow10ExactMax) up = frac > half || (frac == half && (p1 | p0)) ? 1 : (frac == half ? 2 : 0);
        else if (frac >= half) up = 1;      // the true product is above P
        else if (frac == half - 1 && p1 == ~0ull) decided = false, up = 0;   // ... by less than one unit of p1
        else up = 0;
        if (!decided || force_exact) {
            // v * 10^p against n6 + 1/2  <=>  m64 * 2^(e2 + 1) * 10^p against s = 2 * n6 + 1
            const nu64 s = 2ull * n6 + 1ull;
            const int c = p >= 0 ? num_exact_cmp(m64, p, s, -(e2 + p + 1)) : -num_exact_cmp(s, -p, m64, e2 + 1 + p);
            up = c > 0 ? 1 : (c == 0 ? 2 : 0);
        }
        if (up == 2) up = int(n6 & 1u);
        n6 += uint32_t(up);
        if (n6 == 1000000u) {
            n6 = 100000u;
            ++x;
        }
        break;
    }
    return NumDec6{n6, x};
}

template <class Text>
__device__ __forceinline__ int num_put_word(bool neg, uint32_t a, uint32_t b, uint32_t c, Text& out) {   // "inf", "nan" behind an optional '-'
    int pos = 0;
    if (neg) out.put(pos++, '-');
    out.put(pos++, a);
    out.put(pos++, b);
    out.put(pos++, c);
    return pos;
}
// The text of (-1)^neg * m * 2^e, m != 0: printf("%g").
template <class Text>
__device__ __forceinline__ int num_put_finite(bool neg, nu64 m, int e, const NumPow10* tab, bool force_exact, Text& out) {
    const NumDec6 d = num_round6(m, e, tab, force_exact);
    // byte k of asc: the ASCII digit k (0 the most significant); nsig: the digits left without the trailing zeros
    nu64 asc = 0;
    int zeros = 0;
    bool seen = false;
    uint32_t t = d.digits;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const uint32_t q = t / 10u, r = t - q * 10u;
        t = q;
        asc = (asc << 8) | ('0' + r);
        if (!seen && r == 0) ++zeros;
        else seen = true;
    }
    const int nsig = 6 - zeros, x = d.exp10;
    int pos = 0;
    if (neg) out.put(pos++, '-');
    if (x >= -4 && x < 6) {
        int k = 0;
        if (x >= 0) {
            for (; k <= x; ++k) out.put(pos++, uint32_t(asc >> (8 * k)) & 0xFFu);
        } else {
            out.put(pos++, '0');
        }
        if (nsig > k) {
            out.put(pos++, '.');
            for (int z = x + 1; z < 0; ++z) out.put(pos++, '0');
            for (; k < nsig; ++k) out.put(pos++, uint32_t(asc >> (8 * k)) & 0xFFu);
        }
    } else {
        out.put(pos++, uint32_t(asc) & 0xFFu);
        if (nsig > 1) {
            out.put(pos++, '.');
            for (int k = 1; k < nsig; ++k) out.put(pos++, uint32_t(asc >> (8 * k)) & 0xFFu);
        }
        out.put(pos++, 'e');
        out.put(pos++, x < 0 ? '-' : '+');
        const uint32_t a = uint32_t(x < 0 ? -x : x), h = a / 100u, r = a - h * 100u, tens = (r * 205u) >> 11;
        if (h) out.put(pos++, '0' + h);
        out.put(pos++, '0' + tens);
        out.put(pos++, '0' + (r - tens * 10u));
    }
    return pos;
}
template <class Text>
__device__ __forceinline__ int num_put_f64(nu64 bits, const NumPow10* tab, bool force_exact, Text& out) {
    const bool neg = (bits >> 63) != 0;
    const int ex = int(bits >> 52) & 0x7FF;
    const nu64 frac = bits & ((1ull << 52) - 1ull);
    if (ex == 0x7FF) return frac ? num_put_word(neg, 'n', 'a', 'n', out) : num_put_word(neg, 'i', 'n', 'f', out);
    if (ex == 0 && frac == 0) {
        if (neg) out.put(0, '-');
        out.put(neg ? 1 : 0, '0');
        return neg ? 2 : 1;
    }
    return ex ? num_put_finite(neg, frac | (1ull << 52), ex - 1075, tab, force_exact, out) : num_put_finite(neg, frac, -1074, tab, force_exact, out);
}
// f32: the float widened to double, exactly -- done on the bits, so that no float mode (denormal flushing) has a say
template <class Text>
__device__ __forceinline__ int num_put_f32(uint32_t bits, const NumPow10* tab, bool force_exact, Text& out) {
    const bool neg = (bits >> 31) != 0;
    const int ex = int(bits >> 23) & 0xFF;
    const uint32_t frac = bits & 0x7FFFFFu;
    if (ex == 0xFF) return frac ? num_put_word(neg, 'n', 'a', 'n', out) : num_put_word(neg, 'i', 'n', 'f', out);
    if (ex == 0 && frac == 0) {
        if (neg) out.put(0, '-');
        out.put(neg ? 1 : 0, '0');
        return neg ? 2 : 1;
    }
    return ex ? num_put_finite(neg, nu64(frac | 0x800000u), ex - 150, tab, force_exact, out) : num_put_finite(neg, nu64(frac), -149, tab, force_exact, out);
}

// ------------------------------------------------------------------------------------------------ the element types
// (the values of OVTK_NUM_* in include/ovtk_amd.h)
enum : int { kNumI8 = 0, kNumI16, kNumI32, kNumI64, kNumU8, kNumU16, kNumU32, kNumU64, kNumF32, kNumF64, kNumBool, kNumTypes };

struct NumIn {
    const void* data;
    long long n;
    const NumPow10* tab;   // (floats)
    int force_exact;       // (floats) OVTK_NUM2STR_EXACT
};

template <class Text>
__device__ __forceinline__ int num_put_i32(int32_t v, Text& out) {
    return num_put_u32(v < 0, v < 0 ? 0u - uint32_t(v) : uint32_t(v), out);
}
template <int DT, class Text>
__device__ __forceinline__ int num_format(const NumIn& in, long long i, Text& out) {
    if (DT == kNumI8) return num_put_i32(static_cast<const int8_t*>(in.data)[i], out);
    if (DT == kNumI16) return num_put_i32(static_cast<const int16_t*>(in.data)[i], out);
    if (DT == kNumI32) return num_put_i32(static_cast<const int32_t*>(in.data)[i], out);
    if (DT == kNumI64) {
        const long long v = static_cast<const long long*>(in.data)[i];
        return num_put_u64(v < 0, v < 0 ? 0ull - nu64(v) : nu64(v), out);
    }
    if (DT == kNumU8) return num_put_u32(false, static_cast<const uint8_t*>(in.data)[i], out);
    if (DT == kNumU16) return num_put_u32(false, static_cast<const uint16_t*>(in.data)[i], out);
    if (DT == kNumU32) return num_put_u32(false, static_cast<const uint32_t*>(in.data)[i], out);
    if (DT == kNumU64) return num_put_u64(false, static_cast<const nu64*>(in.data)[i], out);
    if (DT == kNumF32) return num_put_f32(static_cast<const uint32_t*>(in.data)[i], in.tab, in.force_exact != 0, out);
    if (DT == kNumF64) return num_put_f64(static_cast<const nu64*>(in.data)[i], in.tab, in.force_exact != 0, out);
    // boolean: numeric_to_string.cpp:75
    const bool v = static_cast<const uint8_t*>(in.data)[i] != 0;
    const uint32_t word = v ? 0x65757274u : 0x736C6166u;   // "true" / "fals", little-endian
#pragma unroll
    for (int k = 0; k < 4; ++k) out.put(k, (word >> (8 * k)) & 0xFFu);
    if (!v) out.put(4, 'e');
    return v ? 4 : 5;
}

// ------------------------------------------------------------------------------------------------ the passes
template <int DT>
static __global__ __launch_bounds__(kBlockThreads) void num_count_kernel(NumIn in, uint8_t* lens) {
    const long long i = (long long)blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= in.n) return;
    NumNoText none;
    lens[i] = uint8_t(num_format<DT>(in, i, none));
}
struct NumLen {
    const uint8_t* lens;
    __device__ long long operator()(long long i) const { return lens[i]; }
};
struct NumOffsets {
    int32_t* begins;
    int32_t* ends;
    __device__ void operator()(long long i, long long off, long long len) const {
        begins[i] = int32_t(off);
        ends[i] = int32_t(off + len);
    }
};
struct NumFin {
    RunStatus* status;
    long long cap;
    __device__ void operator()(long long total) const {
        status->n_out = total >= INT32_MAX ? INT32_MAX : int32_t(total);
        if (total >= INT32_MAX) atomicOr(&status->flags, kFlagTooLong);
        else if (total > cap) atomicOr(&status->flags, kFlagOutCapacity);
    }
};
// A wave owns 64 consecutive elements: their texts are one stretch of the output, begins[first] .. ends[last].  Every lane formats
// its element into LDS at its place in the stretch -- shifted by the stretch's misalignment in memory, so that LDS dword d IS the
// aligned dword d of the output -- and the wave stores whole dwords, 256 contiguous bytes per instruction; the two ragged ends go
// out as bytes.  (64 lanes each walking their own 1..20 bytes would be 64 scattered byte stores per step.)
template <int DT>
static __global__ __launch_bounds__(kBlockThreads) void num_write_kernel(NumIn in, const int32_t* begins, uint8_t* out, const RunStatus* status,
                                                                       uint32_t skip_flags) {
    __shared__ uint32_t stage[kWavesPerBlock][kNumStageWords];
    if (status->flags & skip_flags) return;
    const long long i = (long long)blockIdx.x * kBlockThreads + threadIdx.x;
    const long long first = i - lane_id();
    if (first >= in.n) return;   // (the whole wave)
    const int base = begins[first];
    const int mis = int((reinterpret_cast<uintptr_t>(out) + size_t(base)) & 3u);
    uint32_t* words = stage[wave_in_block()];
    int rel = 0, len = 0;
    if (i < in.n) {
        rel = begins[i] - base;
        if (rel >= 0 && rel <= (kWave - 1) * kNumMaxText) {   // (always: 63 texts of at most 20 bytes in front of this one)
            NumLdsText text{reinterpret_cast<uint8_t*>(words) + mis + rel};
            len = num_format<DT>(in, i, text);
        }
    }
    const int last = int(in.n - first < kWave ? in.n - first : kWave) - 1;
    const int span = mis + __shfl(rel + len, last);
    wave_sync();
    uint8_t* g = out + base - mis;   // 4-byte aligned; bytes in front of `mis` and from `span` on are not this wave's
    for (int d = lane_id(); d * 4 < span; d += kWave) {
        const uint32_t w = words[d];
        const int lo = d * 4;
        if (lo >= mis && lo + 4 <= span) {
            *reinterpret_cast<uint32_t*>(g + lo) = w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (lo + k >= mis && lo + k < span) g[lo + k] = uint8_t(w >> (8 * k));
        }
    }
}

}  // namespace ovtk
