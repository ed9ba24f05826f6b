// charsmap_kernels.hpp -- CharsMapNormalization, NormalizeUnicode and CaseFold (src/charsmap_normalization.cpp:34-69,
// src/normalize_unicode.cpp:32-62, src/case_fold.cpp:34-73): sentencepiece's normalizer::Normalizer::Normalize over a precompiled
// charsmap, per string, inside evaluate_normalization_helper (src/utils.cpp:178-234).
//
// What the reference does per string (restated in tests/charsmap_ref.py):
//   * at each byte position the charsmap's Darts double array is walked as commonPrefixSearch walks it; of the first 32 keys that end on
//     the way the longest wins: its replacement string is emitted and its bytes are consumed.  No key: one well-formed UTF-8 character
//     (right trail bytes, not overlong, no surrogate, at most U+10FFFF, not cut off by the string's end) is emitted as it stands, anything
//     else is EF BF BD for ONE byte;
//   * while the prefix before ended in a space (initially: remove_extra_whitespaces) the leading spaces of what a prefix emits are
//     dropped; "ended in a space" changes only with a non-empty rest and is cleared after every prefix without remove_extra_whitespaces;
//     0x20 becomes E2 96 81 under escape_whitespaces; add_dummy_prefix puts one space symbol in front;
//   * with remove_extra_whitespaces the space symbol is stripped from the end of the output for as long as it is there -- under
//     escape_whitespaces that eats a literal U+2581 of the input too (kept).  The reference's skipping of leading " " prefixes changes
//     nothing these rules do not already give: a row that emits nothing but its dummy prefix loses that to the strip.
//
// The only dependency along a string is which positions are prefix starts (p -> p + consumed[p]) and one bit, "ended in a space".
//   * A wave per string, 64 bytes at a time, a lane per byte: every lane decodes its position as if it were a start -- a 256-bit table
//     of the bytes some key starts with (kernel argument) keeps ASCII and most other text out of the trie; the rest walks the double
//     array (~180 KB, L2).  A replacement's length, leading / trailing spaces and space count come from one 8-byte record per
//     replacement built at create.
//   * The starts of a tile without a key match are mask algebra: everything from the tile's entry point on that no well-formed
//     character covers.  A tile with a match is walked by the wave, one readlane per prefix.
//   * "Ended in a space" per start: a prefix sets it, clears it or leaves it (empty replacement) -- the last lane below that sets or
//     clears decides, two ballots.  The trailing strip is a run length carried along the row: space symbols at the end of the output.
//   * count (a wave per row) -> scan over the rows -> write (the same walk again, bytes stored, cut at the row's final length).
//     Rows with skips[i] != 0 are copied.  A row longer than a few KB is still one wave's work: not split here.
#pragma once

#include "device_common.hpp"
#include "ops_kernels.hpp"

namespace ovtk {

constexpr int kCmMaxResults = 32;          // sentencepiece's kMaxTrieResultsSize: matches looked at per position
constexpr int kCmMaxRepBytes = 1023;       // a replacement's length, leading spaces and space count take 10 bits each
constexpr uint32_t kCmRepCopy = 0xFFFFFFFFu;   // a prefix emits the character it consumed
constexpr uint32_t kCmRepBad = 0xFFFFFFFEu;    // ... or U+FFFD for one byte

// m0 of a replacement's record: length | leading spaces << 10 | spaces << 20 | ends in a space << 30 | nothing but space symbols << 31;
// m1: space symbols at its end (0x20, and E2 96 81 under escape_whitespaces)
__host__ __device__ __forceinline__ uint32_t cm_pack(uint32_t len, uint32_t ls, uint32_t ns, bool ends, bool all_units) {
    return len | (ls << 10) | (ns << 20) | (ends ? 1u << 30 : 0u) | (all_units ? 1u << 31 : 0u);
}

struct CharsmapDev {
    const uint32_t* units;      // nullptr: an empty blob, no trie
    uint32_t n_units;
    const uint8_t* strings;     // the replacement strings
    const uint2* meta;          // [n_strings] the record of the replacement that starts at this byte (filled for the ones keys map to)
    uint32_t n_strings;
    unsigned long long first[4];   // bit c: some key starts with byte c
    int add_dummy, remove_extra, escape;
};

__device__ __forceinline__ uint32_t cm_offset(uint32_t u) { return (u >> 10) << ((u & 0x200u) >> 6); }

// The longest of the first kCmMaxResults keys that are prefixes of s[0, avail): its length (0: none) and its value.  Every index is
// checked against the array: a blob that create let through cannot send a lane outside it either.
__device__ __forceinline__ int cm_match(const CharsmapDev& d, const uint8_t* s, int avail, uint32_t& value) {
    uint32_t pos = cm_offset(d.units[0]);
    int best = 0, found = 0;
    for (int k = 0; k < avail; ++k) {
        const uint32_t c = s[k];
        pos ^= c;
        if (pos >= d.n_units) break;
        const uint32_t u = d.units[pos];
        if ((u & 0x800000FFu) != c) break;
        pos ^= cm_offset(u);
        if (pos >= d.n_units) break;
        if ((u >> 8) & 1u) {
            if (found < kCmMaxResults) {
                best = k + 1;
                value = d.units[pos] & 0x7FFFFFFFu;
            }
            ++found;
        }
    }
    return best;
}

// Bytes of the well-formed UTF-8 character in the low bytes of w (bytes behind the string's end are 0: no trail bytes), 0: none.
__device__ __forceinline__ int cm_utf8_len(uint32_t w) {
    const uint32_t c0 = w & 0xFF, c1 = (w >> 8) & 0xFF, c2 = (w >> 16) & 0xFF, c3 = w >> 24;
    if (c0 < 0x80) return 1;
    const bool t1 = (c1 & 0xC0) == 0x80, t2 = (c2 & 0xC0) == 0x80, t3 = (c3 & 0xC0) == 0x80;
    if (c0 >= 0xC2 && c0 <= 0xDF) return t1 ? 2 : 0;
    if (c0 >= 0xE0 && c0 <= 0xEF) return (t1 && t2 && !(c0 == 0xE0 && c1 < 0xA0) && !(c0 == 0xED && c1 >= 0xA0)) ? 3 : 0;
    if (c0 >= 0xF0 && c0 <= 0xF4) return (t1 && t2 && t3 && !(c0 == 0xF0 && c1 < 0x90) && !(c0 == 0xF4 && c1 >= 0x90)) ? 4 : 0;
    return 0;
}

struct __attribute__((packed, aligned(1))) CmBytes4 { uint32_t d; };

// each_wave_kernel: a row.  WRITE = false: its final length to lens[i]; WRITE = true (behind the scan): its bytes to out_chars +
// out_begins[i], cut at lens[i].
template <bool WRITE>
struct CmRow {
    CharsmapDev d;
    const int32_t* begins;
    const int32_t* ends;
    const uint8_t* chars;
    long long n_chars;
    const uint8_t* skips;   // or nullptr
    int32_t* lens;
    const int32_t* out_begins;
    uint8_t* out_chars;

    __device__ void operator()(long long i) const {
        const long long b = begins[i], e = ends[i];
        const int l = lane_id();
        if (b < 0 || e < b || e > n_chars) {   // (flagged by check_strings_kernel)
            if (!WRITE && l == 0) lens[i] = 0;
            return;
        }
        const int n = int(e - b);
        const uint8_t* text = chars + b;
        uint8_t* dst = WRITE ? out_chars + out_begins[i] : nullptr;
        if (skips && skips[i]) {
            if (WRITE) wave_copy_bytes(text, dst, n);
            else if (l == 0) lens[i] = n;
            return;
        }
        const long long limit = WRITE ? lens[i] : 0;
        const int unit = d.escape ? 3 : 1;
        long long total = 0;    // bytes emitted so far, before the strip
        int run = 0;            // space symbols at the end of them
        if (n > 0 && d.add_dummy) {
            if (WRITE && l < unit && l < limit) dst[l] = d.escape ? (l == 0 ? 0xE2 : l == 1 ? 0x96 : 0x81) : 0x20;
            total = unit;
            run = 1;
        }
        int state = d.remove_extra ? 1 : 0;   // the prefix before ended in a space
        int entry = 0;                        // the first start of the tile at hand
        for (int t0 = 0; t0 < n; t0 += kWave) {
            if (entry >= kWave) {   // (a key longer than a tile)
                entry -= kWave;
                continue;
            }
            const int p = t0 + l;
            const bool in = p < n;
            uint32_t w = 0;
            if (p + 4 <= n) w = reinterpret_cast<const CmBytes4*>(text + p)->d;
            else
                for (int k = 0; p + k < n; ++k) w |= uint32_t(text[p + k]) << (8 * k);
            const uint32_t c0 = w & 0xFF;
            int cons = 1;
            uint32_t rep = kCmRepBad, m0 = cm_pack(3, 0, 0, false, false), m1 = 0;
            bool matched = false;
            if (in) {
                int mlen = 0;
                uint32_t value = 0;
                const unsigned long long fm = c0 < 128 ? (c0 < 64 ? d.first[0] : d.first[1]) : (c0 < 192 ? d.first[2] : d.first[3]);
                if (d.units && ((fm >> (c0 & 63)) & 1ull)) mlen = cm_match(d, text + p, n - p, value);
                if (mlen) {
                    matched = true;
                    cons = mlen;
                    rep = value;
                    const uint2 m = value < d.n_strings ? d.meta[value] : uint2{cm_pack(0, 0, 0, false, true), 0};
                    m0 = m.x;
                    m1 = m.y;
                } else if (const int clen = cm_utf8_len(w)) {
                    cons = clen;
                    rep = kCmRepCopy;
                    const bool space = c0 == 0x20, symbol = d.escape && (w & 0xFFFFFFu) == 0x8196E2u;
                    m0 = cm_pack(uint32_t(clen), space, space, space, space || symbol);
                    m1 = (space || symbol) ? 1 : 0;
                }
            }
            // the starts: from `entry` on, p -> p + cons[p]
            const unsigned long long ge = __ballot(in && l >= entry);
            unsigned long long vis = 0;
            int exit = entry;
            if (__ballot(matched) == 0) {
                const bool copy = in && l >= entry && rep == kCmRepCopy;
                const unsigned long long v2 = __ballot(copy && cons == 2), v3 = __ballot(copy && cons == 3), v4 = __ballot(copy && cons == 4);
                vis = ge & ~(((v2 | v3 | v4) << 1) | ((v3 | v4) << 2) | (v4 << 3));
                if (vis) {
                    const int last = 63 - __clzll(vis);
                    exit = last + wave_readlane(cons, last);
                }
            } else {
                while (exit < kWave && t0 + exit < n) {
                    vis |= 1ull << exit;
                    exit += wave_readlane(cons, exit);
                }
            }
            entry = exit > kWave ? exit - kWave : 0;
            const bool visited = (vis >> l) & 1ull;
            const int len = int(m0 & 1023u), ls = int((m0 >> 10) & 1023u), ns = int((m0 >> 20) & 1023u);
            const bool ends_sp = (m0 >> 30) & 1u, all_units = (m0 >> 31) & 1u;
            int st = 0;
            if (d.remove_extra) {
                const unsigned long long c1 = __ballot(visited && len > 0 && ends_sp), c0s = __ballot(visited && len > 0 && !ends_sp);
                const unsigned long long below = (c1 | c0s) & lanemask_lt();
                st = below ? int((c1 >> (63 - __clzll(below))) & 1ull) : state;
                if (c1 | c0s) state = int((c1 >> (63 - __clzll(c1 | c0s))) & 1ull);
            }
            const int drop = st ? ls : 0, kept = len - drop;
            const int bytes = visited ? kept + (d.escape ? 2 * (ns - drop) : 0) : 0;
            const int incl = wave_incl_sum(bytes);
            if (!WRITE && d.remove_extra) {
                // the run of space symbols at the end: a prefix whose rest is nothing but symbols adds them, any other non-empty rest
                // starts the run again with the symbols at its own end
                const unsigned long long resets = __ballot(visited && kept > 0 && !all_units);
                const int top = resets ? 63 - __clzll(resets) : -1;
                const int add = wave_sum(visited && all_units && l > top ? int(m1) - drop : 0);
                run = (resets ? wave_readlane(int(m1), top) : run) + add;
            }
            if (WRITE && bytes > 0) {
                long long o = total + incl - bytes;
                auto put = [&](uint32_t c) {
                    if (d.escape && c == 0x20) {
                        if (o < limit) dst[o] = 0xE2;
                        if (o + 1 < limit) dst[o + 1] = 0x96;
                        if (o + 2 < limit) dst[o + 2] = 0x81;
                        o += 3;
                    } else {
                        if (o < limit) dst[o] = uint8_t(c);
                        ++o;
                    }
                };
                if (rep == kCmRepCopy) {
                    for (int k = 0; k < kept; ++k) put((w >> (8 * k)) & 0xFF);   // (kept is 0 for a dropped space, else the character)
                } else if (rep == kCmRepBad) {
                    put(0xEF);
                    put(0xBF);
                    put(0xBD);
                } else {
                    const uint8_t* src = d.strings + rep + drop;
                    for (int k = 0; k < kept; ++k) put(src[k]);
                }
            }
            total += wave_readlane(incl, kWave - 1);
        }
        if (!WRITE && l == 0) {
            const long long fin = total - (d.remove_extra ? (long long)run * unit : 0);
            lens[i] = fin > INT32_MAX ? INT32_MAX : int32_t(fin);
        }
    }
};

// CaseFold with encoding "" (src/case_fold.cpp:56-64, case_fold.hpp:21-23): bytes lo..hi shifted by delta, a wave per string.
struct CaseFoldLen {
    const int32_t* begins;
    const int32_t* ends;
    long long n_chars;
    __device__ long long operator()(long long i) const {
        const long long b = begins[i], e = ends[i];
        return (b < 0 || e < b || e > n_chars) ? 0 : e - b;   // flagged by check_strings_kernel
    }
};
struct CaseFoldWrite {
    const int32_t* begins;
    const int32_t* ends;
    const uint8_t* chars;
    const int32_t* out_begins;
    uint8_t* out_chars;
    uint32_t lo, hi;
    int delta;
    __device__ void operator()(long long i) const {
        const uint8_t* src = chars + begins[i];
        uint8_t* dst = out_chars + out_begins[i];
        const int n = ends[i] - begins[i];
        for (int k = lane_id(); k < n; k += kWave) {
            const uint32_t c = src[k];
            dst[k] = uint8_t(c >= lo && c <= hi ? int(c) + delta : int(c));
        }
    }
};

}  // namespace ovtk
