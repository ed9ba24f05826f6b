// regex_subst_kernels.hpp -- RegexNormalization (src/regex_normalization.cpp; PCRE2Wrapper::substitute, src/utils.cpp:315-382, per
// string inside evaluate_normalization_helper, :178-234): pcre2_substitute with the plan of regex_subst.hpp.
//
// count (the row's final length and whether it comes back unchanged: a wave per row on the class path, a lane per row on the general
// path) -> scan over the rows -> write (a wave per row: the same walk again, bytes stored), the shape of charsmap_kernels.hpp.  Two walks:
//   * the CLASS path -- every match is one character decided by its class alone (`\s`, `\p{Mn}`, `([\p{Han}])`, a literal, ...): no
//     position depends on another.  A lane per byte, 64 bytes a tile: the lane of a character's first byte classifies it through the
//     program's ASCII / two-level tables, ballots tell the character's other bytes that they belong to a match and which of them is
//     its last, a prefix sum over the wave and a running total along the row give every lane its place in the output.  Neighbouring
//     lanes store neighbouring bytes;
//   * the GENERAL path -- the count pass is a lane per row (each_kernel), every lane with a matcher of its own; in the write pass (a
//     wave per row) lane 0 runs the matcher (one program, or one per top-level alternative: leftmost start, lowest alternative
//     first) with pcre2_substitute's rule for empty matches: behind an empty match at p first a non-empty match anchored at p
//     (RegexProgram::start_nonempty), else one character is passed over.  The wave copies the text between the matches 16 bytes a lane
//     and emits the template's segments: literal bytes, and group spans [start + front characters, end - back characters).
// Per string, as the reference: a match of an alternative that leaves a referenced group unset gives the whole string back (PCRE2
// error -55), and so does a result that does not fit the reference's buffer, out_len + 1 > 4 * (len + rc * template_len) with rc =
// pcre2_match's return value for the first match.  Where unreferenced optional groups leave rc open between two values and the
// result falls between the two bounds, the call reports OVTK_E_UNSUPPORTED (kFlagSubstUndecided).
#pragma once

#include "device_common.hpp"
#include "ops_kernels.hpp"
#include "regex_device.hpp"

namespace ovtk {

struct __attribute__((packed, aligned(1))) SubstBytes4 { uint32_t d; };
constexpr uint32_t kFlagSubstUndecided = 256u;   // RunStatus::flags: the reference's buffer quirk depends on which optional groups were set

struct SubstAltDev {
    RegexDev R;
    uint16_t start_nonempty[kRegexMaxCtx];
    int32_t rc_min, rc_max, has_unset, seg_first;   // seg_first: the alternative's first entry in SubstDev::segs
};
struct SubstSegDev {
    int32_t kind, a, b;   // SubstSeg
};
struct SubstDev {
    const SubstAltDev* alts;
    int32_t n_alts;
    const SubstSegDev* segs;
    int32_t n_segs;             // per alternative
    const uint8_t* lits;
    int32_t global, all_anchored, tmpl_len, identity;
    int32_t class_path, class_has_ref, pre_len, suf_len;
    const uint8_t* match_class; // [256]
    const uint8_t* class_lits;  // pre_len + suf_len bytes
};

// One attempt of alternative A at position p: the end of the match PCRE2 finds there, or false.
__device__ __forceinline__ bool subst_attempt(const SubstAltDev& A, bool nonempty, const uint8_t* s, int slen, int p, int& me, int& first_len) {
    const RegexDev& R = A.R;
    const RegexTables T{R.trans, R.ascii_class};
    const int ctx = regex_context(R, T, s, slen, p);
    me = regex_attempt(R, T, s, slen, p, nonempty ? A.start_nonempty[ctx] : R.start[ctx], first_len);
    return me >= 0;
}

// The match at or after `from` (anchored: at `from`, and not empty): leftmost start, at that start the first alternative.
__device__ __forceinline__ bool subst_next(const SubstDev& S, const uint8_t* s, int slen, int from, bool anchored_nonempty, int& mb, int& me, int& alt) {
    for (int p = from; p <= slen;) {
        int first_len = 1;
        for (int a = 0; a < S.n_alts; ++a)
            if (subst_attempt(S.alts[a], anchored_nonempty, s, slen, p, me, first_len)) {
                mb = p;
                alt = a;
                return true;
            }
        if (anchored_nonempty || p >= slen || S.all_anchored) break;   // (`^` / `\A` in front of every alternative: offset 0 or nowhere)
        p += first_len > 0 ? first_len : 1;
    }
    return false;
}

// The next match pcre2_substitute replaces, from (at, behind_empty) -- pcre2_substitute.c: behind an empty match the next attempt is
// PCRE2_NOTEMPTY_ATSTART | PCRE2_ANCHORED; when that fails one whole character is passed over and matching goes on as usual.
__device__ __forceinline__ bool subst_step(const SubstDev& S, const uint8_t* s, int slen, int& at, bool& behind_empty, int& mb, int& me, int& alt) {
    if (behind_empty) {
        if (subst_next(S, s, slen, at, true, mb, me, alt)) return true;
        if (at >= slen || S.all_anchored) return false;
        int len = 1;
        const RegexDev& R = S.alts[0].R;
        regex_symbol(R, RegexTables{R.trans, R.ascii_class}, s, slen, at, len);
        at += len > 0 ? len : 1;
        behind_empty = false;
    }
    return subst_next(S, s, slen, at, false, mb, me, alt);
}

// `chars` characters on from position i (not past hi).
__device__ __forceinline__ int subst_forward(const uint8_t* s, int i, int hi, int chars) {
    for (; chars > 0 && i < hi; --chars) {
        const uint32_t b = s[i];
        i += b < 0xC0u ? 1 : (b >= 0xF0u ? 4 : (b >= 0xE0u ? 3 : 2));
    }
    return i < hi ? i : hi;
}

// each_wave_kernel: a row.  WRITE = false: lens[i] = its final length, ident[i] = it comes back unchanged; WRITE = true (behind the
// scan): its bytes to out_chars + out_begins[i].  LANE (each_kernel, the general path's count pass): a LANE per row -- counting copies
// nothing, so every lane runs a matcher of its own, as regex_split_kernel's lanes do.
template <bool WRITE, bool LANE = false>
struct SubstRow {
    SubstDev S;
    const int32_t* begins;
    const int32_t* ends;
    const uint8_t* chars;
    long long n_chars;
    const uint8_t* skips;   // or nullptr
    int32_t* lens;
    uint8_t* ident;
    const int32_t* out_begins;
    uint8_t* out_chars;
    RunStatus* status;

    // count pass: the row's length and the two per-string identity quirks
    __device__ void file(long long i, int n, long long out, bool any, bool unset, int rc_min, int rc_max) const {
        bool same = unset;
        if (any && !same) {
            const long long lo = 4ll * (n + (long long)rc_min * S.tmpl_len), hi = 4ll * (n + (long long)rc_max * S.tmpl_len);
            if (out + 1 > hi) same = true;   // PCRE2_ERROR_NOMEMORY: the reference returns the input
            else if (out + 1 > lo) atomicOr(&status->flags, kFlagSubstUndecided);
        }
        lens[i] = same ? n : (out > INT32_MAX ? INT32_MAX : int32_t(out));
        ident[i] = same ? 1 : 0;
    }

    __device__ void operator()(long long i) const {
        const long long b = begins[i], e = ends[i];
        static_assert(!(WRITE && LANE), "the write pass copies with the whole wave");
        const int l = LANE ? 0 : lane_id();
        if (b < 0 || e < b || e > n_chars) {   // (flagged by check_strings_kernel)
            if (!WRITE && l == 0) {
                lens[i] = 0;
                ident[i] = 1;
            }
            return;
        }
        const int n = int(e - b);
        const uint8_t* text = chars + b;
        uint8_t* dst = WRITE ? out_chars + out_begins[i] : nullptr;
        if ((skips && skips[i]) || S.identity || (WRITE && ident[i])) {
            if (WRITE) wave_copy_bytes(text, dst, n);
            else if (l == 0) {
                lens[i] = n;
                ident[i] = 1;
            }
            return;
        }
        if (!LANE && S.class_path) class_row(i, text, n, dst);
        else general_row(i, text, n, dst);
    }

    __device__ void class_row(long long i, const uint8_t* text, int n, uint8_t* dst) const {
        const int l = lane_id();
        const SubstAltDev& A = S.alts[0];
        const RegexDev& R = A.R;
        long long total = 0;
        bool any = false;
        unsigned long long carry_mem = 0, carry_last = 0;   // bytes of a matched character that reach into this tile, and its last one
        for (int t0 = 0; t0 < n; t0 += kWave) {
            const int p = t0 + l;
            const bool in = p < n;
            uint32_t w = 0;
            if (p + 4 <= n) w = reinterpret_cast<const SubstBytes4*>(text + p)->d;
            else
                for (int k = 0; p + k < n; ++k) w |= uint32_t(text[p + k]) << (8 * k);
            const uint32_t b0 = w & 0xFFu;
            bool match = false;
            int clen = 1;
            if (in && (b0 & 0xC0u) != 0x80u) {   // the first byte of a character: regex_symbol(), on the four bytes in hand
                int cls;
                if (b0 < 0x80u) {
                    cls = R.ascii_class[b0];
                } else {
                    int nb = b0 >= 0xF0u ? 4 : (b0 >= 0xE0u ? 3 : 2);
                    if (p + nb > n) nb = n - p;
                    uint32_t cp = b0 & (0xFFu >> (nb + 1));
                    for (; clen < nb && ((w >> (8 * clen)) & 0xC0u) == 0x80u; ++clen) cp = (cp << 6) | ((w >> (8 * clen)) & 0x3Fu);
                    if (cp > 0x10FFFFu) cp = 0x10FFFFu;
                    cls = R.cp_blocks[uint32_t(R.cp_index[cp >> 7]) * 128u + (cp & 127u)];
                }
                match = S.match_class[cls] != 0;
            }
            const unsigned long long m1 = __ballot(match && clen == 1), m2 = __ballot(match && clen == 2), m3 = __ballot(match && clen == 3),
                                     m4 = __ballot(match && clen == 4);
            const unsigned long long ge2 = m2 | m3 | m4, ge3 = m3 | m4;
            const unsigned long long mem = m1 | ge2 | (ge2 << 1) | (ge3 << 2) | (m4 << 3) | carry_mem;
            const unsigned long long last = m1 | (m2 << 1) | (m3 << 2) | (m4 << 3) | carry_last;
            carry_mem = (ge2 >> 63) | (ge3 >> 62) | (m4 >> 61);
            carry_last = (m2 >> 63) | (m3 >> 62) | (m4 >> 61);
            any = any || (m1 | ge2) != 0;
            const bool is_mem = (mem >> l) & 1ull, is_last = (last >> l) & 1ull;
            const bool keep = in && (S.class_has_ref || !is_mem);   // the byte itself goes to the output
            const int bytes = (keep ? 1 : 0) + (match ? S.pre_len : 0) + (is_last ? S.suf_len : 0);
            const int incl = wave_incl_sum(bytes);
            if (WRITE && bytes > 0) {
                uint8_t* o = dst + total + incl - bytes;
                if (match)
                    for (int k = 0; k < S.pre_len; ++k) *o++ = S.class_lits[k];
                if (keep) *o++ = uint8_t(b0);
                if (is_last)
                    for (int k = 0; k < S.suf_len; ++k) *o++ = S.class_lits[S.pre_len + k];
            }
            total += wave_readlane(incl, kWave - 1);
        }
        if (!WRITE && l == 0) file(i, n, total, any, false, A.rc_min, A.rc_max);
    }

    __device__ void general_row(long long i, const uint8_t* text, int n, uint8_t* dst) const {
        const int l = LANE ? 0 : lane_id();
        int at = 0, pos = 0;          // lane 0: where matching goes on; all lanes: the text up to here is in the output
        bool behind_empty = false, any = false, unset = false;
        int rc_min = 1, rc_max = 1;
        long long out = 0;
        for (;;) {
            int found = 0, mb = 0, me = 0, alt = 0;
            if (l == 0) found = subst_step(S, text, n, at, behind_empty, mb, me, alt) ? 1 : 0;
            if (!LANE) found = wave_readlane(found, 0);
            if (!found) break;
            if (!LANE) {
                mb = wave_readlane(mb, 0);
                me = wave_readlane(me, 0);
                alt = wave_readlane(alt, 0);
            }
            const SubstAltDev& A = S.alts[alt];
            if (!any) {
                rc_min = A.rc_min;
                rc_max = A.rc_max;
            }
            any = true;
            if (A.has_unset) {   // PCRE2_ERROR_UNSET: the whole string comes back
                unset = true;
                break;
            }
            if (WRITE) wave_copy_bytes(text + pos, dst + out, mb - pos);
            out += mb - pos;
            for (int k = 0; k < S.n_segs; ++k) {
                const SubstSegDev g = S.segs[A.seg_first + k];
                const uint8_t* src = S.lits + g.a;
                int len = g.b;
                if (g.kind) {
                    const int gb = subst_forward(text, mb, me, g.a), ge = regex_step_back(text, gb, me, g.b);
                    src = text + gb;
                    len = ge - gb;
                }
                if (WRITE) wave_copy_bytes(src, dst + out, len);
                out += len;
            }
            pos = me;
            if (!S.global) break;
            at = me;
            behind_empty = me == mb;
        }
        if (unset) {
            if (!WRITE && l == 0) file(i, n, n, true, true, 1, 1);
            return;
        }
        if (WRITE) wave_copy_bytes(text + pos, dst + out, n - pos);
        out += n - pos;
        if (!WRITE && l == 0) file(i, n, out, any, false, rc_min, rc_max);
    }
};

}  // namespace ovtk
