// sp_special_kernels.hpp -- SentencepieceTokenizer's 8-input form (src/sentence_piece.cpp:200-230, :286-329): the added tokens are cut
// out of every row by a generated pattern, what lies between them is encoded part by part, and the tokens' ids stand between the parts.
//
// The pattern is the tokens in input order joined by `|`, each quoted; a token of ASCII letters only is `\bTOK|TOK\b`; PCRE2_UTF |
// PCRE2_UCP; searched from a cursor over the whole row (src/utils.cpp:396-420).  Without PCRE2 that is:
//   * the smallest position p >= cursor at which some token matches; among the tokens that match there the first in list order;
//   * a letters-only token matches at p iff its bytes stand there and (p == 0 or the character in front of p is no word character) or
//     (it ends the row or the character behind it is no word character); \w = L | N | Mn | Pc (PCRE2 10.46, regex_compile.cpp's
//     word_set(): the bit table is made from unicode_general_categories());
//   * whether a token matches at p does not depend on the cursor (\b sees the character in front of it), so the positions are tested
//     in parallel and only the walk from match to match is sequential.
// Malformed UTF-8 (the reference's pcre2_jit_match does not validate: undefined there) follows SpecialTokensSplit's convention
// (split_seq_device.hpp, seq_char): no match begins at a continuation byte; the character at a position is decoded leniently -- a
// lead byte takes the continuation bytes that follow it, as many as it asks for at most, a stray continuation byte is a character
// of its own and no word character; the character in front of p is the one whose lenient decoding ends at p, else the byte p - 1
// alone (no word character unless ASCII); a value beyond U+10FFFF is no word character.
//
//   * SpCut<false> (each_wave_kernel, a wave per row): a sweep of 1 024 bytes per step, 16 per lane, against the tokens' first bytes
//     (bytes16_in_list); a step without a candidate byte ends there.  Each lane tests its candidates (token_at + the boundary rule),
//     the wave then walks the hits in order.  Counts the row's slots: a part (text between two matches, not empty) or a token's id.
//   * scan over the slot counts -> SpCut<true> writes the slots: begins / ends of a part into the caller's chars (nothing is copied;
//     a token's slot is an empty part), slot_id = the token's id or -1.
//   * the slots are the sentences of the normalizer and the unigram / BPE passes (sentencepiece_kernels.hpp, sp_bpe_kernels.hpp) with
//     eos and reverse switched off: every part gets its dummy prefix and its bos by itself.
//   * SpRowLen: a row's ids = the sum over its slots (a part's count, or 1) + eos; the longest row.  scan -> SpAssemble, a wave per row:
//     the (row, position) pairs and the values, from the last position down for a reversed row.
#pragma once

#include "device_common.hpp"
#include "sentencepiece_kernels.hpp"
#include "split_seq_device.hpp"

namespace ovtk {

constexpr int kSpMaxSpecialTokens = 4096;      // tokens of one handle
constexpr int kSpMaxSpecialTokenBytes = 1023;  // bytes of one token
constexpr int kSpCutStep = 16 * kWave;         // bytes a wave sweeps per step
constexpr uint32_t kSpWordTableWords = 0x110000 / 32;

struct SpSpecialDev {
    SpecialDev lit;               // the literal matcher's view: tok_* (padded to 16 bytes), first / n_first; no groups
    const int32_t* tok_ids;       // [tokens]
    const uint8_t* tok_alpha;     // [tokens] 1: ASCII letters only (the \b rule)
    const int32_t* bucket_off;    // [257] tokens by first byte, list order kept inside a bucket:
    const int32_t* bucket_tok;    // [tokens]  bucket_tok[bucket_off[b] .. bucket_off[b + 1])
    const uint32_t* word_bits;    // [kSpWordTableWords] \w under UCP
};

__device__ __forceinline__ bool sp_is_word(const SpSpecialDev& T, uint32_t cp) {
    return cp < 0x110000u && ((T.word_bits[cp >> 5] >> (cp & 31u)) & 1u);
}
// the character at pos (pos < slen), decoded as seq_char decodes it
__device__ __forceinline__ uint32_t sp_char_at(const uint8_t* s, int pos, int slen, int& len) {
    const uint32_t b = s[pos];
    len = 1;
    if (b < 0x80u) return b;
    if (b < 0xC0u) return 0xFFFFFFFFu;   // a stray continuation byte
    int n = b >= 0xF0u ? 4 : (b >= 0xE0u ? 3 : 2);
    if (pos + n > slen) n = slen - pos;
    uint32_t cp = b & (0xFFu >> (n + 1));
    for (; len < n && (s[pos + len] & 0xC0u) == 0x80u; ++len) cp = (cp << 6) | (s[pos + len] & 0x3Fu);
    return cp;
}
__device__ __forceinline__ bool sp_word_at(const SpSpecialDev& T, const uint8_t* s, int pos, int slen) {
    int len;
    return sp_is_word(T, sp_char_at(s, pos, slen, len));
}
// the character in front of p (p > 0)
__device__ __forceinline__ bool sp_word_before(const SpSpecialDev& T, const uint8_t* s, int p, int slen) {
    int q = p - 1;
    if (s[q] < 0x80u) return sp_is_word(T, s[q]);
    while (q > 0 && p - q < 4 && (s[q] & 0xC0u) == 0x80u) --q;
    int len;
    const uint32_t cp = sp_char_at(s, q, slen, len);
    return q + len == p && sp_is_word(T, cp);   // (else: the byte p - 1 stands alone, and it is not ASCII)
}
// The first token in list order that matches at p: its length and id; 0: none.
__device__ __forceinline__ int sp_match_at(const SpSpecialDev& T, const uint8_t* s, int slen, int p, int32_t& id) {
    const uint32_t first = s[p];
    if ((first & 0xC0u) == 0x80u) return 0;
    const SpecialTabs tb = special_tabs(T.lit);
    for (int j = T.bucket_off[first], je = T.bucket_off[first + 1]; j < je; ++j) {
        const int t = T.bucket_tok[j];
        if (!token_at(T.lit, tb, t, s, slen, p)) continue;
        const int n = tb.tok_ends[t] - tb.tok_begins[t];
        if (T.tok_alpha[t]) {
            const bool free_front = p == 0 || !sp_word_before(T, s, p, slen);
            if (!free_front && !(p + n == slen || !sp_word_at(T, s, p + n, slen))) continue;
        }
        id = T.tok_ids[t];
        return n;
    }
    return 0;
}
// bit k: byte p16 + k (< slen) is some token's first byte
__device__ __forceinline__ uint32_t sp_candidates16(const SpSpecialDev& T, const uint8_t* s, int slen, int p16) {
    if (T.lit.n_first >= 0 && p16 + 16 <= slen) return bytes16_in_list(s + p16, T.lit.first, T.lit.n_first);
    uint32_t out = 0;
    const int n = slen - p16 < 16 ? slen - p16 : 16;
    for (int k = 0; k < n; ++k) {
        const uint32_t b = s[p16 + k];
        out |= uint32_t(T.bucket_off[b + 1] > T.bucket_off[b]) << k;
    }
    return out;
}

template <bool Write>
struct SpCut {
    SpSpecialDev T;
    const int32_t* begins;   // the rows
    const int32_t* ends;
    const uint8_t* chars;
    long long n_chars;
    int32_t* slot_cnt;        // [rows]  (count pass)
    const int32_t* slot_b;    // [rows]  the scan's offsets (write pass)
    int32_t* part_b;          // [slots] into chars; a token's slot: 0, 0
    int32_t* part_e;
    int32_t* slot_id;         // [slots] the token's id, -1: a part

    __device__ void operator()(long long row) const {
        const long long b = begins[row], e = ends[row];
        const int l = lane_id();
        int n_slots = 0;
        if (!(b < 0 || e < b || e > n_chars) && e > b) {   // (else: flagged by check_strings_kernel, or an empty row: no slot at all)
            const uint8_t* s = chars + b;
            const int slen = int(e - b);
            const long long out = Write ? slot_b[row] : 0;
            auto emit = [&](long long pb, long long pe, int32_t id) {
                if (Write && l == 0) {
                    part_b[out + n_slots] = int32_t(pb);
                    part_e[out + n_slots] = int32_t(pe);
                    slot_id[out + n_slots] = id;
                }
                ++n_slots;
            };
            int cursor = 0;
            for (int base = 0; base < slen; base += kSpCutStep) {
                const int p16 = base + 16 * l;
                uint32_t cand = p16 < slen ? sp_candidates16(T, s, slen, p16) : 0u;
                if (!__ballot(cand != 0u)) continue;
                uint32_t hit = 0;   // this lane's positions at which a token matches
                while (cand) {
                    const int k = __ffs(cand) - 1;
                    cand &= cand - 1u;
                    int32_t id;
                    if (sp_match_at(T, s, slen, p16 + k, id) > 0) hit |= 1u << k;
                }
                unsigned long long lanes = __ballot(hit != 0u);
                while (lanes) {   // the hits in order (wave-uniform from here on)
                    const int ln = __ffsll(lanes) - 1;
                    lanes &= lanes - 1ull;
                    uint32_t h = uint32_t(__shfl(int(hit), ln));
                    while (h) {
                        const int p = base + 16 * ln + (__ffs(h) - 1);
                        h &= h - 1u;
                        if (p < cursor) continue;   // inside the match before it
                        int32_t id = -1;
                        const int len = sp_match_at(T, s, slen, p, id);
                        if (cursor < p) emit(b + cursor, b + p, -1);
                        emit(0, 0, id);
                        cursor = p + len;
                    }
                }
            }
            if (cursor < slen) emit(b + cursor, b + slen, -1);
        }
        if (!Write && l == 0) slot_cnt[row] = n_slots;
    }
};

// The scan over the rows' slot counts ends here: the number of slots, for the host (RunStatus::n_pending has no other reader here).
struct SpSlotsFin {
    RunStatus* status;
    __device__ void operator()(long long total) const {
        status->n_pending = total > INT32_MAX ? INT32_MAX : int32_t(total);
        if (total >= INT32_MAX) atomicOr(&status->flags, kFlagItemsOverflow);
    }
};

// each_wave_kernel: the ids of a row -- every part's, one per token, eos -- and the longest row (it is no shorter than any part: the
// passes in front have raised RunStatus::width to the longest part at most).
struct SpRowLen {
    const int32_t* slot_b;     // [rows]
    const int32_t* slot_e;
    const int32_t* slot_id;    // [slots]
    const int32_t* part_len;   // [slots] ids of the part
    int32_t* row_len;          // [rows]
    int add_eos;
    RunStatus* status;
    __device__ void operator()(long long row) const {
        int sum = 0;
        for (int k = slot_b[row] + lane_id(); k < slot_e[row]; k += kWave) sum += slot_id[k] >= 0 ? 1 : part_len[k];
        sum = wave_sum(sum) + (add_eos ? 1 : 0);
        if (lane_id() == 0) {
            row_len[row] = sum;
            // (one address for every row of the batch: device_common.hpp on what such a counter sustains.  The passes in front have left the
            // longest part there, so only rows longer than that still have something to say; a stale read costs an atomic, never a
            // wrong maximum)
            if (sum > *const_cast<volatile int32_t*>(&status->width)) atomicMax(&status->width, sum);
        }
    }
};

// each_wave_kernel, behind the scan: a row's (row, position) pairs, one vector store each, and its values slot by slot.
struct SpAssemble {
    const int32_t* out_begins;   // [rows] the scan's offsets
    const int32_t* out_ends;
    const int32_t* slot_b;       // [rows]
    const int32_t* slot_e;
    const int32_t* slot_id;      // [slots]
    const int32_t* part_len;     // [slots]
    const long long* part_start; // [slots] where the part's ids start in src
    const int32_t* src;
    int64_t* indices;            // [total][2]
    int32_t* values;
    int32_t eos_id;
    int add_eos, reverse;
    __device__ void operator()(long long row) const {
        const long long ob = out_begins[row];
        const int len = int(out_ends[row] - ob);
        const int l = lane_id();
        SparsePair<int64_t>* dst = reinterpret_cast<SparsePair<int64_t>*>(indices) + ob;
        for (int k = l; k < len; k += kWave) dst[k] = SparsePair<int64_t>{int64_t(row), int64_t(k)};
        int32_t* val = values + ob;
        const bool rev = reverse && len > 1;
        int at = 0;
        for (int k = slot_b[row], ke = slot_e[row]; k < ke; ++k) {
            const int32_t id = slot_id[k];
            if (id >= 0) {
                if (l == 0) val[rev ? len - 1 - at : at] = id;
                ++at;
            } else {
                const int n = part_len[k];
                const int32_t* from = src + part_start[k];
                for (int i = l; i < n; i += kWave) val[rev ? len - 1 - (at + i) : at + i] = from[i];
                at += n;
            }
        }
        if (add_eos && l == 0) val[rev ? len - 1 - at : at] = eos_id;
    }
};

}  // namespace ovtk
