// sp_bpe_tables.hpp -- what ovtk_sentencepiece_create derives from a BPE model's vocabulary besides the pieces' trie: the refusals
// that belong to BPE models and the proof of the cut rule (host code, no HIP; tools/sp_bpe_host_check.cpp runs it under the sanitizers).
//
// The candidates' lookup is the trie of the NORMAL pieces (tables.hpp, TrieBucketsDev) walked over the text of two adjacent symbols:
// a symbol is always a contiguous stretch of the normalized text, so the pair's bytes are there to be walked, and the table needs
// nothing entered but the pieces themselves -- no split of a piece into operands, no refusal of a piece with a character that is
// no piece ("SentencepieceTokenizer, BPE models").
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "sp_model.hpp"

namespace ovtk {

// bpe::Model::Encode's characters: the length from the lead byte's high nibble, clipped to the end
inline size_t sp_bpe_char_count(const std::string& s) {
    size_t n = 0;
    for (size_t k = 0; k < s.size(); ++n) {
        const uint8_t b = uint8_t(s[k]);
        k += b < 0xC0 ? 1 : b < 0xE0 ? 2 : b < 0xF0 ? 3 : 4;
    }
    return n;
}

// false: a BPE model this library does not run, *why says which trait (the caller has already refused USER_DEFINED pieces).
inline bool sp_bpe_accepts(const SpModel& m, std::string* why) {
    std::vector<uint32_t> multi;   // the score bits of the NORMAL pieces of two or more characters
    for (const SpPiece& pc : m.pieces) {
        if (pc.type == kSpUnused) {
            *why = "a BPE model with UNUSED pieces (they are merged and split again by the sentence's last operands)";
            return false;
        }
        const size_t chars = sp_bpe_char_count(pc.piece);
        if (chars == 1 && (pc.type == kSpControl || pc.type == kSpUnknown || pc.type == kSpByte)) {
            *why = "a BPE model with a CONTROL, UNKNOWN or BYTE piece of one character (PieceToId would find it for that character)";
            return false;
        }
        if (pc.type == kSpNormal && chars >= 2) {
            float sc = pc.score == 0.0f ? 0.0f : pc.score;   // (-0 and +0 compare equal)
            uint32_t bits;
            std::memcpy(&bits, &sc, 4);
            multi.push_back(bits);
        }
    }
    std::sort(multi.begin(), multi.end());
    if (std::adjacent_find(multi.begin(), multi.end()) != multi.end()) {
        *why = "a BPE model in which two NORMAL pieces of two or more characters share one float32 score (no BPE trainer writes such a model)";
        return false;
    }
    return true;
}

// The cut rule: a symbol boundary p of the normalized text with text[p, p + 3) = "▁" and text[p - 3, p) != "▁" (or p < 3) is never
// inside a merged symbol.  A merged symbol is a NORMAL piece that equals text[a, c), a < p < c, and holds the whole character at p,
// so the piece has "▁" at its byte k = p - a >= 1 and not "▁" at [k - 3, k) (or k < 3): the rule holds when no NORMAL piece has that.
// Bytes only: nothing here assumes the text or the pieces to be valid UTF-8.
inline bool sp_bpe_cut_rule_holds(const SpModel& m) {
    static const char kSpace[3] = {char(0xE2), char(0x96), char(0x81)};
    for (const SpPiece& pc : m.pieces) {
        if (pc.type != kSpNormal) continue;
        const std::string& s = pc.piece;
        for (size_t k = 1; k + 3 <= s.size(); ++k)
            if (std::memcmp(s.data() + k, kSpace, 3) == 0 && !(k >= 3 && std::memcmp(s.data() + k - 3, kSpace, 3) == 0)) return false;
    }
    return true;
}

}  // namespace ovtk
