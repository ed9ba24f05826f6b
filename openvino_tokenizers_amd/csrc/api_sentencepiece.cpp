// api_sentencepiece.cpp -- C-ABI entry points of SentencepieceTokenizer (unigram and BPE models) and RaggedToSparse.  Compiled as HIP (hipcc -x hip).
// Reference behaviour replaced: src/sentence_piece.cpp:188-350 (evaluate, 4-input form: SentencePieceProcessor::Encode with the
// extra options of :58-73, then the sparse outputs of :331-347; 8-input form: the added tokens of :200-230 cut out of every row, the
// loop of :286-329 -- sp_special_kernels.hpp), src/ragged_to_sparse.cpp:27-47.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "api_common.hpp"
#include "charsmap_handle.hpp"
#include "ops_kernels.hpp"
#include "regex_compile.hpp"
#include "runtime.hpp"
#include "sentencepiece_kernels.hpp"
#include "sp_bpe_kernels.hpp"
#include "sp_bpe_tables.hpp"
#include "sp_model.hpp"
#include "sp_special_kernels.hpp"
#include "tables.hpp"

using namespace ovtk;

struct ovtk_sentencepiece {
    int device = 0;
    ovtk_charsmap* cm = nullptr;
    UnigramDev uni{};
    SpDev sp{};
    DevBuf root, buckets, scores, types, byte_ids;
    int32_t nbest_size = 0;
    float alpha = 0.0f;   // stored as the reference stores it; only sampling reads it
    bool bpe = false;     // a BPE model: sp_bpe_kernels.hpp stands where the lattice kernels stand
    int bpe_cuts = 0;     // ... and its cut rule is proved for this vocabulary (sp_bpe_tables.hpp)
    bool special = false;   // created with added tokens (the 8-input form): sp_special_kernels.hpp in front of and behind the passes
    SpSpecialDev spc{};
    DevBuf tok_begins, tok_ends, tok_chars, tok_ids, tok_alpha, bucket_off, bucket_tok, word_bits;
    int64_t min_token_len = 0;   // bytes of the shortest token (0: no tokens)
    ~ovtk_sentencepiece() { ovtk_charsmap_destroy(cm); }
};

namespace {

int sp_begin_status(Workspace& ws, hipStream_t s, RunStatus** st) {
    if (!ws.host_status) return set_error(OVTK_E_HIP, "pinned host allocation failed");
    if (int rc = ws.status.ensure(sizeof(RunStatus))) return rc;
    *st = ws.status.as<RunStatus>();
    OVTK_HIP(hipMemsetAsync(*st, 0, sizeof(RunStatus), s));
    return OVTK_OK;
}

// dense_shape of a call without a launch (an empty batch)
int sp_write_shape(int64_t* dense_shape, int64_t rows, int64_t width, int mem, hipStream_t s) {
    const int64_t v[2] = {rows, width};
    if (mem == OVTK_MEM_HOST) {
        std::memcpy(dense_shape, v, sizeof v);
        return OVTK_OK;
    }
    OVTK_HIP(hipMemcpyAsync(dense_shape, v, sizeof v, hipMemcpyHostToDevice, s));
    OVTK_HIP(hipStreamSynchronize(s));
    return OVTK_OK;
}

// The added tokens of the 8-input form, in input order (host side).
struct SpSpecialHost {
    std::vector<std::string> tokens;
    std::vector<int32_t> ids;
};

bool sp_valid_utf8(const std::string& t) {   // what pcre2_compile(PCRE2_UTF) accepts: no overlong form, no surrogate, nothing above U+10FFFF
    const size_t n = t.size();
    for (size_t i = 0; i < n;) {
        const uint32_t b = uint8_t(t[i]);
        if (b < 0x80u) {
            ++i;
            continue;
        }
        const int len = b >= 0xF0u ? 4 : (b >= 0xE0u ? 3 : 2);
        if (b < 0xC2u || b > 0xF4u || i + size_t(len) > n) return false;
        uint32_t cp = b & (0xFFu >> (len + 1));
        for (int k = 1; k < len; ++k) {
            const uint32_t c = uint8_t(t[i + size_t(k)]);
            if ((c & 0xC0u) != 0x80u) return false;
            cp = (cp << 6) | (c & 0x3Fu);
        }
        if ((len == 3 && cp < 0x800u) || (len == 4 && cp < 0x10000u) || cp > 0x10FFFFu || (cp >= 0xD800u && cp <= 0xDFFFu)) return false;
        i += size_t(len);
    }
    return true;
}

// The device tables of the added tokens (sp_special_kernels.hpp).
int sp_upload_special(ovtk_sentencepiece& h, const SpSpecialHost& sp) {
    const size_t n = sp.tokens.size();
    std::vector<int32_t> begins(n), ends(n), bucket_off(257, 0), bucket_tok(n);
    std::vector<uint8_t> chars, alpha(n);
    int64_t shortest = 0;
    for (size_t i = 0; i < n; ++i) {
        const std::string& t = sp.tokens[i];
        begins[i] = int32_t(chars.size());
        ends[i] = begins[i] + int32_t(t.size());
        chars.insert(chars.end(), t.begin(), t.end());
        chars.resize((chars.size() + 15) & ~size_t(15), 0);   // token_at compares 16 bytes at a time
        alpha[i] = std::all_of(t.begin(), t.end(), [](char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }) ? 1 : 0;   // std::isalpha, "C" locale
        shortest = i == 0 ? int64_t(t.size()) : std::min<int64_t>(shortest, int64_t(t.size()));
        ++bucket_off[size_t(uint8_t(t[0])) + 1];
    }
    for (int b = 0; b < 256; ++b) bucket_off[size_t(b) + 1] += bucket_off[size_t(b)];
    std::vector<int32_t> fill(bucket_off.begin(), bucket_off.end() - 1);
    for (size_t i = 0; i < n; ++i) bucket_tok[size_t(fill[uint8_t(sp.tokens[i][0])]++)] = int32_t(i);
    std::vector<uint8_t> gc;
    unicode_general_categories(gc);
    std::vector<uint32_t> word(kSpWordTableWords, 0u);
    for (uint32_t cp = 0; cp < 0x110000u; ++cp) {   // unicode_gc.inc's order: Lu Ll Lt Lm Lo = 1..5, Mn = 6, Nd Nl No = 9..11, Pc = 12
        const unsigned g = gc[cp];
        if ((g >= 1 && g <= 6) || (g >= 9 && g <= 12)) word[cp >> 5] |= 1u << (cp & 31u);
    }
    std::vector<int32_t> ids = sp.ids;
    if (n == 0) {   // (no empty uploads: one entry nobody reads)
        chars.resize(16, 0);
        begins.resize(1, 0);
        ends.resize(1, 0);
        ids.resize(1, 0);
        alpha.resize(1, 0);
        bucket_tok.resize(1, 0);
    }
    if (int rc = h.tok_begins.upload(begins.data(), begins.size() * 4)) return rc;
    if (int rc = h.tok_ends.upload(ends.data(), ends.size() * 4)) return rc;
    if (int rc = h.tok_chars.upload(chars.data(), chars.size())) return rc;
    if (int rc = h.tok_ids.upload(ids.data(), ids.size() * 4)) return rc;
    if (int rc = h.tok_alpha.upload(alpha.data(), alpha.size())) return rc;
    if (int rc = h.bucket_off.upload(bucket_off.data(), bucket_off.size() * 4)) return rc;
    if (int rc = h.bucket_tok.upload(bucket_tok.data(), bucket_tok.size() * 4)) return rc;
    if (int rc = h.word_bits.upload(word.data(), word.size() * 4)) return rc;
    SpSpecialDev& d = h.spc;
    d = SpSpecialDev{};
    d.lit.tok_begins = h.tok_begins.as<int32_t>();
    d.lit.tok_ends = h.tok_ends.as<int32_t>();
    d.lit.tok_chars = h.tok_chars.as<uint8_t>();
    d.lit.n_tokens = int32_t(n);
    d.lit.n_tok_chars = int32_t(chars.size());
    d.lit.tok_padded = 1;
    d.lit.n_tok_first = -1;
    d.lit.n_first = 0;
    for (int b = 0; b < 256; ++b) {
        if (bucket_off[size_t(b) + 1] == bucket_off[size_t(b)]) continue;
        d.lit.first_bytes[b >> 5] |= 1u << (b & 31);
        if (d.lit.n_first >= 0 && d.lit.n_first < 16) d.lit.first[d.lit.n_first++] = uint8_t(b);
        else d.lit.n_first = -1;   // more than 16 distinct first bytes: the sweep asks the buckets byte by byte
    }
    d.tok_ids = h.tok_ids.as<int32_t>();
    d.tok_alpha = h.tok_alpha.as<uint8_t>();
    d.bucket_off = h.bucket_off.as<int32_t>();
    d.bucket_tok = h.bucket_tok.as<int32_t>();
    d.word_bits = h.word_bits.as<uint32_t>();
    h.special = true;
    h.min_token_len = shortest;
    return OVTK_OK;
}

int sp_create(const uint8_t* model, int64_t model_len, const ovtk_sentencepiece_params* p, const SpSpecialHost* special, ovtk_sentencepiece** out);

}  // namespace

extern "C" {

int ovtk_sentencepiece_create(const uint8_t* model, int64_t model_len, const ovtk_sentencepiece_params* p, ovtk_sentencepiece** out) {
    return sp_create(model, model_len, p, nullptr, out);
}

int ovtk_sentencepiece_create_special(const uint8_t* model, int64_t model_len, const ovtk_sentencepiece_params* p, const ovtk_strings* tokens,
                                      const int32_t* token_ids, ovtk_sentencepiece** out) {
    if (!tokens || tokens->n < 0 || tokens->n_chars < 0 || (tokens->n > 0 && (!tokens->begins || !tokens->ends || !token_ids)) ||
        (tokens->n_chars > 0 && !tokens->chars))
        return set_error(OVTK_E_ARG, "sentencepiece: bad special-token argument");
    if (tokens->n > kSpMaxSpecialTokens)
        return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: more than 4 096 special tokens");
    SpSpecialHost sp;
    for (int64_t i = 0; i < tokens->n; ++i) {
        const int64_t b = tokens->begins[i], e = tokens->ends[i];
        if (b < 0 || e < b || e > tokens->n_chars) return set_error(OVTK_E_RANGE, "sentencepiece: a special token's begins/ends index outside its chars tensor");
        if (e == b) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: an empty special token (its alternative \\b|\\b would end every search)");
        if (e - b > kSpMaxSpecialTokenBytes) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: a special token is longer than 1 023 bytes");
        sp.tokens.emplace_back(reinterpret_cast<const char*>(tokens->chars) + b, size_t(e - b));
        if (token_ids[i] < 0)   // (the slot lists mark a part by a negative id; the reference would push the id as it is)
            return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: a special token with a negative id");
        sp.ids.push_back(token_ids[i]);
        if (!sp_valid_utf8(sp.tokens.back()))
            return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: a special token is not valid UTF-8 (the reference's pattern does not compile and matches nothing)");
    }
    return sp_create(model, model_len, p, &sp, out);
}

}  // extern "C"

namespace {

// The slots of a call with added tokens (sp_special_kernels.hpp): workspace buffers the passes behind do not touch.
struct SpSlots {
    int64_t n = 0;                                // slots of the batch
    int32_t *slot_b = nullptr, *slot_e = nullptr;  // [rows] a row's slots
    int32_t* row_len = nullptr;                   // [rows] ids of the row (the assemble pass)
    int32_t *part_b = nullptr, *part_e = nullptr;  // [n] into the caller's chars
    int32_t* slot_id = nullptr;                   // [n]
};
// Cuts the rows at the added tokens: count -> scan -> (the host reads the number of slots and sizes their buffers) -> write.
// st: the call's zeroed status block; it stays the first attempt's.
int sp_cut_rows(ovtk_sentencepiece* h, Workspace& ws, hipStream_t s, RunStatus* st, int64_t n_rows, const int32_t* b, const int32_t* e, const uint8_t* c,
                int64_t n_chars, SpSlots& o) {
    if (int rc = ws.row_cnt.ensure(size_t(n_rows) * 4)) return rc;
    if (int rc = ws.in_rb.ensure(size_t(n_rows) * 4)) return rc;
    if (int rc = ws.in_re.ensure(size_t(n_rows) * 4)) return rc;
    if (int rc = ws.exact.ensure(size_t(n_rows) * 4)) return rc;
    if (int rc = ws.tiles.ensure(scan_tiles_bytes(n_rows))) return rc;
    int32_t* slot_cnt = ws.row_cnt.as<int32_t>();
    o.slot_b = ws.in_rb.as<int32_t>();
    o.slot_e = ws.in_re.as<int32_t>();
    o.row_len = ws.exact.as<int32_t>();
    const int row_grid = int(std::min<long long>((n_rows + kTileThreads / kWave - 1) / (kTileThreads / kWave), (long long)device_cu_count(h->device) * 16));
    OVTK_LAUNCH(ws.marks, "check_strings", check_strings_kernel, grid_for_elems(n_rows), kBlockThreads, s, b, e, (long long)n_rows, (long long)n_chars, st);
    OVTK_LAUNCH(ws.marks, "sp_special_count", each_wave_kernel<SpCut<false>>, row_grid, kTileThreads, s, (long long)n_rows,
                (SpCut<false>{h->spc, b, e, c, (long long)n_chars, slot_cnt, nullptr, nullptr, nullptr, nullptr}), (const RunStatus*)st, kFlagRange);
    launch_scan(ws.marks, "sp_special_offsets", s, n_rows, FiledLen{slot_cnt}, RowOffsets{o.slot_b, o.slot_e, 0}, SpSlotsFin{st}, ws.tiles.as<long long>(), st,
                kFlagRange);
    if (int rc = finish_status(ws, s)) return rc;
    const uint32_t f = ws.host_status->flags;
    if (f & kFlagRange) return set_error(OVTK_E_RANGE, "input begins/ends index outside the chars tensor");
    o.n = ws.host_status->n_pending;
    if ((f & kFlagItemsOverflow) || o.n >= INT32_MAX - 1) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: too many parts for one call; split it");
    const size_t room = size_t(std::max<int64_t>(o.n, 1)) * 4;
    if (int rc = ws.row_stage.ensure(room)) return rc;
    if (int rc = ws.row_used.ensure(room)) return rc;
    if (int rc = ws.wave_off.ensure(room)) return rc;
    o.part_b = ws.row_stage.as<int32_t>();
    o.part_e = ws.row_used.as<int32_t>();
    o.slot_id = ws.wave_off.as<int32_t>();
    if (o.n > 0)
        OVTK_LAUNCH(ws.marks, "sp_special_cut", each_wave_kernel<SpCut<true>>, row_grid, kTileThreads, s, (long long)n_rows,
                    (SpCut<true>{h->spc, b, e, c, (long long)n_chars, nullptr, o.slot_b, o.part_b, o.part_e, o.slot_id}), (const RunStatus*)st, kFlagRange);
    return OVTK_OK;
}

// special: the added tokens of ovtk_sentencepiece_create_special, nullptr for ovtk_sentencepiece_create.
int sp_create(const uint8_t* model, int64_t model_len, const ovtk_sentencepiece_params* p, const SpSpecialHost* special, ovtk_sentencepiece** out) {
    if (!p || !out || model_len < 0 || (model_len > 0 && !model)) return set_error(OVTK_E_ARG, "sentencepiece: bad argument");
    SpModel m;
    std::string why;
    if (!sp_model_parse(model, size_t(model_len), m, &why)) return set_error(OVTK_E_ARG, "sentencepiece: the model is truncated or malformed (in " + why + ")");
    if (m.pieces.empty()) return set_error(OVTK_E_ARG, "sentencepiece: the model has no pieces");
    // what this library does not run (never an approximation)
    if (p->nbest_size != 0 && p->nbest_size != 1)
        return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: nbest_size other than 0 or 1 selects SampleEncode, which is random (sentence_piece.cpp:238-241)");
    if (!special && p->reverse && (p->add_bos || p->add_eos))   // (the 8-input form applies eos and reverse itself: :196-197, :323-328)
        return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: reverse together with add_bos / add_eos depends on the order of the extra options (sentence_piece.cpp:58-73)");
    if (m.model_type != kSpUnigram && m.model_type != kSpBpe)
        return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: only UNIGRAM and BPE models run here; WORD and CHAR models are the follow-up");
    const bool bpe = m.model_type == kSpBpe;
    if (m.treat_whitespace_as_suffix) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: treat_whitespace_as_suffix");
    if (int64_t(m.pieces.size()) >= int64_t(kUniUnkCode)) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: more than 4 194 302 pieces");
    // ModelInterface::InitializePieces: one UNKNOWN piece, no empty and no repeated piece; min / max score over the NORMAL ones
    std::unordered_map<std::string, int32_t> id_of;
    int32_t unk_id = -1;
    float min_score = FLT_MAX;
    bool byte_found[256] = {};
    std::vector<uint8_t> types(m.pieces.size());
    std::vector<float> scores(m.pieces.size());
    for (size_t i = 0; i < m.pieces.size(); ++i) {
        const SpPiece& pc = m.pieces[i];
        if (pc.piece.empty()) return set_error(OVTK_E_ARG, "sentencepiece: piece " + std::to_string(i) + " is empty");
        if (!id_of.emplace(pc.piece, int32_t(i)).second) return set_error(OVTK_E_ARG, "sentencepiece: piece " + std::to_string(i) + " is already defined");
        if (pc.piece.size() > size_t(kUniMaxTokenBytes)) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: a piece is longer than 1 023 bytes");
        types[i] = pc.type;
        scores[i] = pc.score;
        if (pc.type == kSpUserDefined)
            return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: the model has USER_DEFINED pieces (they bypass the normalizer and score in mixed precision)");
        if (pc.type == kSpNormal) min_score = std::min(min_score, pc.score);
        if (pc.type == kSpUnknown) {
            if (unk_id >= 0) return set_error(OVTK_E_ARG, "sentencepiece: unk is already defined");
            unk_id = int32_t(i);
        }
        if (pc.type == kSpByte) {
            if (!m.byte_fallback) return set_error(OVTK_E_ARG, "sentencepiece: a BYTE piece in a model without byte_fallback");
            unsigned v = 0;
            char tail = 0;
            if (pc.piece.size() != 6 || std::sscanf(pc.piece.c_str(), "<0x%2X%c", &v, &tail) != 2 || tail != '>' || v > 255)
                return set_error(OVTK_E_ARG, "sentencepiece: a BYTE piece that is not <0xHH>");
            byte_found[v] = true;
        }
    }
    if (unk_id < 0) return set_error(OVTK_E_ARG, "sentencepiece: unk is not defined");
    if (m.byte_fallback)
        for (bool f : byte_found)
            if (!f) return set_error(OVTK_E_ARG, "sentencepiece: byte_fallback without all 256 BYTE pieces");
    // SentencePieceProcessor::PieceToId / bos_id() / eos_id(): the piece's id if it is a CONTROL piece, else -1
    auto piece_to_id = [&](const std::string& s) {
        const auto it = id_of.find(s);
        return it == id_of.end() ? unk_id : it->second;
    };
    auto control_id = [&](const std::string& s) {
        const int32_t id = piece_to_id(s);
        return types[size_t(id)] == kSpControl ? id : -1;
    };
    const int32_t bos_id = control_id(m.bos_piece), eos_id = control_id(m.eos_piece);
    if (p->add_bos && bos_id < 0) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: add_bos with a model that has no bos piece (sentencepiece raises)");
    if (p->add_eos && eos_id < 0) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: add_eos with a model that has no eos piece (sentencepiece raises)");
    if (bpe) {
        std::string refusal;
        if (!sp_bpe_accepts(m, &refusal)) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: " + refusal);
    }
    int32_t byte_ids[256];
    for (int v = 0; v < 256; ++v) {
        char name[8];
        std::snprintf(name, sizeof name, "<0x%02X>", v);
        byte_ids[v] = piece_to_id(name);
    }

    if (int rc = use_device(p->device)) return rc;
    auto h = std::make_unique<ovtk_sentencepiece>();
    h->device = p->device;
    h->nbest_size = p->nbest_size;
    h->alpha = p->alpha;
    h->bpe = bpe;
    h->bpe_cuts = bpe && sp_bpe_cut_rule_holds(m) ? 1 : 0;
    const ovtk_charsmap_params cp{m.add_dummy_prefix, m.remove_extra_whitespaces, m.escape_whitespaces};
    if (int rc = ovtk_charsmap_create(reinterpret_cast<const uint8_t*>(m.precompiled_charsmap.data()), int64_t(m.precompiled_charsmap.size()), &cp,
                                      p->device, &h->cm))
        return rc;   // (the builder's own refusals, its message)
    TrieHost t;
    for (size_t i = 0; i < m.pieces.size(); ++i)   // (ModelInterface::InitializePieces: the other types go to a map no text is looked up in)
        if (types[i] == kSpNormal || (!bpe && (types[i] == kSpUserDefined || types[i] == kSpUnused)))   // (BPE: the candidates' lookup; such models have neither)
            t.add(reinterpret_cast<const uint8_t*>(m.pieces[i].piece.data()), m.pieces[i].piece.size(), int32_t(i));
    TrieBucketsHost tb;
    if (!tb.build(t)) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: the pieces' trie has more than 8 million nodes");
    if (int rc = h->root.upload(tb.root.data(), tb.root.size() * sizeof(I2))) return rc;
    if (int rc = h->buckets.upload(tb.buckets.data(), tb.buckets.size() * sizeof(TrieBucket))) return rc;
    if (int rc = h->scores.upload(scores.data(), scores.size() * sizeof(float))) return rc;
    if (int rc = h->types.upload(types.data(), types.size())) return rc;
    if (int rc = h->byte_ids.upload(byte_ids, sizeof byte_ids)) return rc;
    h->uni.trie = TrieBucketsDev{h->root.as<I2>(), h->buckets.as<TrieBucket>(), tb.bucket_mask, tb.bucket_shift};
    h->uni.scores = h->scores.as<float>();
    h->uni.unk_score = min_score - 10.0f;   // unigram_model.cc: min_score() - kUnkPenalty, float32 (FLT_MAX - 10 without a NORMAL piece)
    h->uni.unk_token_id = unk_id;
    h->sp = SpDev{h->types.as<uint8_t>(), h->byte_ids.as<int32_t>(), bos_id, eos_id, m.byte_fallback ? 1 : 0, p->add_bos != 0, p->add_eos != 0, p->reverse != 0};
    if (special)
        if (int rc = sp_upload_special(*h, *special)) return rc;
    OVTK_HIP(hipStreamSynchronize(nullptr));
    *out = h.release();
    return OVTK_OK;
}

}  // namespace

extern "C" {

void ovtk_sentencepiece_destroy(ovtk_sentencepiece* h) { delete h; }

int64_t ovtk_sentencepiece_bound(ovtk_sentencepiece* h, int64_t n, int64_t n_chars) {
    if (!h || n < 0 || n_chars < 0) return -1;
    if (!h->special) return ovtk_charsmap_bound(h->cm, n, n_chars) + 2 * n;   // an id per normalized byte at most, bos and eos
    // added tokens: a match takes at least the shortest token's bytes, so there are at most k = n_chars / shortest of them (each an id)
    // and k + n parts (every one normalized by itself and given a bos); an eos per row
    const int64_t k = h->min_token_len > 0 ? n_chars / h->min_token_len : 0;
    return ovtk_charsmap_bound(h->cm, k + n, n_chars) + (k + n) + k + n;
}

int ovtk_sentencepiece_run(ovtk_sentencepiece* h, const ovtk_strings* in, ovtk_sparse_i32_out* out, int mem, void* stream) {
    if (!h || !in || !out) return set_error(OVTK_E_ARG, "sentencepiece: null argument");
    if (in->n < 0 || in->n_chars < 0 || out->capacity < 0) return set_error(OVTK_E_ARG, "sentencepiece: negative size");
    if (in->n >= INT32_MAX || in->n_chars >= INT32_MAX) return set_error(OVTK_E_ARG, "sentencepiece: tensor sizes must fit int32 offsets");
    if (!out->dense_shape) return set_error(OVTK_E_ARG, "sentencepiece: null dense_shape");
    if (mem != OVTK_MEM_HOST && mem != OVTK_MEM_DEVICE) return set_error(OVTK_E_ARG, "mem must be OVTK_MEM_HOST or OVTK_MEM_DEVICE");
    if (mem == OVTK_MEM_DEVICE && (reinterpret_cast<uintptr_t>(out->indices) & 15u))
        return set_error(OVTK_E_ARG, "sentencepiece: the indices buffer must be 16-byte aligned");
    if (int rc = use_device(h->device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    out->n = 0;
    if (in->n == 0) return sp_write_shape(out->dense_shape, 0, 0, mem, s);
    const int64_t n_rows = in->n;
    int64_t n = n_rows;   // the sentences of the passes: the rows, or -- a handle with added tokens -- their parts
    WorkspaceLease ws(h->device);
    RunStatus* st = nullptr;
    if (int rc = sp_begin_status(*ws.ws, s, &st)) return rc;
    const int32_t *b = nullptr, *e = nullptr;
    const uint8_t* c = nullptr;
    if (int rc = in_source(ws->in_begins, in->begins, size_t(n) * 4, mem, s, &b)) return rc;
    if (int rc = in_source(ws->in_ends, in->ends, size_t(n) * 4, mem, s, &e)) return rc;
    if (int rc = in_source(ws->in_chars, in->chars, size_t(in->n_chars), mem, s, &c)) return rc;
    int64_t* d_idx = nullptr;
    int32_t* d_val = nullptr;
    int64_t* d_shape = nullptr;
    const size_t out_cap = size_t(std::max<int64_t>(out->capacity, 1));
    if (int rc = out_target(ws->out_a, out->indices, out_cap * 16, mem, &d_idx)) return rc;
    if (int rc = out_target(ws->out_b, out->values, out_cap * 4, mem, &d_val)) return rc;
    if (int rc = out_target(ws->out_c, out->dense_shape, size_t(16), mem, &d_shape)) return rc;
    if ((n_rows + kTileElems - 1) / kTileElems > INT32_MAX) return set_error(OVTK_E_UNSUPPORTED, "too many strings for one call; split it");
    SpDev sp = h->sp;
    SpSlots slots{};
    if (h->special) {   // the rows are cut at the added tokens; eos and reverse are the assemble pass's (sentence_piece.cpp:196-197, :323-328)
        if (int rc = sp_cut_rows(h, *ws.ws, s, st, n_rows, b, e, c, in->n_chars, slots)) return rc;
        n = slots.n;
        b = slots.part_b;
        e = slots.part_e;
        sp.add_eos = 0;
        sp.reverse = 0;
    }
    // the normalized text: any input of this size fits ovtk_charsmap_bound bytes (int32 offsets: the rest is the flag's business)
    const int64_t norm_cap = std::min<int64_t>(std::max<int64_t>(ovtk_charsmap_bound(h->cm, n, in->n_chars), 16), INT32_MAX - 1);
    if (int rc = ws->scratch.ensure(size_t(norm_cap))) return rc;
    if (int rc = ws->gen[7].ensure(size_t(n) * 12)) return rc;
    if (int rc = ws->out_d.ensure(size_t(n_rows) * 4)) return rc;
    if (int rc = ws->out_e.ensure(size_t(n_rows) * 4)) return rc;
    uint8_t* norm = ws->scratch.as<uint8_t>();
    int32_t* norm_len = ws->gen[7].as<int32_t>();
    int32_t *norm_b = norm_len + n, *norm_e = norm_len + 2 * n;
    int32_t *row_b = ws->out_d.as<int32_t>(), *row_e = ws->out_e.as<int32_t>();
    if (int rc = ws->gen[0].ensure(size_t(n) * 8)) return rc;
    if (int rc = ws->gen[1].ensure(size_t(n) * 4)) return rc;
    if (int rc = ws->gen[2].ensure(size_t(n) * 4)) return rc;
    if (int rc = ws->gen[3].ensure(size_t(n) * 8)) return rc;
    if ((n + kTileElems - 1) / kTileElems > INT32_MAX) return set_error(OVTK_E_UNSUPPORTED, "too many strings for one call; split it");
    if (int rc = ws->tiles.ensure(scan_tiles_bytes(std::max(n, n_rows)))) return rc;
    UniWork w{};
    w.begins = norm_b;
    w.ends = norm_e;
    w.chars = norm;
    w.n_rows = 0;
    w.n_strings = n;
    w.n_chars = norm_cap;
    w.dev = h->uni;
    w.node_off = ws->gen[0].as<long long>();
    w.str_over = ws->gen[2].as<int32_t>();
    int32_t* row_len = ws->gen[1].as<int32_t>();
    long long* row_start = ws->gen[3].as<long long>();
    const CharsmapDev& cm = h->cm->dev;
    const int wave_grid = int(std::min<long long>((n + kTileThreads / kWave - 1) / (kTileThreads / kWave), (long long)device_cu_count(h->device) * 16));
    const int row_grid = int(std::min<long long>((n_rows + kTileThreads / kWave - 1) / (kTileThreads / kWave), (long long)device_cu_count(h->device) * 16));
    const unsigned lane_grid = unsigned((n + kTileThreads - 1) / kTileThreads);
    constexpr uint32_t kStop = kFlagRange | kFlagItemsOverflow | kFlagStageOverflow;
    // a node per normalized byte and one per sentence; the text usually grows by its escaped spaces: a second attempt where it grows more
    int64_t cap = std::min<int64_t>(2 * in->n_chars + 4 * n + 64, norm_cap + n + 1);
    uint32_t f = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (attempt)
            if (int rc = sp_begin_status(*ws.ws, s, &st)) return rc;
        w.status = st;
        if (cap >= INT32_MAX - 1) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: too much text for one call; split it");
        if (int rc = ws->gen[4].ensure(size_t(cap) * sizeof(int32_t))) return rc;
        if (int rc = ws->gen[5].ensure(size_t(cap) * (h->bpe ? sizeof(SpBpeSym) : sizeof(UniEdgeList)))) return rc;
        if (int rc = ws->gen[6].ensure(size_t(cap) * sizeof(UniNode))) return rc;
        if (int rc = ws->stage.ensure(size_t(cap + 2 * n + 2) * sizeof(int32_t))) return rc;
        w.owner = ws->gen[4].as<int32_t>();
        w.lists = ws->gen[5].as<UniEdgeList>();
        w.nodes = ws->gen[6].as<UniNode>();
        w.ids = ws->stage.as<int32_t>();
        w.cap = cap;
        if (n > 0) {   // (a handle with added tokens and a batch of empty rows: no sentence at all)
            // normalize: a wave per sentence counts -> scan -> a wave per sentence writes
            OVTK_LAUNCH(ws->marks, "check_strings", check_strings_kernel, grid_for_elems(n), kBlockThreads, s, b, e, (long long)n, (long long)in->n_chars, st);
            OVTK_LAUNCH(ws->marks, "sp_norm_count", each_wave_kernel<CmRow<false>>, wave_grid, kTileThreads, s, (long long)n,
                        (CmRow<false>{cm, b, e, c, (long long)in->n_chars, nullptr, norm_len, nullptr, nullptr}), (const RunStatus*)st, kFlagRange);
            launch_scan(ws->marks, "sp_norm_offsets", s, n, FiledLen{norm_len}, RowOffsets{norm_b, norm_e, 0}, SpNormFin{st, (long long)norm_cap},
                        ws->tiles.as<long long>(), st, kFlagRange);
            OVTK_LAUNCH(ws->marks, "sp_norm_write", each_wave_kernel<CmRow<true>>, wave_grid, kTileThreads, s, (long long)n,
                        (CmRow<true>{cm, b, e, c, (long long)in->n_chars, nullptr, norm_len, norm_b, norm}), (const RunStatus*)st, kStop);
            if (h->bpe) {
                // symbols, segments, merges and ids: a wave per normalized sentence (gen[5]: the left-over path's symbol lists)
                launch_scan(ws->marks, "spbpe_stretch", s, n, SpBpeStretch{w}, SpBpeStretchApply{w}, UniStretchFin{st, (long long)cap}, ws->tiles.as<long long>(),
                            st, kFlagRange | kFlagItemsOverflow);
                OVTK_LAUNCH(ws->marks, "spbpe_merge", sp_bpe_kernel, wave_grid, kTileThreads, s, (long long)n,
                            (SpBpeRow{w, sp, ws->gen[5].as<SpBpeSym>(), row_start, row_len, h->bpe_cuts}), st, kStop);
            } else {
                // the lattice over each normalized sentence
                launch_scan(ws->marks, "sp_stretch", s, n, UniStretch{w}, UniStretchApply{w}, UniStretchFin{st, (long long)cap}, ws->tiles.as<long long>(), st,
                            kFlagRange | kFlagItemsOverflow);
                OVTK_LAUNCH(ws->marks, "sp_edges", unigram_edges_kernel, unsigned((cap + kTileThreads - 1) / kTileThreads), kTileThreads, s, w);
                OVTK_LAUNCH(ws->marks, "sp_relax", sp_relax_kernel, lane_grid, kTileThreads, s, (long long)n, (SpRelax{w, sp, row_start, row_len}), st, kStop);
            }
        }
        // the sparse outputs
        if (h->special) {
            // a row's ids: its parts', its tokens', eos -> scan -> the pairs and the values, slot by slot
            OVTK_LAUNCH(ws->marks, "sp_special_rows", each_wave_kernel<SpRowLen>, row_grid, kTileThreads, s, (long long)n_rows,
                        (SpRowLen{slots.slot_b, slots.slot_e, slots.slot_id, row_len, slots.row_len, h->sp.add_eos, st}), (const RunStatus*)st, kStop);
            launch_scan(ws->marks, "sp_offsets", s, n_rows, FiledLen{slots.row_len}, RowOffsets{row_b, row_e, 0},
                        (SparseFin<int64_t>{st, (long long)std::min<int64_t>(out->capacity, INT32_MAX - 1), (long long)n_rows, kStop, d_shape}),
                        ws->tiles.as<long long>(), st, kStop);
            OVTK_LAUNCH(ws->marks, "sp_special_assemble", each_wave_kernel<SpAssemble>, row_grid, kTileThreads, s, (long long)n_rows,
                        (SpAssemble{row_b, row_e, slots.slot_b, slots.slot_e, slots.slot_id, row_len, row_start, w.ids, d_idx, d_val, h->sp.eos_id,
                                    h->sp.add_eos, h->sp.reverse}),
                        (const RunStatus*)st, kStop | kFlagOutCapacity);
        } else {
            launch_scan(ws->marks, "sp_offsets", s, n, FiledLen{row_len}, RowOffsets{row_b, row_e, 0},
                        (SparseFin<int64_t>{st, (long long)std::min<int64_t>(out->capacity, INT32_MAX - 1), (long long)n, kStop, d_shape}),
                        ws->tiles.as<long long>(), st, kStop);
            OVTK_LAUNCH(ws->marks, "sp_sparse", each_wave_kernel<SparseRows<int64_t>>, wave_grid, kTileThreads, s, (long long)n,
                        (SparseRows<int64_t>{row_b, row_e, d_idx, row_start, w.ids, d_val}), (const RunStatus*)st, kStop | kFlagOutCapacity);
        }
        if (int rc = finish_status(*ws.ws, s)) return rc;
        f = ws->host_status->flags;
        if (f & kFlagRange) return set_error(OVTK_E_RANGE, "input begins/ends index outside the chars tensor");
        if (f & kFlagItemsOverflow)
            return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: the normalized text reaches 2^31 bytes; split the call");
        if (!(f & kFlagStageOverflow)) break;
        if (ws->host_status->stage_need >= INT32_MAX - 1) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceTokenizer: too much text for one call; split it");
        if (attempt) return set_error(OVTK_E_HIP, "SentencepieceTokenizer: workspace sizing did not converge");
        cap = ws->host_status->stage_need;
    }
    if (h->bpe && ws->host_status->n_exact > 0) Profiler::get().count("spbpe_leftover_segments", ws->host_status->n_exact);
    out->n = ws->host_status->n_out;
    if (f & kFlagOutCapacity)
        return set_error(OVTK_E_CAPACITY, "SentencepieceTokenizer: output buffers too small (" + std::to_string(out->n) + " ids, capacity " +
                                              std::to_string(out->capacity) + ")");
    int err = 0;
    err = err ? err : copy_back(out->indices, d_idx, size_t(out->n) * 16, mem, s);
    err = err ? err : copy_back(out->values, d_val, size_t(out->n) * 4, mem, s);
    err = err ? err : copy_back(out->dense_shape, d_shape, size_t(16), mem, s);
    if (err) return err;
    if (mem == OVTK_MEM_HOST) OVTK_HIP(hipStreamSynchronize(s));
    return OVTK_OK;
}

int ovtk_ragged_to_sparse(const int32_t* begins, const int32_t* ends, int64_t n_rows, int32_t* out, int64_t capacity, int64_t* n_out, int mem,
                          int device, void* stream) {
    if (!n_out || n_rows < 0 || capacity < 0 || (n_rows > 0 && (!begins || !ends))) return set_error(OVTK_E_ARG, "ragged_to_sparse: bad argument");
    if (n_rows >= INT32_MAX) return set_error(OVTK_E_ARG, "ragged_to_sparse: tensor sizes must fit int32 offsets");
    if (mem != OVTK_MEM_HOST && mem != OVTK_MEM_DEVICE) return set_error(OVTK_E_ARG, "mem must be OVTK_MEM_HOST or OVTK_MEM_DEVICE");
    if (mem == OVTK_MEM_DEVICE && (reinterpret_cast<uintptr_t>(out) & 7u)) return set_error(OVTK_E_ARG, "ragged_to_sparse: the output must be 8-byte aligned");
    if (int rc = use_device(device)) return rc;
    *n_out = 0;
    if (n_rows == 0) return OVTK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WorkspaceLease ws(device);
    RunStatus* st = nullptr;
    if (int rc = sp_begin_status(*ws.ws, s, &st)) return rc;
    const int32_t *b = nullptr, *e = nullptr;
    if (int rc = in_source(ws->in_begins, begins, size_t(n_rows) * 4, mem, s, &b)) return rc;
    if (int rc = in_source(ws->in_ends, ends, size_t(n_rows) * 4, mem, s, &e)) return rc;
    int32_t* d_out = nullptr;
    if (int rc = out_target(ws->out_a, out, size_t(std::max<int64_t>(capacity, 1)) * 8, mem, &d_out)) return rc;
    if (int rc = ws->out_d.ensure(size_t(n_rows) * 4)) return rc;
    if (int rc = ws->out_e.ensure(size_t(n_rows) * 4)) return rc;
    if ((n_rows + kTileElems - 1) / kTileElems > INT32_MAX) return set_error(OVTK_E_UNSUPPORTED, "too many rows for one call; split it");
    if (int rc = ws->tiles.ensure(scan_tiles_bytes(n_rows))) return rc;
    int32_t *row_b = ws->out_d.as<int32_t>(), *row_e = ws->out_e.as<int32_t>();
    const int wave_grid = int(std::min<long long>((n_rows + kTileThreads / kWave - 1) / (kTileThreads / kWave), (long long)device_cu_count(device) * 16));
    launch_scan(ws->marks, "ragged_to_sparse_offsets", s, n_rows, RaggedRowLen{b, e, st}, RowOffsets{row_b, row_e, 0},
                (SparseFin<int32_t>{st, (long long)std::min<int64_t>(capacity, INT32_MAX - 1), (long long)n_rows, 0u, nullptr}), ws->tiles.as<long long>(), st, 0u);
    OVTK_LAUNCH(ws->marks, "ragged_to_sparse", each_wave_kernel<SparseRows<int32_t>>, wave_grid, kTileThreads, s, (long long)n_rows,
                (SparseRows<int32_t>{row_b, row_e, d_out, nullptr, nullptr, nullptr}), (const RunStatus*)st, kFlagRange | kFlagOutCapacity);
    if (int rc = finish_status(*ws.ws, s)) return rc;
    const uint32_t f = ws->host_status->flags;
    if (f & kFlagRange) return set_error(OVTK_E_RANGE, "ragged_to_sparse: a row ends before it begins");
    *n_out = ws->host_status->n_out;
    if (f & kFlagOutCapacity)
        return set_error(OVTK_E_CAPACITY, "RaggedToSparse: output buffer too small (" + std::to_string(*n_out) + " pairs, capacity " + std::to_string(capacity) + ")");
    if (int rc = copy_back(out, d_out, size_t(*n_out) * 8, mem, s)) return rc;
    if (mem == OVTK_MEM_HOST) OVTK_HIP(hipStreamSynchronize(s));
    return OVTK_OK;
}

}  // extern "C"
