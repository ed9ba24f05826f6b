// sp_model.hpp -- the fields of a serialized SentencePiece ModelProto that SentencepieceTokenizer needs, read straight off the
// protobuf wire format (host code, no protobuf library, no HIP).  What sentencepiece_model.proto declares:
//   ModelProto      1 pieces (repeated message)   2 trainer_spec   3 normalizer_spec   5 denormalizer_spec (a NormalizerSpec)
//   SentencePiece   1 piece (string)   2 score (float)   3 type (enum, default NORMAL)
//   TrainerSpec     3 model_type (enum, default UNIGRAM)   24 treat_whitespace_as_suffix   35 byte_fallback
//                   40 unk_id (0)   41 bos_id (1)   42 eos_id (2)   44 unk_surface (" \xE2\x81\x87 ")   45 unk_piece   46 bos_piece ("<s>")   47 eos_piece ("</s>")
//   NormalizerSpec  2 precompiled_charsmap (bytes)   3 add_dummy_prefix   4 remove_extra_whitespaces   5 escape_whitespaces (all true)
// Absent fields keep the defaults above, the last occurrence of a scalar wins, a sub-message that occurs twice is merged, unknown
// fields are skipped by their wire type, an enum value the proto does not declare is dropped (proto2).  The bytes are untrusted:
// every read is checked against the end of the buffer first, a length that reaches past it, a varint of more than 10 bytes, a
// group tag or wire type 6 / 7 make the whole buffer malformed.  tools/sp_model_fuzz.cpp feeds it every truncation of the fixtures.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace ovtk {

enum SpPieceType : uint8_t { kSpNormal = 1, kSpUnknown = 2, kSpControl = 3, kSpUserDefined = 4, kSpUnused = 5, kSpByte = 6 };
enum SpModelType : int32_t { kSpUnigram = 1, kSpBpe = 2, kSpWord = 3, kSpChar = 4 };

struct SpPiece {
    std::string piece;
    float score = 0.0f;
    uint8_t type = kSpNormal;
};

struct SpModel {
    std::vector<SpPiece> pieces;
    // trainer_spec
    int32_t model_type = kSpUnigram;
    bool byte_fallback = false, treat_whitespace_as_suffix = false;
    int32_t unk_id = 0, bos_id = 1, eos_id = 2;
    std::string unk_piece = "<unk>", bos_piece = "<s>", eos_piece = "</s>";
    std::string unk_surface;        // what Decode writes for the unknown piece, if the field is present (has_unk_surface)
    bool has_unk_surface = false;
    // normalizer_spec
    std::string precompiled_charsmap;
    bool add_dummy_prefix = true, remove_extra_whitespaces = true, escape_whitespaces = true;
    // denormalizer_spec
    std::string denormalizer_charsmap;
};

namespace sp_wire {

struct Reader {
    const uint8_t* p;
    const uint8_t* end;
    bool varint(uint64_t& v) {
        v = 0;
        for (int shift = 0; shift < 70; shift += 7) {
            if (p >= end) return false;
            const uint8_t b = *p++;
            if (shift < 64) v |= uint64_t(b & 0x7F) << shift;
            if (!(b & 0x80)) return true;
        }
        return false;   // an eleventh byte
    }
    bool fixed(size_t n, uint64_t& v) {
        if (size_t(end - p) < n) return false;
        v = 0;
        for (size_t k = 0; k < n; ++k) v |= uint64_t(p[k]) << (8 * k);
        p += n;
        return true;
    }
    bool bytes(Reader& sub) {
        uint64_t len = 0;
        if (!varint(len) || len > uint64_t(end - p)) return false;
        sub = Reader{p, p + len};
        p += len;
        return true;
    }
};

// One message: f(field, wire type, value of a varint / fixed field, the bytes of a length-delimited one) -> false: malformed.
template <class F>
inline bool each_field(Reader r, F&& f) {
    while (r.p < r.end) {
        uint64_t tag = 0, v = 0;
        if (!r.varint(tag)) return false;
        const uint64_t field = tag >> 3;
        const int wt = int(tag & 7);
        if (field == 0 || field > 0x1FFFFFFFull) return false;
        Reader sub{nullptr, nullptr};
        switch (wt) {
        case 0: if (!r.varint(v)) return false; break;
        case 1: if (!r.fixed(8, v)) return false; break;
        case 2: if (!r.bytes(sub)) return false; break;
        case 5: if (!r.fixed(4, v)) return false; break;
        default: return false;   // groups (3, 4) are not part of this schema; 6 and 7 do not exist
        }
        if (!f(uint32_t(field), wt, v, sub)) return false;
    }
    return true;
}

inline std::string str_of(const Reader& r) { return std::string(reinterpret_cast<const char*>(r.p), size_t(r.end - r.p)); }

}  // namespace sp_wire

// false: the buffer is truncated or malformed (*why says where).  Never reads outside data[0, len).
inline bool sp_model_parse(const uint8_t* data, size_t len, SpModel& m, std::string* why = nullptr) {
    using namespace sp_wire;
    auto fail = [&](const char* what) {
        if (why) *why = what;
        return false;
    };
    if (len > 0 && !data) return fail("null buffer");
    bool sub_ok = true;
    const char* where = "ModelProto";
    const bool ok = each_field(Reader{data, data + len}, [&](uint32_t field, int wt, uint64_t, const Reader& sub) {
        if (wt != 2) return true;   // (every field read here is a message; a scalar under one of their numbers is an unknown field)
        if (field == 1) {
            SpPiece pc;
            sub_ok = each_field(sub, [&](uint32_t f, int w, uint64_t v, const Reader& s) {
                if (f == 1 && w == 2) pc.piece = str_of(s);
                else if (f == 2 && w == 5) {
                    const uint32_t bits = uint32_t(v);
                    std::memcpy(&pc.score, &bits, 4);
                } else if (f == 3 && w == 0) {
                    const int32_t t = int32_t(uint32_t(v));
                    if (t >= 1 && t <= 6) pc.type = uint8_t(t);
                }
                return true;
            });
            where = "a piece";
            m.pieces.push_back(std::move(pc));
        } else if (field == 2) {
            sub_ok = each_field(sub, [&](uint32_t f, int w, uint64_t v, const Reader& s) {
                if (w == 0) {
                    const int32_t i = int32_t(uint32_t(v));
                    if (f == 3) {
                        if (i >= 1 && i <= 4) m.model_type = i;
                    } else if (f == 24) m.treat_whitespace_as_suffix = v != 0;
                    else if (f == 35) m.byte_fallback = v != 0;
                    else if (f == 40) m.unk_id = i;
                    else if (f == 41) m.bos_id = i;
                    else if (f == 42) m.eos_id = i;
                } else if (w == 2) {
                    if (f == 44) {
                        m.unk_surface = str_of(s);
                        m.has_unk_surface = true;
                    } else if (f == 45) m.unk_piece = str_of(s);
                    else if (f == 46) m.bos_piece = str_of(s);
                    else if (f == 47) m.eos_piece = str_of(s);
                }
                return true;
            });
            where = "trainer_spec";
        } else if (field == 3) {
            sub_ok = each_field(sub, [&](uint32_t f, int w, uint64_t v, const Reader& s) {
                if (f == 2 && w == 2) m.precompiled_charsmap = str_of(s);
                else if (f == 3 && w == 0) m.add_dummy_prefix = v != 0;
                else if (f == 4 && w == 0) m.remove_extra_whitespaces = v != 0;
                else if (f == 5 && w == 0) m.escape_whitespaces = v != 0;
                return true;
            });
            where = "normalizer_spec";
        } else if (field == 5) {
            sub_ok = each_field(sub, [&](uint32_t f, int w, uint64_t, const Reader& s) {
                if (f == 2 && w == 2) m.denormalizer_charsmap = str_of(s);
                return true;
            });
            where = "denormalizer_spec";
        }
        return sub_ok;
    });
    if (!sub_ok) return fail(where);
    if (!ok) return fail("ModelProto");
    return true;
}

}  // namespace ovtk
