// sp_model_fuzz.cpp -- feeds csrc/sp_model.hpp (the reader of untrusted sentencepiece ModelProto bytes) every fixture model, every
// truncation of it at every length, and the same with one byte flipped here and there; under AddressSanitizer and UBSan a read past
// the end of the buffer or an overflow stops the program.  Each input is copied into a heap block of exactly its length, so the
// sanitizer sees the true end.  Host code only; nothing here touches a GPU.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I openvino_tokenizers_amd/csrc \
//       tools/sp_model_fuzz.cpp -o /tmp/sp_model_fuzz
//   /tmp/sp_model_fuzz tests/golden/spm_unigram_nfkc.model tests/golden/spm_unigram_bytes.model tests/golden/spm_unigram_edit.model \
//       tests/golden/spm_refuse_bpe.model tests/golden/spm_detok_*.model
// Every model is also run with a trainer_spec that holds unk_surface and a denormalizer_spec that holds a charsmap appended (protobuf
// merges a repeated sub-message), cut at every length of the appended part: the fields SentencepieceDetokenizer reads.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>

#include "sp_model.hpp"

static bool parse_exact(const uint8_t* data, size_t len, ovtk::SpModel& m) {
    std::unique_ptr<uint8_t[]> block(new uint8_t[len ? len : 1]);
    if (len) std::memcpy(block.get(), data, len);
    return ovtk::sp_model_parse(block.get(), len, m);
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s model...\n", argv[0]);
        return 2;
    }
    for (int a = 1; a < argc; ++a) {
        std::ifstream f(argv[a], std::ios::binary);
        std::vector<uint8_t> data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (data.empty()) {
            std::fprintf(stderr, "%s: cannot read\n", argv[a]);
            return 2;
        }
        ovtk::SpModel whole;
        if (!parse_exact(data.data(), data.size(), whole) || whole.pieces.empty()) {
            std::fprintf(stderr, "%s: the whole model does not parse\n", argv[a]);
            return 1;
        }
        size_t ok = 0, bad = 0;
        for (size_t len = 0; len < data.size(); ++len) {   // every truncation
            ovtk::SpModel m;
            (parse_exact(data.data(), len, m) ? ok : bad) += 1;
        }
        uint32_t x = 12345;
        for (int k = 0; k < 4000; ++k) {   // a byte flipped, then cut
            x = x * 1664525u + 1013904223u;
            std::vector<uint8_t> d(data.begin(), data.begin() + std::min<size_t>(data.size(), 16384));
            d[(x >> 8) % d.size()] ^= uint8_t(1u << (x & 7));
            x = x * 1664525u + 1013904223u;
            ovtk::SpModel m;
            (parse_exact(d.data(), (x >> 4) % (d.size() + 1), m) ? ok : bad) += 1;
        }
        // the detokenizer's fields: trainer_spec.unk_surface (44) and denormalizer_spec (5) .precompiled_charsmap (2), appended
        static const uint8_t tail[] = {0x12, 0x06, 0xE2, 0x02, 0x03, '<', '?', '>',                          // trainer_spec { 44: "<?>" }
                                       0x2A, 0x09, 0x12, 0x03, 'a', 'b', 'c', 0x18, 0x01, 0x20, 0x00};       // denormalizer_spec { 2: "abc", 3: 1, 4: 0 }
        std::vector<uint8_t> grown(data);
        grown.insert(grown.end(), tail, tail + sizeof tail);
        ovtk::SpModel g;
        if (!parse_exact(grown.data(), grown.size(), g) || !g.has_unk_surface || g.unk_surface != "<?>" || g.denormalizer_charsmap != "abc" ||
            g.pieces.size() != whole.pieces.size()) {
            std::fprintf(stderr, "%s: the appended unk_surface / denormalizer_spec were not read\n", argv[a]);
            return 1;
        }
        for (size_t len = data.size(); len < grown.size(); ++len) {   // every truncation of the appended fields
            ovtk::SpModel m;
            (parse_exact(grown.data(), len, m) ? ok : bad) += 1;
        }
        for (size_t at = data.size(); at < grown.size(); ++at)        // ... and every one of their bytes flipped
            for (int bit = 0; bit < 8; ++bit) {
                std::vector<uint8_t> d2(grown);
                d2[at] ^= uint8_t(1u << bit);
                ovtk::SpModel m;
                (parse_exact(d2.data(), d2.size(), m) ? ok : bad) += 1;
            }
        std::printf("%s: unk_surface %s, denormalizer charsmap %zu bytes\n", argv[a], whole.has_unk_surface ? whole.unk_surface.c_str() : "(absent)",
                    whole.denormalizer_charsmap.size());
        std::printf("%s: %zu pieces, model_type %d, charsmap %zu bytes; %zu inputs parsed, %zu refused\n", argv[a], whole.pieces.size(),
                    whole.model_type, whole.precompiled_charsmap.size(), ok, bad);
    }
    return 0;
}
