// tools/sp_bpe_host_check.cpp -- the host side of SentencepieceTokenizer's BPE path (csrc/sp_bpe_tables.hpp: the refusals and the cut
// rule's proof condition) over the fixture models, every truncation of them and bit-flipped copies.  Host code only; build and run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I openvino_tokenizers_amd/csrc \
//       -o /tmp/sp_bpe_host_check tools/sp_bpe_host_check.cpp && /tmp/sp_bpe_host_check tests/golden
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "sp_bpe_tables.hpp"

using namespace ovtk;

static std::vector<uint8_t> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// 0: not parsed, 1: refused, 2: accepted with cuts, 3: accepted without
static int judge(const std::vector<uint8_t>& data, std::string* why) {
    SpModel m;
    if (!sp_model_parse(data.data(), data.size(), m)) return 0;
    if (!sp_bpe_accepts(m, why)) return 1;
    return sp_bpe_cut_rule_holds(m) ? 2 : 3;
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : "tests/golden";
    const struct { const char* file; int want; } cases[] = {
        {"spm_bpe_bytes.model", 2}, {"spm_bpe_unk.model", 2}, {"spm_bpe_edit.model", 3},
        {"spm_bpe_refuse_unused.model", 1}, {"spm_bpe_refuse_tie.model", 1}, {"spm_refuse_bpe.model", 1},
    };
    int bad = 0;
    long tried = 0;
    for (const auto& c : cases) {
        const std::vector<uint8_t> data = slurp(dir + "/" + c.file);
        std::string why;
        const int got = data.empty() ? -1 : judge(data, &why);
        std::printf("%-32s %zu bytes -> %d (want %d) %s\n", c.file, data.size(), got, c.want, why.c_str());
        bad += got != c.want;
        if (data.size() > 20000) continue;   // (the nmt_nfkc charsmap: the small models cover the same code)
        for (size_t cut = 0; cut < data.size(); ++cut, ++tried) judge(std::vector<uint8_t>(data.begin(), data.begin() + long(cut)), &why);
        for (size_t k = 0; k < data.size(); ++k, ++tried) {
            std::vector<uint8_t> flipped = data;
            flipped[k] ^= uint8_t(1u << (k % 8));
            judge(flipped, &why);
        }
    }
    std::printf("%ld damaged copies judged; %d fixtures judged wrongly\n", tried, bad);
    return bad ? 1 : 0;
}
