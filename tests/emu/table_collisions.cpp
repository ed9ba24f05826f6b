// tests/emu/table_collisions.cpp -- finds the inputs on which the device hash tables of csrc/tables.hpp COLLIDE, builds each table with the
// project's own builders (tables.cpp is linked, nothing of it is restated here) and prints one JSON document: per case the inputs and the
// structural facts that make the case what it is (slots, chain lengths, wraps, overflowing buckets, stored / refused).
//
// TEST INFRASTRUCTURE ONLY, pure host code (make -C openvino_tokenizers_amd/csrc collisions).  tests/gen_golden_table_collisions.py writes the
// output to tests/golden/table_collisions.json; tests/test_table_collisions.py runs it again and compares (a changed hash constant must not
// quietly turn the cases into ordinary inputs) and feeds the cases to the ops.
//
// Every search is deterministic: sizes ascending, seeds ascending, the first hit is taken.  What a search may assume about a hash function
// it checks with the function itself before it reports.
//
// BPE vocabularies are synthetic: base token i is four lower-case letters (i in base 26, most significant first), a merged token is the
// concatenation of its halves and sits at a spare id behind the base tokens.  Every merge is then legal for build_bpe, and a piece made
// of base tokens reaches the merge table with exactly the (left id, right id) pairs the case names.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/ovtk_amd.h"
#include "tables.hpp"

using namespace ovtk;

namespace {

constexpr int64_t kCacheCapacity = 64;   // the cache_capacity the memo cases are sized for (tests pass the same value)

struct Strs {
    std::vector<int32_t> b, e;
    std::vector<uint8_t> c;
    void add(const std::string& s) {
        b.push_back(int32_t(c.size()));
        c.insert(c.end(), s.begin(), s.end());
        e.push_back(int32_t(c.size()));
    }
    StringsView view() const { return StringsView{b.data(), e.data(), c.data(), int64_t(b.size())}; }
};

uint64_t g_rng;
uint64_t rnd() {   // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

std::string base_tok(uint32_t i) {
    std::string s(4, 'a');
    for (int k = 3; k >= 0; --k, i /= 26) s[size_t(k)] = char('a' + i % 26);
    return s;
}
std::string hex(const std::string& s) {
    static const char* d = "0123456789abcdef";
    std::string o;
    for (unsigned char ch : s) { o += d[ch >> 4]; o += d[ch & 15]; }
    return o;
}
std::string jhexs(const std::vector<std::string>& v) {
    std::string o = "[";
    for (size_t i = 0; i < v.size(); ++i) o += (i ? ", \"" : "\"") + hex(v[i]) + "\"";
    return o + "]";
}
template <class T>
std::string jnums(const std::vector<T>& v) {
    std::string o = "[";
    for (size_t i = 0; i < v.size(); ++i) o += (i ? ", " : "") + std::to_string(v[i]);
    return o + "]";
}
typedef std::pair<uint32_t, uint32_t> LR;
std::string jpairs(const std::vector<LR>& v) {
    std::string o = "[";
    for (size_t i = 0; i < v.size(); ++i) o += std::string(i ? ", " : "") + "[" + std::to_string(v[i].first) + ", " + std::to_string(v[i].second) + "]";
    return o + "]";
}
std::string jstr(const std::string& s) {
    std::string o = "\"";
    for (char ch : s) { if (ch == '"' || ch == '\\') o += '\\'; o += ch; }
    return o + "\"";
}
[[noreturn]] void die(const char* what) {
    std::fprintf(stderr, "table_collisions: %s\n", what);
    std::exit(2);
}

// ------------------------------------------------------------------------------------------------ BPE: the merge table
// n_base base tokens, then one merged token per merge at ids n_base, n_base + 1, ...
struct BpeCase {
    uint32_t n_base = 0;
    std::vector<LR> merges;
    BpeHost host;
    std::string err;
    int rc = 0;
    void build() {
        Strs vocab, left, right, none;
        for (uint32_t i = 0; i < n_base; ++i) vocab.add(base_tok(i));
        for (const LR& m : merges) {
            vocab.add(base_tok(m.first) + base_tok(m.second));
            left.add(base_tok(m.first));
            right.add(base_tok(m.second));
        }
        const StringsView r = right.view();
        host = BpeHost();
        rc = build_bpe(vocab.view(), left.view(), &r, none.view(), nullptr, "", "", false, host, err);
    }
    // slot of a key in the built table, or -1
    int64_t slot_of(uint64_t key) const {
        for (size_t i = 0; i < host.merges.size(); ++i)
            if (host.merges[i].s[0].kr != kEmptySlot && (host.merges[i].s[0].kr >> kMaxRankBits) == key) return int64_t(i);
        return -1;
    }
};

// The set of `want` merges with one merge_mix that needs the fewest ids (all below kIds; empty: there is none).  merge_mix_sum is linear in the key's fields: with
// A = merge_mix_sum(1) (odd), g(l) = merge_mix_sum(merge_key(l, 0)) / A, the sum of (l, r) is A * (g(l) + r) -- so left ids whose g lie
// within a window narrower than the vocabulary collide for right ids that make up the differences.  The completeness of the search rests
// on that; the set it reports is checked with merge_mix itself, and so are the slots (a set whose two candidate slots coincide in a table of
// 2^26 cannot be placed at all and is passed over).
std::vector<LR> equal_mix_set_below(size_t want, uint32_t kIds, uint32_t& v_out) {
    const uint32_t A = merge_mix_sum(1);
    uint32_t inv = A;   // Newton: five steps double 3 correct bits to 32 and more
    for (int k = 0; k < 5; ++k) inv *= 2u - A * inv;
    if (A * inv != 1u) die("merge_mix_sum(1) is even");
    std::vector<std::pair<uint32_t, uint32_t>> g;   // (g(l), l)
    for (uint32_t l = 0; l < kIds; ++l) g.emplace_back(merge_mix_sum(merge_key(l, 0)) * inv, l);
    std::sort(g.begin(), g.end());
    uint32_t best_v = 0;
    std::vector<LR> best;
    for (size_t i = 0; i < g.size(); ++i) {
        // the left ids whose g is at most 65 535 above g[i] (going round the end of the 32-bit range)
        std::vector<std::pair<uint32_t, uint32_t>> win;   // (distance, l)
        for (size_t j = (i + 1) % g.size(); j != i && uint32_t(g[j].first - g[i].first) < kIds; j = (j + 1) % g.size())
            win.emplace_back(g[j].first - g[i].first, g[j].second);
        if (win.size() + 1 < want) continue;
        // g[i] and every choice of want - 1 of the others (want is 2 or 3); the member with the largest g takes right id 0
        for (size_t a = 0; a < win.size(); ++a)
            for (size_t b = (want == 3 ? a + 1 : a); b < (want == 3 ? win.size() : a + 1); ++b) {
                for (uint32_t t = 0; t < 2; ++t) {   // (all right ids one up: another mix, one more id perhaps)
                    const uint32_t top = std::max(win[a].first, win[b].first) + t;
                    std::vector<LR> set{LR{g[i].second, top}, LR{win[a].second, top - win[a].first}};
                    if (want == 3) set.push_back(LR{win[b].second, top - win[b].first});
                    uint32_t need = 0;
                    for (const LR& m : set) need = std::max(need, std::max(m.first, m.second) + 1);
                    const uint64_t key = merge_key(set[0].first, set[0].second);
                    if (need > kIds || merge_h1(key, 6) == merge_h2(key, 6)) continue;
                    if (best.empty() || need < best_v) { best = set; best_v = need; }
                }
            }
    }
    if (best.empty()) return best;
    std::sort(best.begin(), best.end());
    for (const LR& m : best)
        if (merge_mix(merge_key(m.first, m.second)) != merge_mix(merge_key(best[0].first, best[0].second))) die("equal_mix_set: not equal");
    v_out = best_v;
    return best;
}

// (ids below 65 536 first, then twice as many, up to what four letters number)
std::vector<LR> equal_mix_set(size_t want, uint32_t& v_out) {
    for (uint32_t ids = 65536; ids <= 26 * 26 * 26 * 26; ids *= 2) {
        const std::vector<LR> set = equal_mix_set_below(want, ids, v_out);
        if (!set.empty()) return set;
    }
    die("no set of merges with one merge_mix among 456 976 ids");
}

std::string merge_cases() {
    std::string o = "  \"merge\": {\n";
    // (a) two merges, one mix: both placed, one in each slot
    {
        BpeCase c;
        c.merges = equal_mix_set(2, c.n_base);
        c.build();
        if (c.rc) die(("case a: build_bpe failed: " + c.err + " n_base " + std::to_string(c.n_base) + " " + jpairs(c.merges)).c_str());
        const uint64_t k0 = merge_key(c.merges[0].first, c.merges[0].second), k1 = merge_key(c.merges[1].first, c.merges[1].second);
        const uint32_t h1 = merge_h1(k0, c.host.bucket_shift), h2 = merge_h2(k0, c.host.bucket_shift);
        const int64_t s0 = c.slot_of(k0), s1 = c.slot_of(k1);
        if (s0 < 0 || s1 < 0 || s0 == s1 || (s0 != h1 && s0 != h2) || (s1 != h1 && s1 != h2)) die("case a: not one in each slot");
        // pairs that are no merges: the same two with the right id beside theirs, with their right ids exchanged, and pairs of small ids
        // that land on one of the two occupied slots
        auto beside = [&](uint32_t r) { return r + 1 < c.n_base ? r + 1 : r - 1; };
        std::vector<LR> absent{LR{c.merges[0].first, beside(c.merges[0].second)}, LR{c.merges[1].first, beside(c.merges[1].second)},
                               LR{c.merges[0].first, c.merges[1].second}, LR{c.merges[1].first, c.merges[0].second}};
        for (uint32_t l = 0; l < 512 && absent.size() < 8; ++l)
            for (uint32_t r = 0; r < 512 && absent.size() < 8; ++r) {
                const uint64_t k = merge_key(l, r);
                const uint32_t a = merge_h1(k, c.host.bucket_shift), b = merge_h2(k, c.host.bucket_shift);
                if (a == h1 || a == h2 || b == h1 || b == h2) absent.push_back(LR{l, r});
            }
        o += "    \"a\": {\"n_base\": " + std::to_string(c.n_base) + ", \"merges\": " + jpairs(c.merges) + ", \"mix\": " + std::to_string(merge_mix(k0)) +
             ", \"buckets\": " + std::to_string(c.host.merges.size()) + ", \"candidate_slots\": " + jnums(std::vector<uint32_t>{h1, h2}) +
             ", \"slots\": " + jnums(std::vector<int64_t>{s0, s1}) + ", \"kicks\": " + std::to_string(c.host.merge_kicks) + ", \"absent\": " + jpairs(absent) + "},\n";
    }
    // (b) the smallest random set of merges whose build evicts: sizes ascending, seeds ascending
    {
        bool found = false;
        for (uint32_t n = 3; n <= 48 && !found; ++n)
            for (uint64_t seed = 0; seed < 64 && !found; ++seed) {
                g_rng = 0xB000 + seed * 1000 + n;
                BpeCase c;
                c.n_base = 16;
                std::set<LR> seen;
                while (c.merges.size() < n) {
                    const LR m{uint32_t(rnd() % 16), uint32_t(rnd() % 16)};
                    if (seen.insert(m).second) c.merges.push_back(m);
                }
                c.build();
                if (c.rc) die("case b: build_bpe failed");
                if (c.host.merge_kicks == 0) continue;
                for (const LR& m : c.merges)
                    if (c.slot_of(merge_key(m.first, m.second)) < 0) die("case b: a merge is not in the table");
                std::vector<LR> absent;
                for (uint32_t l = 0; l < 16 && absent.size() < 12; ++l)
                    for (uint32_t r = 0; r < 16 && absent.size() < 12; ++r)
                        if (!seen.count(LR{l, r})) absent.push_back(LR{l, r});
                o += "    \"b\": {\"n_base\": 16, \"seed\": " + std::to_string(seed) + ", \"merges\": " + jpairs(c.merges) + ", \"buckets\": " +
                     std::to_string(c.host.merges.size()) + ", \"kicks\": " + std::to_string(c.host.merge_kicks) + ", \"absent\": " + jpairs(absent) + "},\n";
                found = true;
            }
        if (!found) die("case b: no set of merges needed a kick");
    }
    // (c) three merges, one mix: no table holds them.  Two other merges stand between them, so the message has indices to get right.
    {
        BpeCase c;
        const std::vector<LR> t = equal_mix_set(3, c.n_base);
        c.merges = {LR{0, 1}, t[0], LR{2, 3}, t[1], t[2]};
        c.build();
        o += "    \"c\": {\"n_base\": " + std::to_string(c.n_base) + ", \"vocab_size\": " + std::to_string(c.n_base + c.merges.size()) + ", \"merges\": " +
             jpairs(c.merges) + ", \"triple\": [1, 3, 4], \"mix\": " + std::to_string(merge_mix(merge_key(t[0].first, t[0].second))) +
             ", \"left_high_words\": " + jnums(std::vector<uint64_t>{merge_key(t[0].first, 0) >> 32, merge_key(t[1].first, 0) >> 32, merge_key(t[2].first, 0) >> 32}) +
             ", \"rc\": " + std::to_string(c.rc) + ", \"unsupported\": " + (c.rc == OVTK_E_UNSUPPORTED ? "true" : "false") + ", \"message\": " + jstr(c.err) + "}\n";
    }
    return o + "  }";
}

// ------------------------------------------------------------------------------------------------ the piece memo
// The key halves of a piece as build_piece_table makes them (the bytes, zero padded, the length in the last one).
void piece_key(const std::string& s, uint64_t& k0, uint64_t& k1) {
    uint8_t kb[16] = {0};
    std::memcpy(kb, s.data(), s.size());
    kb[15] = uint8_t(s.size());
    std::memcpy(&k0, kb, 8);
    std::memcpy(&k1, kb + 8, 8);
}
uint32_t piece_mix_of(const std::string& s) {
    uint64_t k0, k1;
    piece_key(s, k0, k1);
    return piece_mix(k0, k1);
}
// The table build_memo would make of a vocabulary in which every token encodes to its own id (true of the vocabularies below: a token
// is a base token, or the one merge of two base tokens).
void memo_table(const std::vector<std::string>& vocab, PieceTableHost& out) {
    Strs v;
    std::vector<int32_t> ib, ie, ids;
    for (size_t i = 0; i < vocab.size(); ++i) {
        v.add(vocab[i]);
        ib.push_back(int32_t(i));
        ie.push_back(int32_t(i + 1));
        ids.push_back(int32_t(i));
    }
    build_piece_table(v.view(), ib.data(), ie.data(), ids.data(), out, size_t(kCacheCapacity), true);
}
bool slot_holds(const PieceTableHost& t, const std::string& s) {
    uint64_t k0, k1;
    piece_key(s, k0, k1);
    const PieceEntry& e = t.slots[piece_h(piece_mix(k0, k1), t.shift)];
    return e.k0 == k0 && e.k1 == k1;
}
std::string jmerges(const std::vector<std::pair<std::string, std::string>>& m) {
    std::string o = "[";
    for (size_t i = 0; i < m.size(); ++i) o += std::string(i ? ", " : "") + "[\"" + hex(m[i].first) + "\", \"" + hex(m[i].second) + "\"]";
    return o + "]";
}
// X and Y, two strings of eight lower-case letters in one slot (same_mix: with all 32 bits of piece_mix equal), each the merge of its two
// halves.  Two handles over the base tokens aaaa .. aaad + the four halves:
//   fixed    the vocabulary also holds X and Y (merges (x1, x2), (y1, y2)): build_piece_table stores X and refuses Y
//   learned  it holds aaaaaaaa and aaabaaab instead: X and Y are pieces of two ids, whichever the device merges first takes the (free)
//            slot, the other is refused by memo_insert
// The search: random strings (a fixed seed), sorted by mix, the first neighbours that qualify.
std::string memo_case(const char* name, bool same_mix, bool last) {
    g_rng = same_mix ? 0xE0E0 : 0xD0D0;
    const size_t n = same_mix ? 600000 : 4000;
    std::vector<std::pair<uint32_t, std::string>> all;
    for (size_t i = 0; i < n; ++i) {
        std::string w(8, 'a');
        uint64_t v = rnd();
        for (int k = 0; k < 8; ++k, v /= 26) w[size_t(k)] = char('a' + v % 26);
        all.emplace_back(piece_mix_of(w), w);
    }
    std::sort(all.begin(), all.end());
    const std::vector<std::string> base{base_tok(0), base_tok(1), base_tok(2), base_tok(3)};
    for (size_t i = 0; i + 1 < all.size(); ++i) {
        const size_t j = i + 1;
        const std::string X = all[i].second, Y = all[j].second;
        if (X == Y) continue;
        std::vector<std::string> common = base;
        for (const std::string& h : {X.substr(0, 4), X.substr(4), Y.substr(0, 4), Y.substr(4)})
            if (std::find(common.begin(), common.end(), h) == common.end()) common.push_back(h);
        if (common.size() != 8) continue;   // (halves that repeat: another pair)
        std::vector<std::string> vf = common, vl = common;
        vf.push_back(X);
        vf.push_back(Y);
        vl.push_back(base[0] + base[0]);
        vl.push_back(base[1] + base[1]);
        PieceTableHost fixed, learned;
        memo_table(vf, fixed);
        memo_table(vl, learned);
        if (fixed.shift != learned.shift) die("memo: the two handles' tables differ in size");
        const uint32_t slot = piece_h(all[i].first, fixed.shift);
        const bool hit = piece_h(all[j].first, fixed.shift) == slot && (all[i].first == all[j].first) == same_mix;
        if (!hit) continue;
        if (learned.slots[slot].k1 != 0) continue;                      // a token of the learned handle's own sits there
        if (!slot_holds(fixed, X) || slot_holds(fixed, Y)) continue;    // (X itself refused: another token has the slot)
        // look-alikes: the halves crossed and swapped (pieces of two tokens, no merges)
        const std::vector<std::string> near{X.substr(0, 4) + Y.substr(4), Y.substr(0, 4) + X.substr(4), X.substr(4) + X.substr(0, 4), Y.substr(4) + Y.substr(0, 4)};
        return std::string("    \"") + name + "\": {\"cache_capacity\": " + std::to_string(kCacheCapacity) + ", \"x_hex\": \"" + hex(X) + "\", \"y_hex\": \"" + hex(Y) +
               "\", \"mix_x\": " + std::to_string(all[i].first) + ", \"mix_y\": " + std::to_string(all[j].first) + ", \"tag_x\": " + std::to_string(piece_tag(all[i].first, 1)) +
               ", \"tag_y\": " + std::to_string(piece_tag(all[j].first, 1)) + ", \"slots\": " + std::to_string(fixed.slots.size()) + ", \"slot\": " + std::to_string(slot) +
               ", \"fixed\": {\"vocab\": " + jhexs(vf) + ", \"merges\": " + jmerges({{X.substr(0, 4), X.substr(4)}, {Y.substr(0, 4), Y.substr(4)}}) + ", \"stored\": " +
               std::to_string(fixed.stored) + ", \"refused\": " + std::to_string(fixed.refused) + ", \"x_stored\": true, \"y_refused\": true}" +
               ", \"learned\": {\"vocab\": " + jhexs(vl) + ", \"merges\": " + jmerges({{base[0], base[0]}, {base[1], base[1]}}) + ", \"stored\": " + std::to_string(learned.stored) +
               ", \"refused\": " + std::to_string(learned.refused) + ", \"slot_free\": true}, \"near\": " + jhexs(near) + "}" + (last ? "\n" : ",\n");
    }
    die("memo: no pair found");
}

// ------------------------------------------------------------------------------------------------ VocabEncoder's string map
struct MapFacts {
    StringMapHost host;
    std::vector<uint32_t> home, slot;   // per key
};
MapFacts build_map(const std::vector<std::string>& keys) {
    MapFacts f;
    Strs k;
    for (const auto& s : keys) k.add(s);
    std::string err;
    if (build_string_map(k.view(), f.host, err)) die("build_string_map failed");
    for (size_t i = 0; i < keys.size(); ++i) {
        f.home.push_back(hash_bytes(reinterpret_cast<const uint8_t*>(keys[i].data()), int(keys[i].size())) & f.host.mask);
        uint32_t at = ~0u;
        for (uint32_t s = 0; s <= f.host.mask; ++s)
            if (f.host.slots[s] != kEmptySlot && uint32_t(f.host.slots[s]) == uint32_t(i)) at = s;
        if (at == ~0u) die("string map: a key is missing");
        f.slot.push_back(at);
    }
    return f;
}
uint32_t hb(const std::string& s) { return hash_bytes(reinterpret_cast<const uint8_t*>(s.data()), int(s.size())); }
std::string key_n(const char* stem, uint32_t i) { return std::string(stem) + std::to_string(i); }

// four keys with one home slot in a map of four keys (16 slots); wrap: the home slot is the last one
std::string map_chain_case(const char* name, bool wrap) {
    const uint32_t mask = 15;
    for (uint32_t home = 0; home <= mask; ++home) {
        if (wrap ? home != mask : home + 4 > mask) continue;
        std::vector<std::string> keys, absent;
        for (uint32_t i = 0; i < 4000 && (keys.size() < 4 || absent.size() < 4); ++i) {
            const std::string k = key_n("key", i);
            if ((hb(k) & mask) != home) continue;
            if (keys.size() < 4) keys.push_back(k);
            else absent.push_back(k);
        }
        // absent keys whose home is inside the chain, not at its head
        for (uint32_t i = 0; i < 4000 && absent.size() < 7; ++i) {
            const std::string k = key_n("mid", i);
            const uint32_t d = ((hb(k) & mask) - home) & mask;
            if (d >= 1 && d <= 3) absent.push_back(k);
        }
        if (keys.size() < 4) continue;
        const MapFacts f = build_map(keys);
        if (f.host.mask != mask) die("string map: unexpected size");
        bool wrapped = false;
        for (size_t i = 0; i < 4; ++i) {
            if (f.home[i] != home || f.slot[i] != ((home + i) & mask)) die("string map: not a chain");
            wrapped |= f.slot[i] < home;
        }
        if (wrapped != wrap) die("string map: wrap");
        return std::string("    \"") + name + "\": {\"keys\": " + jhexs(keys) + ", \"mask\": " + std::to_string(mask) + ", \"home\": " + std::to_string(home) +
               ", \"slots\": " + jnums(f.slot) + ", \"chain_length\": 4, \"wrap\": " + (wrap ? "true" : "false") + ", \"absent\": " + jhexs(absent) + "},\n";
    }
    die("string map: no chain");
}
// pairs of 8-byte keys (any byte values) with one 32-bit hash_bytes: random keys until two pairs are there (a birthday search)
std::string map_full_hash_case() {
    g_rng = 0x4A5B;
    std::vector<std::pair<uint32_t, std::string>> all;
    for (int i = 0; i < 400000; ++i) {
        std::string k(8, '\0');
        const uint64_t v = rnd();
        std::memcpy(&k[0], &v, 8);
        all.emplace_back(hb(k), k);
    }
    std::sort(all.begin(), all.end());
    std::vector<std::pair<std::string, std::string>> pairs;
    for (size_t i = 0; i + 1 < all.size() && pairs.size() < 2; ++i)
        if (all[i].first == all[i + 1].first && all[i].second != all[i + 1].second) { pairs.emplace_back(all[i].second, all[i + 1].second); ++i; }
    if (pairs.size() < 2) die("string map: no two keys with one hash");
    // the map holds both keys of the first pair and ONE of the second: its partner is absent and shares all 32 bits with a present key
    const std::vector<std::string> keys{pairs[0].first, pairs[0].second, pairs[1].first, "filler"};
    const MapFacts f = build_map(keys);
    if (hb(keys[0]) != hb(keys[1]) || hb(pairs[1].second) != hb(keys[2])) die("string map: hashes differ");
    if (f.home[0] != f.home[1] || f.slot[0] == f.slot[1]) die("string map: the pair does not share a chain");
    return "    \"h\": {\"keys\": " + jhexs(keys) + ", \"mask\": " + std::to_string(f.host.mask) + ", \"hashes\": " +
           jnums(std::vector<uint32_t>{hb(keys[0]), hb(keys[1]), hb(keys[2]), hb(keys[3])}) + ", \"slots\": " + jnums(f.slot) + ", \"absent\": " +
           jhexs({pairs[1].second}) + ", \"absent_hash\": " + std::to_string(hb(pairs[1].second)) + "}\n";
}

// ------------------------------------------------------------------------------------------------ the two trie forms
// a random vocabulary: every letter of the alphabet (TrieTokenizer needs a token at every position) + n words of 2..5 letters
std::vector<std::string> random_vocab(uint64_t seed, const std::string& alphabet, uint32_t n, const char* prefix_some = nullptr) {
    g_rng = seed;
    std::vector<std::string> v;
    std::set<std::string> seen;
    for (char ch : alphabet) { v.push_back(std::string(1, ch)); seen.insert(v.back()); }
    while (v.size() < alphabet.size() + n) {
        std::string w;
        const int len = 2 + int(rnd() % 4);
        for (int k = 0; k < len; ++k) w += alphabet[rnd() % alphabet.size()];
        if (prefix_some && rnd() % 2) w = prefix_some + w;
        if (seen.insert(w).second) v.push_back(w);
    }
    return v;
}

// the walk of TrieBucketsHost's table for one edge: buckets read, whether the walk wrapped; the child or -1
struct BucketStep { int child = -1; uint32_t home = 0, buckets_read = 0; bool wrapped = false, kids = false; int32_t value = -1; };
BucketStep bucket_step(const TrieBucketsHost& t, int node, uint8_t byte) {
    BucketStep s;
    const uint32_t key = (uint32_t(node) << 8) | byte;
    uint32_t bk = s.home = trie_bucket_of(uint32_t(node), byte, t.bucket_mask);
    for (;; bk = (bk + 1) & t.bucket_mask) {
        ++s.buckets_read;
        if (bk < s.home) s.wrapped = true;
        bool any_free = false;
        for (int j = 0; j < 4; ++j) {
            const uint32_t k = t.buckets[bk].kv[2 * j];
            if (k == kTrieFree) { any_free = true; continue; }
            if ((k & ~kTrieKids) == key) {
                s.child = int(4 * bk + uint32_t(j));
                s.kids = (k & kTrieKids) != 0;
                s.value = int32_t(t.buckets[bk].kv[2 * j + 1]);
                return s;
            }
        }
        if (any_free || s.buckets_read > t.bucket_mask + 1) return s;
    }
}
struct BucketFacts {
    uint32_t n_buckets = 0, full_buckets = 0;
    std::vector<std::string> crossing, wrapping, absent_past_full;   // strings whose walk reads a second bucket / wraps / misses behind a full bucket
    std::vector<uint32_t> overflowing;                               // home buckets of the edges that were sent on
};
BucketFacts bucket_facts(const std::vector<std::string>& vocab, const std::string& alphabet) {
    TrieHost th;
    for (size_t i = 0; i < vocab.size(); ++i) th.add(reinterpret_cast<const uint8_t*>(vocab[i].data()), vocab[i].size(), int32_t(i));
    th.finalize();
    TrieBucketsHost tb;
    if (!tb.build(th)) die("bucket trie: build failed");
    BucketFacts f;
    f.n_buckets = tb.bucket_mask + 1;
    for (const TrieBucket& b : tb.buckets) {
        bool full = true;
        for (int j = 0; j < 4; ++j) full &= b.kv[2 * j] != kTrieFree;
        f.full_buckets += full;
    }
    std::set<std::string> seen_absent;
    std::set<uint32_t> over;
    for (const std::string& w : vocab) {
        int node = kTrieRoot;
        bool crosses = false, wraps = false;
        for (size_t p = 0; p < w.size(); ++p) {
            // the edges this node does not have
            for (char ch : alphabet) {
                const BucketStep a = bucket_step(tb, node, uint8_t(ch));
                if (a.child < 0 && a.buckets_read >= 2) {
                    const std::string q = w.substr(0, p) + ch;
                    if (seen_absent.insert(q).second) f.absent_past_full.push_back(q);
                }
            }
            const BucketStep s = bucket_step(tb, node, uint8_t(w[p]));
            if (s.child < 0) die("bucket trie: a token's edge is missing");
            if (s.buckets_read >= 2) { crosses = true; over.insert(s.home); }
            wraps |= s.wrapped;
            node = s.child;
            if (p + 1 == w.size() && s.value == -1) die("bucket trie: a token has no value");
        }
        if (crosses) f.crossing.push_back(w);
        if (wraps) f.wrapping.push_back(w);
    }
    f.overflowing.assign(over.begin(), over.end());
    return f;
}
std::string bucket_case(const char* name, int which, bool last) {
    const std::string alphabet = "abcd";
    for (uint32_t n = 4; n <= 96; n += 2)
        for (uint64_t seed = 0; seed < 400; ++seed) {
            const std::vector<std::string> vocab = random_vocab(0x7000 + seed * 131 + n, alphabet, n);
            const BucketFacts f = bucket_facts(vocab, alphabet);
            const bool ok = which == 0 ? !f.crossing.empty() : which == 1 ? !f.wrapping.empty() : !f.absent_past_full.empty();
            if (!ok) continue;
            const std::vector<std::string> absent(f.absent_past_full.begin(), f.absent_past_full.begin() + std::min<size_t>(f.absent_past_full.size(), 8));
            return std::string("    \"") + name + "\": {\"seed\": " + std::to_string(seed) + ", \"words\": " + std::to_string(n) + ", \"vocab\": " + jhexs(vocab) +
                   ", \"n_buckets\": " + std::to_string(f.n_buckets) + ", \"full_buckets\": " + std::to_string(f.full_buckets) + ", \"overflowing_buckets\": " +
                   jnums(f.overflowing) + ", \"crossing\": " + jhexs(f.crossing) + ", \"wrapping\": " + jhexs(f.wrapping) + ", \"absent_past_full_bucket\": " +
                   jhexs(absent) + "}" + (last ? "\n" : ",\n");
        }
    die("bucket trie: no seed qualifies");
}

// The open-addressed TrieEdge table: per string of the vocabulary the longest probe chain on its path and whether one wrapped; absent
// edges whose probe passes two or more taken slots.
struct EdgeFacts {
    uint32_t capacity = 0, longest = 0;
    std::vector<std::string> chained, wrapping, absent;   // tokens whose path has a probe of >= 3 slots / a probe that wraps; absent: path + byte
};
void edge_facts(const TrieHost& t, const std::string& alphabet, EdgeFacts& f) {
    f.capacity = t.edge_mask + 1;
    auto probe = [&](uint32_t node, uint8_t byte, uint32_t& len, bool& wrapped) -> int {   // -> child or -1
        const uint32_t key = (node << 8) | byte;
        const uint32_t home = (hash_u32(key) >> t.edge_shift) & t.edge_mask;
        len = 0;
        wrapped = false;
        for (uint32_t idx = home;; idx = (idx + 1) & t.edge_mask) {
            ++len;
            if (idx < home) wrapped = true;
            if (t.edges[idx].key == kNoEdge) return -1;
            if (t.edges[idx].key == key) return t.edges[idx].child;
        }
    };
    // depth first from the root's children (the root's own edges are a direct table)
    struct Item { int node; std::string path; bool chained, wrapped; };
    std::vector<Item> stack;
    for (const auto& k : t.b.kids[0]) stack.push_back(Item{k.second, std::string(1, char(k.first)), false, false});
    while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        if (t.b.value[size_t(it.node)] != -1) {
            if (it.chained) f.chained.push_back(it.path);
            if (it.wrapped) f.wrapping.push_back(it.path);
        }
        for (char ch : alphabet) {
            uint32_t len;
            bool wrapped;
            const int child = probe(uint32_t(it.node), uint8_t(ch), len, wrapped);
            if (child < 0) {
                if (len >= 3 && f.absent.size() < 8) f.absent.push_back(it.path + ch);
                continue;
            }
            f.longest = std::max(f.longest, len);
            stack.push_back(Item{child, it.path + ch, it.chained || len >= 3, it.wrapped || wrapped});
        }
    }
    std::sort(f.chained.begin(), f.chained.end());
    std::sort(f.wrapping.begin(), f.wrapping.end());
}
std::string jedge(const EdgeFacts& f) {
    return "{\"capacity\": " + std::to_string(f.capacity) + ", \"longest_chain\": " + std::to_string(f.longest) + ", \"chained\": " + jhexs(f.chained) +
           ", \"wrapping\": " + jhexs(f.wrapping) + ", \"absent\": " + jhexs(f.absent) + "}";
}
std::string edge_cases() {
    std::string o = "  \"edge_trie\": {\n";
    const std::string alphabet = "abcd";
    // WordPiece: the root trie and the "##" trie of one vocabulary; (l) a probe chain of three or more slots, (m) one that wraps, in either
    for (int which = 0; which < 2; ++which) {
        bool found = false;
        for (uint32_t n = 6; n <= 400 && !found; n += 2)
            for (uint64_t seed = 0; seed < 200 && !found; ++seed) {
                const std::vector<std::string> vocab = random_vocab(0xE000 + seed * 77 + n, alphabet, n, "##");
                Strs v;
                for (const auto& w : vocab) v.add(w);
                TrieHost root, sub;
                std::string err;
                if (build_wordpiece(v.view(), "##", root, sub, err)) die("build_wordpiece failed");
                EdgeFacts fr, fs;
                edge_facts(root, alphabet, fr);
                edge_facts(sub, alphabet, fs);
                if (which == 0 ? (fr.chained.empty() && fs.chained.empty()) : (fr.wrapping.empty() && fs.wrapping.empty())) continue;
                o += std::string("    \"wordpiece_") + (which == 0 ? "l" : "m") + "\": {\"seed\": " + std::to_string(seed) + ", \"words\": " + std::to_string(n) + ", \"vocab\": " +
                     jhexs(vocab) + ", \"root\": " + jedge(fr) + ", \"sub\": " + jedge(fs) + "},\n";
                found = true;
            }
        if (!found) die("edge trie: no WordPiece vocabulary qualifies");
    }
    // BPE: the trie of n_base base tokens and one merge (0, 1), as build_bpe builds it
    bool found = false;
    for (uint32_t n_base = 8; n_base <= 4096 && !found; ++n_base) {
        BpeCase c;
        c.n_base = n_base;
        c.merges = {LR{0, 1}};
        c.build();
        if (c.rc) die("edge trie: build_bpe failed");
        EdgeFacts f;
        edge_facts(c.host.trie, "abcdefghijklmnopqrstuvwxyz", f);
        if (f.chained.empty() || f.wrapping.empty()) continue;
        o += "    \"bpe\": {\"n_base\": " + std::to_string(n_base) + ", \"merges\": " + jpairs(c.merges) + ", \"trie\": " + jedge(f) + "}\n";
        found = true;
    }
    if (!found) die("edge trie: no BPE vocabulary qualifies");
    return o + "  }";
}

}  // namespace

int main() {
    std::string o = "{\n";
    o += merge_cases() + ",\n";
    o += "  \"memo\": {\n" + memo_case("d", false, false) + memo_case("e", true, true) + "  },\n";
    o += "  \"string_map\": {\n" + map_chain_case("f", false) + map_chain_case("g", true) + map_full_hash_case() + "  },\n";
    o += "  \"bucket_trie\": {\n" + bucket_case("i", 0, false) + bucket_case("j", 1, false) + bucket_case("k", 2, true) + "  },\n";
    o += edge_cases() + "\n}\n";
    std::fputs(o.c_str(), stdout);
    return 0;
}
