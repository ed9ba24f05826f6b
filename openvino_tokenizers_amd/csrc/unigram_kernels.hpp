// unigram_kernels.hpp -- UnigramTokenizer (src/unigram_tokenizer.cpp:147-224, tokenize_into): the best path through the lattice of
// vocabulary tokens, scores added in float32, ties to the earliest start.
//
// What the reference does per string of n bytes (restated in tests/unigram_ref.py):
//   * a node per byte position 0..n, {token_id = unk_token_id, best_score = 0.0f, starts_at = -1} (:159);
//   * starts_at walks the string by CHARACTERS whose length is read off the lead byte's high nibble alone (:85-87, :168-171, :206),
//     cut to the bytes that are left; nothing is validated;
//   * from each start the trie is walked byte by byte (:173-195); every token that ends on the way is a candidate for the node at its
//     end, candidate = scores[id] + best_score[start] (one float32 addition), taken when the node is unset or candidate > best_score,
//     strictly (:185);
//   * no token of exactly the character's length at this start: the node one character on gets the unknown edge under the same rule
//     (:197-205), unk_score = min(scores) - 10 rounded once to float32 (:157);
//   * back-tracking from node n (:210-223): an id equal to unk_token_id that directly follows another such id is dropped, whatever
//     produced it; the list is reversed.
// byte_fallback and fuse_unk are stored by the reference and change nothing in evaluate(); they are accepted and ignored here too.
// This library's choices where the reference leaves the answer to its trie builder: a vocabulary string that occurs more than once
// answers with its LOWEST id; an empty vocabulary string never matches.  Non-finite scores are outside the contract.
//
// The forward pass has one true dependency, best_score along the string; the trie walks -- nearly all the memory traffic -- have none:
//   * unigram_edges_kernel, a lane per byte position of every string: the walk from that position through the bucketed trie
//     (tables.hpp: one 32-byte sector per step), what it finds filed as (length << 22 | id) in a list of kUniEdges entries -- one
//     32-byte sector per position.  Nothing here depends on scores.  A position that is PROVABLY no character start is not walked:
//     the bytes-to-swallow state is 0 behind three bytes below 0xC0 (or at the string's first byte) whatever it was before, so a
//     lane looks back up to kUniLookBack bytes for such an anchor and steps forward from it; without an anchor in reach the lane
//     walks anyway (the relaxation only ever reads the lists of true starts, which it finds by stepping itself).  A position with
//     more matches than the list holds marks its string for the left-over path.
//   * UniRelax (each_kernel), a lane per string: starts in ascending order, each start's edges pushed with a plain float add and >,
//     the winning (length, id) per node kept in the lattice (8 bytes per node, HBM; a lane reads back what it wrote itself);
//     then back-tracking with the rule above, ids written right-aligned into the string's staging stretch.  A string marked for the
//     left-over path walks the trie from every start itself, serially, instead of reading the lists: same pushes, same order.
//   * the rows' counts -> scan (the reference's running ragged_offset, :57-74) -> a wave per row gathers its strings' ids, 64 strings
//     at a time.
// No fmaf, no reassociation: a sum is `score + best`, compared with `>`.
#pragma once

#include "device_common.hpp"
#include "ops_kernels.hpp"
#include "tables.hpp"

namespace ovtk {

constexpr int kUniEdges = 7;                               // matches filed per position: a count word + 7 entries = one 32-byte sector
constexpr int kUniIdBits = 22;
constexpr uint32_t kUniIdMask = (1u << kUniIdBits) - 1;
constexpr uint32_t kUniUnkCode = kUniIdMask;               // an edge's id field: the unknown edge (vocabulary ids stay below it)
constexpr int kUniMaxTokenBytes = (1 << (32 - kUniIdBits)) - 1;   // 1 023: a length fits the bits above the id
constexpr uint32_t kUniUnset = 0xFFFFFFFFu;                // a node's edge before anything reached it (starts_at == -1)
constexpr int kUniLookBack = 16;

struct alignas(32) UniEdgeList {
    uint32_t n;
    uint32_t e[kUniEdges];   // length << 22 | id, lengths ascending
};
struct alignas(8) UniNode {
    float score;
    uint32_t edge;   // the winning edge INTO this node: length << 22 | id (kUniUnkCode: the unknown edge), or kUniUnset
};

struct UnigramDev {
    TrieBucketsDev trie;
    const float* scores;
    float unk_score;
    int32_t unk_token_id;
};

struct UniWork {
    const int32_t* ragged_begins;
    const int32_t* ragged_ends;
    const int32_t* begins;
    const int32_t* ends;
    const uint8_t* chars;
    long long n_rows, n_strings, n_chars;
    UnigramDev dev;
    RunStatus* status;
    long long* node_off;     // [n_strings] first node of the string's stretch (n + 1 nodes)
    int32_t* owner;          // [nodes] the string a node belongs to
    UniEdgeList* lists;      // [nodes]
    UniNode* nodes;          // [nodes]
    int32_t* ids;            // [nodes] a string's ids, right-aligned in front of its last node
    int32_t* str_cnt;        // [n_strings]
    int32_t* str_over;       // [n_strings] 1: some position has more matches than a list holds
    int32_t* row_len;        // [n_rows]
    long long cap;           // nodes the buffers hold

    // bytes of string s, -1 where its offsets leave the chars tensor (an error only if a row names the string)
    __device__ __forceinline__ int str_bytes(long long s) const {
        const long long b = begins[s], e = ends[s];
        return (b < 0 || e < b || e > n_chars) ? -1 : int(e - b);
    }
};

// src/unigram_tokenizer.cpp:85-87: "\1\1\1\1\1\1\1\1\1\1\1\1\2\2\3\4"[byte >> 4]
__device__ __forceinline__ int uni_char_len(uint32_t byte) { return byte < 0xC0 ? 1 : byte < 0xE0 ? 2 : byte < 0xF0 ? 3 : 4; }

// One step of the trie: the edge (cur, byte).  Returns false where there is none; else cur = the child, value = the token that ends
// there or -1, kids = whether anything goes on from it.
__device__ __forceinline__ bool uni_trie_step(const TrieBucketsDev& t, int& cur, uint32_t byte, int32_t& value, bool& kids) {
    const uint32_t key = (uint32_t(cur) << 8) | byte;
    uint32_t bk = trie_bucket_of(uint32_t(cur), byte, t.bucket_mask);
    for (;;) {
        const uint4* p = reinterpret_cast<const uint4*>(t.buckets + bk);
        const uint4 lo = p[0], hi = p[1];
        const uint32_t k[4] = {lo.x, lo.z, hi.x, hi.z};
        const uint32_t v[4] = {lo.y, lo.w, hi.y, hi.w};
        bool any_free = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if ((k[j] & ~kTrieKids) == key && k[j] != kTrieFree) {
                cur = int(4u * bk + uint32_t(j));
                value = int32_t(v[j]);
                kids = (k[j] & kTrieKids) != 0;
                return true;
            }
            any_free |= k[j] == kTrieFree;
        }
        if (any_free) return false;   // (a full bucket sends its surplus to the next one: tables.cpp TrieBucketsHost::build)
        bk = (bk + 1) & t.bucket_mask;
    }
}

// The walk from byte `from` of the string chars[b, b + n): found(length, id) for every token that ends on the way, lengths ascending.
// The text in 16-byte windows that start at the byte at hand (the text loads do not wait for the trie's).
template <class Found>
__device__ __forceinline__ void uni_walk(const UniWork& w, long long b, int n, int from, Found&& found) {
    int cur = kTrieRoot;
    uint64_t lo = 0, hi = 0;
    int wbase = from - 16;
    for (int i = from; i < n; ++i) {
        if (i - wbase >= 16) {
            wbase = i;
            const long long at = b + i;
            uint4 v;
            if (at + 16 > w.n_chars) {
                v = trie_window_tail(w.chars, w.n_chars, at);
            } else {
                const TrieBytes16 t = *reinterpret_cast<const TrieBytes16*>(w.chars + at);
                v = uint4{t.d[0], t.d[1], t.d[2], t.d[3]};
            }
            lo = uint64_t(v.x) | (uint64_t(v.y) << 32);
            hi = uint64_t(v.z) | (uint64_t(v.w) << 32);
        }
        const int k = i - wbase;
        const uint32_t byte = uint32_t(((k < 8 ? lo : hi) >> (8 * (k & 7))) & 0xFF);
        int32_t value = -1;
        bool kids = false;
        if (!uni_trie_step(w.dev.trie, cur, byte, value, kids)) return;
        if (value != -1) found(i + 1 - from, value);
        if (!kids) return;
    }
}

// Scan over the strings: a stretch of n + 1 nodes each.
struct UniStretch {
    UniWork w;
    __device__ long long operator()(long long s) const {
        const int n = w.str_bytes(s);
        return n < 0 ? 0 : n + 1;
    }
};
struct UniStretchApply {
    UniWork w;
    __device__ void operator()(long long s, long long off, long long len) const {
        w.node_off[s] = off;
        w.str_over[s] = 0;
        if (off + len > w.cap) return;   // (UniStretchFin raises the flag: the host grows the buffers and runs the call again)
        for (long long k = 0; k < len; ++k) w.owner[off + k] = int32_t(s);
    }
};
struct UniStretchFin {
    RunStatus* status;
    long long cap;
    __device__ void operator()(long long total) const {
        status->stage_need = total > INT32_MAX ? INT32_MAX : int32_t(total);
        if (total > cap) atomicOr(&status->flags, kFlagStageOverflow);
    }
};

// A lane per node: the node's lattice entry cleared, the matches that start at its byte filed.
static __global__ __launch_bounds__(kTileThreads) void unigram_edges_kernel(UniWork w) {
    if (w.status->flags & (kFlagRange | kFlagStageOverflow)) return;
    const long long g = (long long)blockIdx.x * kTileThreads + threadIdx.x;
    if (g >= w.status->stage_need) return;
    const long long s = w.owner[g];
    const int p = int(g - w.node_off[s]);
    const long long b = w.begins[s];
    const int n = int(w.ends[s] - b);
    w.nodes[g] = UniNode{0.0f, kUniUnset};
    if (p >= n) return;
    // a character start?  An anchor: the string's first byte, or a position behind three bytes that each stand for themselves.
    {
        const uint8_t* text = w.chars + b;
        int q = -1, run = 0, t = p - 1;
        for (; t >= 0 && p - t <= kUniLookBack; --t) {
            if (text[t] >= 0xC0) {
                run = 0;
            } else if (++run == 3) {
                q = t + 3;   // behind the three bytes t, t + 1, t + 2
                break;
            }
        }
        if (q < 0 && t < 0) q = 0;
        if (q >= 0) {
            while (q < p) q += uni_char_len(text[q]);
            if (q != p) return;   // inside a character: no token starts here, the relaxation never reads this list
        }
    }
    uint32_t e[kUniEdges];
#pragma unroll
    for (int k = 0; k < kUniEdges; ++k) e[k] = 0;
    int cnt = 0;
    bool over = false;
    uni_walk(w, b, n, p, [&](int len, int32_t id) {
        const uint32_t entry = (uint32_t(len) << kUniIdBits) | uint32_t(id);
        if (cnt >= kUniEdges) over = true;
#pragma unroll
        for (int k = 0; k < kUniEdges; ++k)
            if (k == cnt) e[k] = entry;
        ++cnt;
    });
    if (over) w.str_over[s] = 1;   // (every lane that finds one stores the same 1)
    uint4* dst = reinterpret_cast<uint4*>(w.lists + g);
    dst[0] = uint4{uint32_t(cnt < kUniEdges ? cnt : kUniEdges), e[0], e[1], e[2]};
    dst[1] = uint4{e[3], e[4], e[5], e[6]};
}

// A lane per string: relaxation in ascending order of starts, back-tracking, the string's ids and their count.
struct UniRelax {
    UniWork w;
    __device__ void operator()(long long s) const {
        const int n = w.str_bytes(s);
        if (n <= 0) {
            w.str_cnt[s] = 0;
            return;
        }
        const long long b = w.begins[s];
        const long long off = w.node_off[s];
        UniNode* nodes = w.nodes + off;
        const bool leftover = w.str_over[s] != 0;
        const float* scores = w.dev.scores;
        const float unk_score = w.dev.unk_score;
        int pos = 0;
        while (pos < n) {
            const int full = uni_char_len(w.chars[b + pos]);
            const int clen = full < n - pos ? full : n - pos;
            const float base = nodes[pos].score;
            bool found = false;
            auto push = [&](int len, uint32_t code) {
                const float cand = (code == kUniUnkCode ? unk_score : scores[code]) + base;
                const UniNode at = nodes[pos + len];
                if (at.edge == kUniUnset || cand > at.score) nodes[pos + len] = UniNode{cand, (uint32_t(len) << kUniIdBits) | code};
                if (len == clen && code != kUniUnkCode) found = true;
            };
            if (!leftover) {
                const uint4* src = reinterpret_cast<const uint4*>(w.lists + off + pos);
                const uint4 a = src[0], c = src[1];
                const uint32_t e[kUniEdges] = {a.y, a.z, a.w, c.x, c.y, c.z, c.w};
                const int cnt = int(a.x);
#pragma unroll
                for (int k = 0; k < kUniEdges; ++k)
                    if (k < cnt) push(int(e[k] >> kUniIdBits), e[k] & kUniIdMask);
            } else {
                uni_walk(w, b, n, pos, [&](int len, int32_t id) { push(len, uint32_t(id)); });
            }
            if (!found) push(clen, kUniUnkCode);
            pos += clen;
        }
        // src/unigram_tokenizer.cpp:210-223
        int32_t* ids = w.ids + off;
        const int32_t unk_id = w.dev.unk_token_id;
        int ends_at = n, cnt = 0;
        int32_t prev = -1;
        while (ends_at > 0) {
            const UniNode at = nodes[ends_at];
            if (at.edge == kUniUnset) break;   // (never: every start reaches the node one character on)
            const uint32_t code = at.edge & kUniIdMask;
            const int32_t id = code == kUniUnkCode ? unk_id : int32_t(code);
            ends_at -= int(at.edge >> kUniIdBits);
            if (id == unk_id && prev == unk_id) continue;
            ids[n - 1 - cnt] = id;
            ++cnt;
            prev = id;
        }
        w.str_cnt[s] = cnt;
    }
};

// A lane per row: the ids of the row's strings; offsets that leave their tensors raise kFlagRange here, where a row names them.
struct UniRowCount {
    UniWork w;
    __device__ void operator()(long long row) const {
        const long long cb = w.ragged_begins[row], ce = w.ragged_ends[row];
        long long sum = 0;
        bool bad = cb < 0 || ce < cb || ce > w.n_strings;
        if (!bad)
            for (long long col = cb; col < ce; ++col) {
                if (w.str_bytes(col) < 0) bad = true;
                else sum += w.str_cnt[col];
            }
        if (bad) atomicOr(&w.status->flags, kFlagRange);
        w.row_len[row] = bad ? 0 : int32_t(sum > INT32_MAX ? INT32_MAX : sum);
    }
};

// A wave per row: its strings' ids, one string after the other, to the row's place in the output.
struct UniGather {
    UniWork w;
    const int32_t* out_begins;
    int32_t* out_ids;
    __device__ void operator()(long long row) const {
        const long long cb = w.ragged_begins[row], ce = w.ragged_ends[row];
        int32_t* dst = out_ids + out_begins[row];
        const int l = lane_id();
        // 64 strings at a time, a lane each (strings are words: a few ids): the lanes' places from a prefix sum of their counts; a string
        // of many ids is copied by the whole wave
        for (long long col0 = cb; col0 < ce; col0 += kWave) {
            const long long col = col0 + l;
            const int cnt = col < ce ? w.str_cnt[col] : 0;
            const int32_t* src = cnt ? w.ids + w.node_off[col] + (w.str_bytes(col) - cnt) : nullptr;
            const int incl = wave_incl_sum(cnt);
            const bool big = cnt > 2 * kWave;
            if (!big)
                for (int k = 0; k < cnt; ++k) dst[incl - cnt + k] = src[k];
            unsigned long long bigs = __ballot(big);
            while (bigs) {
                const int from = __ffsll(bigs) - 1;
                bigs &= bigs - 1;
                const int c = wave_readlane(cnt, from);
                const int at = wave_readlane(incl, from) - c;
                const int32_t* s = w.ids + w.node_off[col0 + from] + (w.str_bytes(col0 + from) - c);
                for (int k = l; k < c; k += kWave) dst[at + k] = s[k];
            }
            dst += wave_readlane(incl, kWave - 1);
        }
    }
};

}  // namespace ovtk
