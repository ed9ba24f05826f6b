// sentencepiece_kernels.hpp -- SentencepieceTokenizer for unigram models (src/sentence_piece.cpp:188-350, 4-input form) and
// RaggedToSparse (src/ragged_to_sparse.cpp:27-47).
//
// What sentencepiece does per sentence (SentencePieceProcessor::Encode with extra options, unigram::Model::EncodeOptimized):
//   * the sentence is normalized whole (charsmap_kernels.hpp) and the best path is searched over the whole normalized text;
//   * the lattice is unigram_kernels.hpp's -- float32 sums, strict >, characters by the lead nibble, an unknown edge of
//     min_score - 10 where no piece is exactly the character -- with the piece types on top: a piece of type UNUSED is found by the
//     trie and skipped before anything else looks at it (no candidate, no "single node"); CONTROL, UNKNOWN and BYTE pieces are not in
//     the trie at all; min_score is taken over the NORMAL pieces (the host does that);
//   * as the ids come out: a piece that is unknown directly behind an unknown one is merged into it (one unk_id for the run); with
//     byte_fallback every unknown piece becomes the id of <0xHH> for each of its bytes instead and nothing is merged;
//   * bos in front, eos behind, or the row reversed.
//
//   * SpRelax (sp_relax_kernel), a lane per sentence: UniRelax with the type table; back-tracking hands the ids out last to first, so
//     they are stored downwards from the end of the sentence's staging stretch (upwards from its start for a reversed row); a
//     sentence of n normalized bytes has at most n ids, its stretch n + 3 entries.  The longest row: a wave maximum, one atomic per wave.
//   * the rows' counts -> scan (dense_shape from its last step) -> SparseRows, a wave per row: one vector store per (row, position)
//     pair -- 16 bytes with i64 indices, 8 with RaggedToSparse's i32 --, the values in coalesced dwords beside them.
#pragma once

#include "device_common.hpp"
#include "ops_kernels.hpp"
#include "unigram_kernels.hpp"

namespace ovtk {

constexpr uint8_t kSpTypeUnused = 5;   // ModelProto.SentencePiece.Type (sp_model.hpp)

struct SpDev {
    const uint8_t* types;       // [pieces]
    const int32_t* byte_ids;    // [256] the id of <0xHH>
    int32_t bos_id, eos_id;
    int byte_fallback, add_bos, add_eos, reverse;
};

// The staging stretch of sentence s: behind its nodes' offset, two entries more per sentence (bos, eos).
__device__ __forceinline__ long long sp_stage_base(const UniWork& w, long long s) { return w.node_off[s] + 2 * s; }

struct SpRelax {
    UniWork w;        // begins / ends / chars: the NORMALIZED sentences; ragged_* unused
    SpDev sp;
    long long* row_start;   // [n] where the sentence's ids start in w.ids
    int32_t* row_len;       // [n]

    __device__ int operator()(long long s) const {
        const int n = w.str_bytes(s);
        const long long base = sp_stage_base(w, s);
        int32_t* ids = w.ids + base;
        if (n <= 0) {   // sentencepiece: an empty normalized sentence has no pieces; the extra options still apply
            int cnt = 0;
            if (sp.add_bos) ids[cnt++] = sp.bos_id;
            if (sp.add_eos) ids[cnt++] = sp.eos_id;
            row_start[s] = base;
            row_len[s] = cnt;
            return cnt;
        }
        const long long b = w.begins[s];
        const long long off = w.node_off[s];
        UniNode* nodes = w.nodes + off;
        const bool leftover = w.str_over[s] != 0;
        const float* scores = w.dev.scores;
        const float unk_score = w.dev.unk_score;
        const uint8_t* types = sp.types;
        int pos = 0;
        while (pos < n) {
            const int full = uni_char_len(w.chars[b + pos]);
            const int clen = full < n - pos ? full : n - pos;
            const float base_score = nodes[pos].score;
            bool found = false;
            auto push = [&](int len, uint32_t code) {
                if (code != kUniUnkCode && types[code] == kSpTypeUnused) return;
                const float cand = (code == kUniUnkCode ? unk_score : scores[code]) + base_score;
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
        // the ids, last to first: downwards from the stretch's entry n (entry n + 1 is eos's), or upwards from entry 0 when reversed
        int lo = 0, hi = n + 1;
        auto emit = [&](int32_t id) {
            if (sp.reverse) ids[lo++] = id;
            else ids[--hi] = id;
        };
        const int32_t unk_id = w.dev.unk_token_id;
        int ends_at = n;
        bool prev_unk = false;
        while (ends_at > 0) {
            const UniNode at = nodes[ends_at];
            if (at.edge == kUniUnset) break;   // (never: every start reaches the node one character on)
            const uint32_t code = at.edge & kUniIdMask;
            const int len = int(at.edge >> kUniIdBits);
            const bool unk = code == kUniUnkCode;
            if (unk && sp.byte_fallback) {
                for (int k = ends_at - 1; k >= ends_at - len; --k) emit(sp.byte_ids[w.chars[b + k]]);
            } else if (!(unk && prev_unk)) {
                emit(unk ? unk_id : int32_t(code));
            }
            prev_unk = unk;
            ends_at -= len;
        }
        int cnt;
        if (sp.reverse) {
            cnt = lo;
            row_start[s] = base;
        } else {
            if (sp.add_bos) ids[--hi] = sp.bos_id;
            cnt = n + 1 - hi;
            if (sp.add_eos) {
                ids[n + 1] = sp.eos_id;
                ++cnt;
            }
            row_start[s] = base + hi;
        }
        row_len[s] = cnt;
        return cnt;
    }
};

static __global__ __launch_bounds__(kTileThreads) void sp_relax_kernel(long long n, SpRelax f, RunStatus* status, uint32_t skip_flags) {
    if (status->flags & skip_flags) return;
    const long long i = (long long)blockIdx.x * kTileThreads + threadIdx.x;
    const int cnt = i < n ? f(i) : 0;
    const int most = wave_max(cnt);
    if (lane_id() == 0 && most > 0) atomicMax(&status->width, most);
}

// Total of the normalized bytes against the workspace they are written to.  An overflow also stops the lattice kernels, which
// would read the text behind its buffer (the host tells the two apart by kFlagItemsOverflow).
struct SpNormFin {
    RunStatus* status;
    long long cap;
    __device__ void operator()(long long total) const {
        status->n_items = total > INT32_MAX ? INT32_MAX : int32_t(total);
        if (total > cap) atomicOr(&status->flags, kFlagItemsOverflow | kFlagStageOverflow);
    }
};

// The scan over the rows' lengths ends here: the number of pairs, and dense_shape = {rows, longest row} where they fit.
template <class Index>
struct SparseFin {
    RunStatus* status;
    long long cap, n_rows;
    uint32_t skip_flags;
    Index* dense_shape;   // or nullptr (RaggedToSparse has none)
    __device__ void operator()(long long total) const {
        status->n_out = total > INT32_MAX ? INT32_MAX : int32_t(total);
        if (total > cap) {
            atomicOr(&status->flags, kFlagOutCapacity);
            return;
        }
        if (dense_shape && !(status->flags & skip_flags)) {
            dense_shape[0] = Index(n_rows);
            dense_shape[1] = Index(status->width);
        }
    }
};

template <class Index>
struct alignas(2 * sizeof(Index)) SparsePair {
    Index row, pos;
};

// RaggedToSparse's row lengths: ends[i] - begins[i]; a negative one (the reference's loop would not end) raises kFlagRange.
struct RaggedRowLen {
    const int32_t* begins;
    const int32_t* ends;
    RunStatus* status;
    __device__ long long operator()(long long i) const {
        const long long len = (long long)ends[i] - begins[i];
        if (len < 0) atomicOr(&status->flags, kFlagRange);
        return len < 0 ? 0 : len;
    }
};

// each_wave_kernel: a row's (row, position) pairs, one vector store each, and -- where there are values -- its ids beside them.
template <class Index>
struct SparseRows {
    const int32_t* out_begins;   // [rows] the scan's offsets
    const int32_t* out_ends;
    Index* indices;              // [total][2]
    const long long* src_start;  // [rows] or nullptr: no values
    const int32_t* src;
    int32_t* values;
    __device__ void operator()(long long row) const {
        const long long ob = out_begins[row];
        const int len = int(out_ends[row] - ob);
        SparsePair<Index>* dst = reinterpret_cast<SparsePair<Index>*>(indices) + ob;
        const int32_t* from = src_start ? src + src_start[row] : nullptr;
        for (int k = lane_id(); k < len; k += kWave) {
            dst[k] = SparsePair<Index>{Index(row), Index(k)};
            if (from) values[ob + k] = from[k];
        }
    }
};

}  // namespace ovtk
