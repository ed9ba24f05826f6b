// sp_bpe_kernels.hpp -- SentencepieceTokenizer for BPE models: the segmentation that stands where unigram_edges_kernel and
// sp_relax_kernel stand for unigram models (sentencepiece_kernels.hpp).  Normalization in front and the sparse outputs behind are shared.
//
// What sentencepiece does per normalized sentence (bpe::Model::Encode; restated in tests/gen_golden_sentencepiece_bpe.py, which
// asserts the restatement against the package):
//   * the text is cut into symbols, one character each, the length read off the lead byte's high nibble, clipped to the text's end;
//   * two adjacent symbols are a candidate when their bytes together are a NORMAL piece (USER_DEFINED and UNUSED pieces: such models
//     are refused at create); until none is left the candidate of the highest score is merged, among equal scores the leftmost;
//   * a remaining symbol's id is its piece's, unk_id where it is none; then SentencePieceProcessor's post-processing as for unigram
//     models: an unknown directly behind an unknown is dropped, with byte_fallback an unknown becomes the <0xHH> ids of its bytes
//     instead; bos in front, eos behind, or the row reversed.
//
// A SEGMENT is a stretch of the sentence between two cuts.  A cut is a symbol boundary no merged symbol can ever span -- proved from
// the vocabulary at create (api_sentencepiece.cpp) --, so segments merge independently and the order of merges in
// different segments cannot change the result.  The one rule: in front of the bytes of "▁" that do not follow the bytes of "▁".
//
// sp_bpe_kernel, a wave per sentence:
//   * a WAVE FORM is 64 consecutive bytes of the sentence, a lane per byte; the lanes of character starts are the live symbols (a
//     lane of a continuation byte is a dead symbol from the start, as a merged-away symbol is later).  The form ends at the last cut
//     in it, so it holds whole segments; the next form starts there.
//   * rounds: every live lane whose pair changed walks the pieces' trie over its symbol and the next live one (the first round: every
//     lane; later: the winner and the live lane in front of it) -> a segmented inclusive arg-max over (score, leftmost) by __shfl_up
//     gives one winner per segment -> winners take the next live lane's bytes, that lane dies.  One merge per segment and round:
//     within a segment exactly the package's order.  A round without a candidate ends the form; every other round removes a symbol.
//   * a segment longer than a form takes the LEFT-OVER path: its symbols are a linked list in the workspace (16 bytes per byte of
//     text), the wave sweeps it 64 bytes at a time for the arg-max, lane 0 merges and looks the two changed pairs up.  Same rule, one
//     merge per round, O(bytes^2 / 64); counted in RunStatus::n_exact.
//   * ids: a prefix sum over the form's live lanes places them in the sentence's staging stretch (sp_stage_base: the unigram path's
//     layout), ascending from entry 1 -- or descending from entry n for a reversed row; "the symbol before was unknown" is carried
//     from form to form.
// No wave waits for another, nothing spins on memory; every loop is bounded by the bytes of the sentence.
#pragma once

#include "device_common.hpp"
#include "ops_kernels.hpp"
#include "sentencepiece_kernels.hpp"
#include "unigram_kernels.hpp"

namespace ovtk {

struct alignas(16) SpBpeSym {   // left-over path: the state of the byte position it stands at
    int32_t end;    // where the symbol that starts here ends; 0: no live symbol starts here
    int32_t prev;   // start of the live symbol in front of it in its segment, -1: none
    int32_t cand;   // the piece this symbol and the next one make together, -1: none
    int32_t id;     // the piece this symbol is since its last merge, -1: never merged
};

struct SpBpeStretch {   // scan over the sentences: n + 1 entries each (UniStretch's layout, without the owners)
    UniWork w;
    __device__ long long operator()(long long s) const {
        const int n = w.str_bytes(s);
        return n < 0 ? 0 : n + 1;
    }
};
struct SpBpeStretchApply {
    UniWork w;
    __device__ void operator()(long long s, long long off, long long) const { w.node_off[s] = off; }
};

struct SpBpeRow {
    UniWork w;          // begins / ends / chars: the NORMALIZED sentences; dev.trie: the NORMAL pieces
    SpDev sp;
    SpBpeSym* syms;     // [w.cap]
    long long* row_start;
    int32_t* row_len;
    int cuts_on;        // the vocabulary proves the cut rule

    // the NORMAL piece that is exactly text[from, to), or -1
    __device__ __forceinline__ int32_t piece_of(const uint8_t* text, int from, int to) const {
        int cur = kTrieRoot;
        int32_t value = -1;
        bool kids = true;
        for (int i = from; i < to; ++i) {
            if (!kids || !uni_trie_step(w.dev.trie, cur, text[i], value, kids)) return -1;
        }
        return value;
    }
    // p is a symbol boundary of a sentence of n bytes: is it a cut?
    __device__ __forceinline__ bool cut_at(const uint8_t* text, int n, int p) const {
        if (!cuts_on || p <= 0 || p + 3 > n) return false;
        if (text[p] != 0xE2 || text[p + 1] != 0x96 || text[p + 2] != 0x81) return false;
        return !(p >= 3 && text[p - 3] == 0xE2 && text[p - 2] == 0x96 && text[p - 1] == 0x81);
    }
    // Character starts among the 64 bytes behind c0, the first at c0 + first (first < 4): bit i = a character starts at c0 + i.
    // m2 / m3 / m4: the lanes whose byte is a lead of at least 2 / 3 / 4 bytes.  Wave-uniform; `first` becomes the first start behind
    // the 64 bytes, relative to c0 + 64.
    static __device__ __forceinline__ unsigned long long chain(unsigned long long m2, unsigned long long m3, unsigned long long m4, int& first) {
        unsigned long long starts = 0;
        int i = first;
        while (i < kWave) {
            starts |= 1ull << i;
            i += 1 + int((m2 >> i) & 1) + int((m3 >> i) & 1) + int((m4 >> i) & 1);
        }
        first = i - kWave;
        return starts;
    }
    static __device__ __forceinline__ bool better(float os, int op, float bs, int bp) {   // (os, op) before (bs, bp)?  position -1: none
        return op >= 0 && (bp < 0 || os > bs || (os == bs && op < bp));
    }
    static __device__ __forceinline__ void fence_wave() {   // global hand-off between the lanes of this wave
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }

    struct Emit {
        int32_t* ids;   // the sentence's staging stretch
        int n, out;     // ids so far
        bool prev_unk, reverse;
        __device__ __forceinline__ void put(int k, int32_t id) const { ids[reverse ? n - k : 1 + k] = id; }
    };
    // The ids of up to 64 symbols in ascending order of lanes: `live` lanes hold a symbol of `len` bytes at text + at, `id` its piece or -1.
    __device__ __forceinline__ void emit(Emit& e, const uint8_t* text, bool live, int at, int len, int32_t id) const {
        const int l = lane_id();
        const unsigned long long lm = __ballot(live);
        const bool unk = live && id < 0;
        const unsigned long long below = lm & lanemask_lt();
        const int pl = below ? 63 - __clzll(below) : -1;
        const int before = __shfl(int(unk), pl < 0 ? l : pl);
        const bool prev_unk = pl < 0 ? e.prev_unk : before != 0;
        int cnt = 0;
        if (live) cnt = !unk ? 1 : sp.byte_fallback ? len : prev_unk ? 0 : 1;
        const int incl = wave_incl_sum(cnt);
        const int k0 = e.out + incl - cnt;
        if (cnt) {
            if (unk && sp.byte_fallback)
                for (int k = 0; k < len; ++k) e.put(k0 + k, sp.byte_ids[text[at + k]]);
            else e.put(k0, unk ? w.dev.unk_token_id : id);
        }
        e.out += wave_readlane(incl, kWave - 1);
        if (lm) e.prev_unk = wave_readlane(int(unk), 63 - __clzll(lm)) != 0;
    }

    // The segment that starts at sb and does not fit a form.  Returns its end.
    __device__ int leftover(const uint8_t* text, int n, int sb, SpBpeSym* S, Emit& e) const {
        const int l = lane_id();
        if (l == 0) atomicAdd(&w.status->n_exact, 1);
        // symbols and the segment's end
        int se = n, first = 0, last_start = -1;
        for (int c0 = sb; c0 < n; c0 += kWave) {
            const int p = c0 + l;
            const int len = p < n ? uni_char_len(text[p]) : 1;
            const unsigned long long m2 = __ballot(len >= 2), m3 = __ballot(len >= 3), m4 = __ballot(len >= 4);
            unsigned long long starts = chain(m2, m3, m4, first);
            if (n - c0 < kWave) starts &= (1ull << (n - c0)) - 1;
            const bool start = (starts >> l) & 1;
            const unsigned long long cuts = __ballot(start && p > sb && cut_at(text, n, p));
            if (cuts) {
                const int c = __ffsll(cuts) - 1;
                se = c0 + c;
                starts &= (1ull << c) - 1;
            }
            if (p < se) {
                const unsigned long long below = starts & lanemask_lt();
                const int prev = below ? c0 + 63 - __clzll(below) : last_start;
                const int end = p + len < n ? p + len : n;
                S[p] = ((starts >> l) & 1) ? SpBpeSym{end, prev, -1, -1} : SpBpeSym{0, -1, -1, -1};
            }
            if (starts) last_start = c0 + 63 - __clzll(starts);
            if (cuts) break;
        }
        fence_wave();
        for (int c0 = sb; c0 < se; c0 += kWave) {
            const int p = c0 + l;
            if (p < se && S[p].end) {
                const int q = S[p].end;
                if (q < se) S[p].cand = piece_of(text, p, S[q].end);
            }
        }
        fence_wave();
        // one merge per round; each removes a symbol
        for (int round = sb; round < se; ++round) {
            float bs = 0.0f;
            int bp = -1;
            for (int c0 = sb; c0 < se; c0 += kWave) {
                const int p = c0 + l;
                if (p >= se) continue;
                const SpBpeSym y = S[p];
                if (!y.end || y.cand < 0) continue;
                const float sc = w.dev.scores[y.cand];
                if (better(sc, p, bs, bp)) {
                    bs = sc;
                    bp = p;
                }
            }
#pragma unroll
            for (int d = kWave / 2; d > 0; d >>= 1) {
                const float os = __shfl_xor(bs, d);
                const int op = __shfl_xor(bp, d);
                if (better(os, op, bs, bp)) {
                    bs = os;
                    bp = op;
                }
            }
            if (bp < 0) break;   // (wave-uniform: every lane holds the wave's best)
            if (l == 0) {
                const int p = bp, q = S[p].end, r = S[q].end;
                S[p].id = S[p].cand;
                S[p].end = r;
                S[q] = SpBpeSym{0, -1, -1, -1};
                if (r < se) S[r].prev = p;
                S[p].cand = r < se ? piece_of(text, p, S[r].end) : -1;
                const int pp = S[p].prev;
                if (pp >= 0) S[pp].cand = piece_of(text, pp, r);
            }
            fence_wave();
        }
        for (int c0 = sb; c0 < se; c0 += kWave) {
            const int p = c0 + l;
            const SpBpeSym y = p < se ? S[p] : SpBpeSym{0, -1, -1, -1};
            const bool live = y.end != 0;
            int32_t id = y.id;
            if (live && id < 0) id = piece_of(text, p, y.end);
            emit(e, text, live, p, y.end - p, id);
        }
        return se;
    }

    __device__ int operator()(long long s) const {
        const int n = w.str_bytes(s);
        const int l = lane_id();
        const long long base = sp_stage_base(w, s);
        int32_t* ids = w.ids + base;
        Emit e{ids, n, 0, false, sp.reverse != 0};
        const uint8_t* text = w.chars + (n > 0 ? w.begins[s] : 0);
        SpBpeSym* S = syms + w.node_off[s];
        int pos = 0;   // a symbol boundary; the start of a segment
        while (pos < n) {
            int wl = n - pos < kWave ? n - pos : kWave;
            const int p = pos + l;
            const int len = l < wl ? uni_char_len(text[p]) : 1;
            const unsigned long long m2 = __ballot(len >= 2), m3 = __ballot(len >= 3), m4 = __ballot(len >= 4);
            int first = 0;
            unsigned long long starts = chain(m2, m3, m4, first);
            if (wl < kWave) starts &= (1ull << wl) - 1;
            else if (first > 0 && pos + kWave < n) {   // the last character leaves the form: it belongs to the next one
                wl = 63 - __clzll(starts);
                starts &= (1ull << wl) - 1;
            }
            const bool start = (starts >> l) & 1;
            unsigned long long segs = __ballot(start && l > 0 && cut_at(text, n, p)) | 1ull;
            if (pos + wl < n && !cut_at(text, n, pos + wl)) {   // the form's last segment goes on behind it
                const int c = 63 - __clzll(segs);
                if (c == 0) {
                    pos = leftover(text, n, pos, S, e);
                    continue;
                }
                wl = c;
                starts &= (1ull << wl) - 1;
                segs &= (1ull << wl) - 1;
            }
            // this lane's segment: [seg_b, seg_e)
            const unsigned long long upto = segs & ((lanemask_lt() << 1) | 1ull);
            const int seg_b = 63 - __clzll(upto);
            const unsigned long long above = segs & ~((lanemask_lt() << 1) | 1ull);
            const int seg_e = above ? __ffsll(above) - 1 : wl;
            bool live = (starts >> l) & 1;   // (the form may have been cut short since `start` was read)
            unsigned long long lm = starts;
            int32_t id = -1, cand = -1;
            float score = 0.0f;
            bool dirty = true;
            for (int round = 0; round < wl; ++round) {
                const unsigned long long m = lm & ~((lanemask_lt() << 1) | 1ull);   // the live lanes above this one
                const int nx = m ? __ffsll(m) - 1 : wl;
                const unsigned long long mm = m & (m - 1);
                const int nx2 = mm ? __ffsll(mm) - 1 : wl;
                if (dirty) {
                    cand = -1;
                    if (live && nx < seg_e) {
                        cand = piece_of(text, p, pos + (nx2 < seg_e ? nx2 : seg_e));
                        if (cand >= 0) score = w.dev.scores[cand];
                    }
                }
                if (!__ballot(cand >= 0)) break;
                // inclusive arg-max from the segment's first lane; its last lane ends up with the segment's winner
                float bs = score;
                int bp = cand >= 0 ? l : -1;
#pragma unroll
                for (int d = 1; d < kWave; d <<= 1) {
                    const float os = __shfl_up(bs, d);
                    const int op = __shfl_up(bp, d);
                    if (l - d >= seg_b && better(os, op, bs, bp)) {
                        bs = os;
                        bp = op;
                    }
                }
                const int win = __shfl(bp, l < wl ? seg_e - 1 : l);
                const bool winner = l < wl && win == l;
                if (winner) id = cand;
                const unsigned long long below = lm & lanemask_lt();
                const int pl = below ? 63 - __clzll(below) : -1;
                const int prev_wins = __shfl(int(winner), pl < 0 ? l : pl);
                const int next_wins = __shfl(int(winner), nx < wl ? nx : l);
                const bool killed = live && pl >= 0 && prev_wins != 0;   // (a winner's next live lane is in its segment: nx < seg_e)
                dirty = winner || (live && nx < wl && next_wins != 0);
                if (killed) {
                    live = false;
                    cand = -1;
                    dirty = false;
                }
                lm = __ballot(live);
            }
            const unsigned long long m = lm & ~((lanemask_lt() << 1) | 1ull);
            const int nx = m ? __ffsll(m) - 1 : wl;
            if (live && id < 0) id = piece_of(text, p, pos + nx);
            emit(e, text, live, p, nx - l, id);
            pos += wl;
        }
        int cnt = e.out;
        if (l == 0) {
            long long first_id = base + 1;
            if (sp.reverse) {
                first_id = base + n + 1 - cnt;
            } else {
                if (sp.add_bos) {
                    ids[0] = sp.bos_id;
                    first_id = base;
                }
                if (sp.add_eos) ids[1 + cnt] = sp.eos_id;
            }
            row_start[s] = first_id;
        }
        if (!sp.reverse) cnt += (sp.add_bos ? 1 : 0) + (sp.add_eos ? 1 : 0);
        if (l == 0) row_len[s] = cnt;
        return cnt;
    }
};

// A wave per sentence, the sentences strided over the grid; the longest row: one atomic per sentence that has ids.
static __global__ __launch_bounds__(kTileThreads) void sp_bpe_kernel(long long n, SpBpeRow f, RunStatus* status, uint32_t skip_flags) {
    if (status->flags & skip_flags) return;
    const long long stride = (long long)gridDim.x * (kTileThreads / kWave);
    for (long long i = (long long)blockIdx.x * (kTileThreads / kWave) + wave_in_block(); i < n; i += stride) {
        const int cnt = f(i);
        if (lane_id() == 0 && cnt > 0) atomicMax(&status->width, cnt);
    }
}

}  // namespace ovtk
