// sp_detok_kernels.hpp -- SentencepieceDetokenizer / SentencepieceStreamDetokenizer (src/sentence_piece.cpp:395-433, :478-523):
// ids [batch, seq] -> one string per row.  The form is decode_count_kernel / decode_write_kernel's (ops_kernels.hpp): a wave per
// segment of kSegTokens tokens of a row counts the segment's bytes, the scan (scan_kernels.hpp) turns them into offsets and row
// bounds, a wave per segment writes -- text assembled in LDS, stored as coalesced dwords.  A token's text comes from a table built
// at create (one 16-byte entry per piece); two things a segment cannot see come from outside it:
//   * the row's first token that ends the start-of-sentence state (sp_detok_first_kernel, a wave per row that stops at the first
//     hit): up to and including it a piece that begins with the space symbol loses that one byte;
//   * for a run of BYTE pieces that reaches a segment's edge, the byte pieces next to it in the row -- ids outside the vocabulary
//     do not count and do not break a run, any other piece does.  Whether a byte is copied or becomes U+FFFD depends on at most
//     three bytes either side (a lead byte is never a continuation), so the count pass walks from the edge only while it sees
//     continuation bytes, at most three of them, skipping dropped ids, bounded by the row; it leaves what it found in unit_ctx
//     for the write pass.  A segment whose edge token is no such byte (all padding, ordinary text) walks nowhere.
// The stream op is the same kernels over a second table (raw pieces, <0xHH> by the name's shape as one byte, no BYTE flag, no
// stripping, no first-token pass).
#pragma once

#include "ops_kernels.hpp"

namespace ovtk {

// A piece's table entry: x, y, z = the first 12 bytes of its text (the space symbol already replaced), w = what follows.
constexpr uint32_t kSdLenMask = 0x3FFu;        // bytes of the text in the middle of a sentence (a BYTE piece: see kSdByte)
constexpr uint32_t kSdInVocab = 1u << 10;      // set in every entry: an id outside [0, V) reads as the all-zero entry
constexpr uint32_t kSdByte = 1u << 11;         // a BYTE piece: bits 16-23 hold its value; 1 byte where its run is UTF-8 there, else 3
constexpr uint32_t kSdStrip = 1u << 12;        // the text's first byte is the space of a leading space symbol: dropped at a sentence's start
constexpr uint32_t kSdEndsStart = 1u << 13;    // the piece ends the start-of-sentence state
constexpr int kSdByteShift = 16;
constexpr int kSdInline = 12;
constexpr int kSdNoByte = 256;                 // context code of "no byte piece here" (any value >= 256 fails every range test below)

struct SpDetokDev {
    const int32_t* ids;        // [batch * seq]
    const uint4* pieces;       // [vocab_size]
    const int32_t* t_begins;   // texts longer than kSdInline bytes are read from t_chars + t_begins[id]
    const uint8_t* t_chars;
    int32_t vocab_size;
    int32_t utf8_runs;         // the table has BYTE entries (Decode; never the stream op)
    const int32_t* row_first;  // [batch] index of the row's first kSdEndsStart token (seq: none); nullptr: nothing is stripped
};

__device__ __forceinline__ bool sd_cont(int c) { return (c & ~0x3F) == 0x80; }
// Length of the well-formed UTF-8 sequence c0 c1 c2 c3 starts with, 0 if none (sentencepiece's DecodeUTF8: shortest form only,
// no surrogates, nothing above U+10FFFF).
__device__ __forceinline__ int sd_seq_len(int c0, int c1, int c2, int c3) {
    if (c0 < 0xC2 || c0 > 0xF4) return 0;
    if (c0 < 0xE0) return sd_cont(c1) ? 2 : 0;
    if (c0 < 0xF0) {
        const int lo = c0 == 0xE0 ? 0xA0 : 0x80, hi = c0 == 0xED ? 0x9F : 0xBF;
        return c1 >= lo && c1 <= hi && sd_cont(c2) ? 3 : 0;
    }
    const int lo = c0 == 0xF0 ? 0x90 : 0x80, hi = c0 == 0xF4 ? 0x8F : 0xBF;
    return c1 >= lo && c1 <= hi && sd_cont(c2) && sd_cont(c3) ? 4 : 0;
}
// w[0] is a byte piece's value, w[-3..3] its neighbours' (kSdNoByte: none): is the byte part of a well-formed character?
__device__ __forceinline__ bool sd_byte_kept(const uint16_t* w) {
    const int b = w[0];
    if (b < 0x80) return true;
    if (b >= 0xC0) return sd_seq_len(b, w[1], w[2], w[3]) > 0;
    for (int k = 1; k <= 3; ++k)   // the nearest byte in front that is no continuation is the only lead that can own this one
        if (!sd_cont(w[-k])) return sd_seq_len(w[-k], w[1 - k], w[2 - k], w[3 - k]) > k;
    return false;
}
__device__ __forceinline__ int sd_code(uint32_t meta) { return (meta & kSdByte) ? int((meta >> kSdByteShift) & 0xFFu) : kSdNoByte; }

// The byte pieces next to token `from` of a row, walking by `dir` (-1 / +1) over [0, seq): out[0..2], nearest first.  Stops
// behind the first that is no continuation byte (nothing beyond it can matter), at a non-byte piece, and at the row's end.
__device__ __forceinline__ void sd_walk(const SpDetokDev& d, const int32_t* rid, int seq, int from, int dir, int (&out)[3]) {
    out[0] = out[1] = out[2] = kSdNoByte;
    int found = 0;
    for (int s = from; s >= 0 && s < seq; s += dir * kWave) {
        const int t = s + dir * lane_id();   // lane 0 is the nearest
        const int32_t id = t >= 0 && t < seq ? rid[t] : INT32_MAX;
        const bool inv = uint32_t(id) < uint32_t(d.vocab_size);
        const int code = inv ? sd_code(d.pieces[id].w) : kSdNoByte;
        unsigned long long m = __ballot(inv);
        while (m) {
            const int k = __ffsll(m) - 1;
            const int c = wave_bcast(code, k);
            out[found++] = c;
            if (found == 3 || !sd_cont(c)) return;
            m &= m - 1;
        }
    }
}

// Row pre-pass: row_first[row] = index of the first token whose piece ends the start-of-sentence state, seq if there is none.
static __global__ __launch_bounds__(kBlockThreads) void sp_detok_first_kernel(SpDetokDev d, int seq, long long batch, int32_t* row_first) {
    const int l = lane_id();
    const long long my_waves = (long long)gridDim.x * kWavesPerBlock;
    for (long long row = (long long)blockIdx.x * kWavesPerBlock + wave_in_block(); row < batch; row += my_waves) {
        const int32_t* rid = d.ids + row * seq;
        int first = seq;
        for (int s = 0; s < seq; s += kWave) {
            const int t = s + l;
            const int32_t id = t < seq ? rid[t] : INT32_MAX;
            const uint32_t meta = uint32_t(id) < uint32_t(d.vocab_size) ? d.pieces[id].w : 0u;
            const unsigned long long m = __ballot((meta & kSdEndsStart) != 0);
            if (m) {
                first = s + __ffsll(m) - 1;
                break;
            }
        }
        if (l == 0) row_first[row] = first;
    }
}

constexpr int kSdChunks = kSegTokens / kWave;   // a lane holds one token of each 64-token chunk of its segment

// kWrite false: the count pass (unit_bytes, unit_ctx; a negative id raises kFlagRange).  true: the write pass.
template <bool kWrite>
static __global__ __launch_bounds__(kBlockThreads) void sp_detok_kernel(SpDetokDev d, int seq, int n_seg, long long n_units, long long* unit_bytes,
                                                                        unsigned long long* unit_ctx, const long long* unit_off, uint8_t* out_chars,
                                                                        RunStatus* status) {
    __shared__ uint16_t ctx_all[kWavesPerBlock][kSegTokens + 8];   // [3 in front][the segment's in-vocabulary tokens][3 behind]
    __shared__ uint32_t seg_all[kWrite ? kWavesPerBlock : 1][kWrite ? kSegLdsBytes / 4 + 2 : 1];
    if (kWrite && (status->flags & (kFlagOutCapacity | kFlagRange))) return;
    const int l = lane_id();
    uint16_t* ctx = ctx_all[wave_in_block()] + 3;
    const long long my_waves = (long long)gridDim.x * kWavesPerBlock;
    for (long long u = (long long)blockIdx.x * kWavesPerBlock + wave_in_block(); u < n_units; u += my_waves) {
        const long long row = u / n_seg;
        const int seg = int(u - row * n_seg);
        const int t0 = seg * kSegTokens, t1 = t0 + kSegTokens < seq ? t0 + kSegTokens : seq;
        const int32_t* rid = d.ids + row * seq;
        const int first = d.row_first ? uniform_load(d.row_first + row) : -1;
        // ---- the segment's table entries
        uint4 pc[kSdChunks];
        bool neg = false, any_byte = false;
#pragma unroll
        for (int c = 0; c < kSdChunks; ++c) {
            const int t = t0 + c * kWave + l;
            const int32_t id = t < t1 ? rid[t] : INT32_MAX;
            neg |= id < 0;
            pc[c] = make_uint4(0, 0, 0, 0);
            if (uint32_t(id) < uint32_t(d.vocab_size)) {
                if (kWrite) pc[c] = d.pieces[id];
                else pc[c].w = d.pieces[id].w;
            }
            any_byte |= (pc[c].w & kSdByte) != 0;
        }
        if (!kWrite && __any(neg)) {
            if (l == 0) atomicOr(&status->flags, kFlagRange);
        }
        // ---- byte pieces: the values of the in-vocabulary tokens in a row of LDS, three neighbours either side
        const bool bytes_here = d.utf8_runs && __any(any_byte);
        if (bytes_here) {
            wave_sync();   // (the previous segment's readers are through)
            int n_inv = 0;
#pragma unroll
            for (int c = 0; c < kSdChunks; ++c) {
                const bool inv = (pc[c].w & kSdInVocab) != 0;
                const unsigned long long m = __ballot(inv);
                if (inv) ctx[n_inv + rank_below(m)] = uint16_t(sd_code(pc[c].w));
                n_inv += __popcll(m);
            }
            wave_sync();
            int pred[3] = {kSdNoByte, kSdNoByte, kSdNoByte}, succ[3] = {kSdNoByte, kSdNoByte, kSdNoByte};
            if (!kWrite) {
                const int head = ctx[0], tail = ctx[n_inv - 1];   // (n_inv >= 1: there is a byte piece)
                if (t0 > 0 && sd_cont(head)) sd_walk(d, rid, seq, t0 - 1, -1, pred);
                if (t1 < seq && tail >= 0x80 && tail < kSdNoByte) sd_walk(d, rid, seq, t1, +1, succ);
                unsigned long long packed = 0;
                for (int k = 0; k < 3; ++k) packed |= (unsigned long long)pred[k] << (9 * k) | (unsigned long long)succ[k] << (27 + 9 * k);
                if (l == 0) unit_ctx[u] = packed;
            } else {
                const unsigned long long packed = uniform_load(unit_ctx + u);
                for (int k = 0; k < 3; ++k) {
                    pred[k] = int(packed >> (9 * k)) & 0x1FF;
                    succ[k] = int(packed >> (27 + 9 * k)) & 0x1FF;
                }
            }
            if (l < 3) {
                ctx[-1 - l] = uint16_t(l == 0 ? pred[0] : l == 1 ? pred[1] : pred[2]);
                ctx[n_inv + l] = uint16_t(l == 0 ? succ[0] : l == 1 ? succ[1] : succ[2]);
            }
            wave_sync();
        }
        // ---- every token's bytes
        int len[kSdChunks];
        int total = 0;
        {
            int n_inv = 0;
#pragma unroll
            for (int c = 0; c < kSdChunks; ++c) {
                const uint32_t meta = pc[c].w;
                const int t = t0 + c * kWave + l;
                len[c] = int(meta & kSdLenMask);
                if ((meta & kSdStrip) && t <= first) len[c] -= 1;
                if (bytes_here) {
                    const unsigned long long m = __ballot((meta & kSdInVocab) != 0);
                    if (meta & kSdByte) len[c] = sd_byte_kept(ctx + n_inv + rank_below(m)) ? 1 : 3;
                    n_inv += __popcll(m);
                }
                total += len[c];
            }
        }
        if (!kWrite) {
            total = wave_sum(total);
            if (l == 0) unit_bytes[u] = total;
            continue;
        }
        // ---- the write pass: the text into LDS at the output's dword phase, then out (decode_write_kernel's flush)
        total = int(unit_bytes[u]);
        const long long base = unit_off[u];
        const int skew = int((reinterpret_cast<uintptr_t>(out_chars) + base) & 3);
        const bool staged = total + skew <= kSegLdsBytes;
        uint32_t* wbuf = seg_all[kWrite ? wave_in_block() : 0];
        uint8_t* buf = reinterpret_cast<uint8_t*>(wbuf);
        wave_sync();   // the previous segment's flush is done with the buffer
        int run = 0;
#pragma unroll
        for (int c = 0; c < kSdChunks; ++c) {
            const int n = len[c];
            const int incl = wave_incl_sum(n);
            const int off = run + incl - n;
            run += wave_readlane(incl, kWave - 1);
            if (n == 0) continue;
            const uint32_t meta = pc[c].w;
            uint32_t w0 = pc[c].x, w1 = pc[c].y, w2 = pc[c].z;
            int skip = 0;
            if (meta & kSdByte) {
                if (n == 3) w0 = 0xBDBFEFu;   // U+FFFD
            } else if (n < int(meta & kSdLenMask)) {   // the start of the sentence: without the leading space
                skip = 1;
                w0 = (w0 >> 8) | (w1 << 24);
                w1 = (w1 >> 8) | (w2 << 24);
                w2 >>= 8;
            }
            const int n_in = n < kSdInline - skip ? n : kSdInline - skip;
            auto emit = [&](uint8_t* dst) {
#pragma unroll
                for (int k = 0; k < kSdInline; ++k) {
                    const uint32_t w = k < 4 ? w0 : k < 8 ? w1 : w2;
                    if (k < n_in) dst[k] = uint8_t(w >> (8 * (k & 3)));
                }
                if (n > n_in) {
                    const int32_t id = rid[t0 + c * kWave + l];
                    const uint8_t* src = d.t_chars + d.t_begins[id] + skip;
                    for (int k = n_in; k < n; ++k) dst[k] = src[k];
                }
            };
            if (staged) emit(buf + skew + off);
            else emit(out_chars + base + off);   // an oversized segment: straight to the output
        }
        if (!staged) continue;
        wave_sync();
        uint8_t* gout = out_chars + base - skew;
        const int lo = skew, hi = skew + total;
        const int d0 = (lo + 3) >> 2, d1 = hi >> 2;   // dwords [d0, d1) lie inside
        for (int k = d0 + l; k < d1; k += kWave) reinterpret_cast<uint32_t*>(gout)[k] = wbuf[k];
        if (d0 <= d1) {
            if (l < 4 * d0 - lo) gout[lo + l] = buf[lo + l];
            if (l < hi - 4 * d1) gout[4 * d1 + l] = buf[4 * d1 + l];
        } else if (l < total) {
            gout[lo + l] = buf[lo + l];
        }
    }
}

}  // namespace ovtk
