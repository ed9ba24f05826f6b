// string_ops_kernels.hpp -- BytesToChars (src/bytes_to_chars.cpp:284-339), CharsToBytes (src/chars_to_bytes.cpp:31-68),
// ContribStringSplit (src/contrib_string_ops.cpp:225-343) and ContribStringJoin (:62-199).  All four are count -> scan -> write
// passes over begins / ends / chars; nothing here keeps state between calls.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"
#include "scan_kernels.hpp"

namespace ovtk {

// ------------------------------------------------------------------------------- the byte <-> character map
// GPT-2's bytes_to_unicode as arithmetic: bytes 33..126, 161..172 and 174..255 are their own code point, the other 68 bytes, in
// ascending order (0..32, 127..160, 173), are U+0100..U+0143.  The character's UTF-8 has one byte for 33..126 and two otherwise.
__device__ __forceinline__ bool b2c_one_byte(uint32_t c) { return c - 33u <= 93u; }
__device__ __forceinline__ uint32_t b2c_code_point(uint32_t c) {
    if (c >= 174u || c - 161u <= 11u || b2c_one_byte(c)) return c;
    return c <= 32u ? 256u + c : c <= 160u ? 289u + (c - 127u) : 323u;
}
// the byte whose image the two-byte character `cp` is; -1: no byte has that image
__device__ __forceinline__ int c2b_byte(uint32_t cp) {
    if (cp < 161u || cp == 173u || cp > 323u) return -1;
    if (cp < 256u) return int(cp);
    const uint32_t k = cp - 256u;
    return k < 33u ? int(k) : k < 67u ? int(127u + k - 33u) : 173;
}
__device__ __forceinline__ bool utf8_cont(uint32_t c) { return (c & 0xC0u) == 0x80u; }   // 128..191
__device__ __forceinline__ bool c2b_lead(uint32_t c) { return c - 194u <= 3u; }           // 194..197

// ------------------------------------------------------------------------------- rows -> covered elements
// A wave per row: checks the row and marks its elements.  Rows must not go backwards: with begin >= the end of the row before
// (and begin <= end) the rows are disjoint and in element order, so the reference's row-by-row walk visits the covered
// elements in the order of their indices -- which is what lets the passes below scan over elements.
static __global__ __launch_bounds__(kBlockThreads) void ragged_cover_kernel(const int32_t* rb, const int32_t* re, long long n_rows,
                                                                            long long n, uint8_t* covered, RunStatus* status) {
    const long long stride = (long long)gridDim.x * kWavesPerBlock;
    for (long long j = (long long)blockIdx.x * kWavesPerBlock + wave_in_block(); j < n_rows; j += stride) {
        const long long b = rb[j], e = re[j];
        if (b < 0 || e < b || e > n) {
            if (lane_id() == 0) atomicOr(&status->flags, kFlagRange);
            continue;
        }
        if (j > 0 && b < re[j - 1] && lane_id() == 0) atomicOr(&status->flags, kFlagOverlap);
        for (long long i = b + lane_id(); i < e; i += kWave) covered[i] = 1;
    }
}

struct MapIn {
    const int32_t* begins;
    const int32_t* ends;
    const uint8_t* chars;
    const uint8_t* covered;
    const uint8_t* skips;   // BytesToChars' 6-input form, or nullptr
    long long n, n_chars;
};

// A lane per element: its length, and its length after the map -- TO_CHARS: plus one per byte outside 33..126 (not for a skipped
// element); else minus one per continuation byte.  An element no row covers counts nothing.  (One lane walks the whole element:
// a multi-megabyte element is a serial loop of that length.)
template <bool TO_CHARS>
static __global__ __launch_bounds__(kBlockThreads) void map_count_kernel(MapIn m, int32_t* in_len, uint32_t* out_len, RunStatus* status) {
    const long long stride = (long long)gridDim.x * kBlockThreads;
    for (long long i = (long long)blockIdx.x * kBlockThreads + threadIdx.x; i < m.n; i += stride) {
        int32_t li = 0;
        uint32_t lo = 0;
        if (m.covered[i]) {
            const long long b = m.begins[i], e = m.ends[i];
            if (b < 0 || e < b || e > m.n_chars) atomicOr(&status->flags, kFlagRange);
            else {
                li = int32_t(e - b);
                uint32_t d = 0;
                const uint8_t* s = m.chars + b;
                if (TO_CHARS) {
                    if (!(m.skips && m.skips[i]))
                        for (int k = 0; k < li; ++k) d += b2c_one_byte(s[k]) ? 0u : 1u;
                    lo = uint32_t(li) + d;
                } else {
                    for (int k = 0; k < li; ++k) d += utf8_cont(s[k]) ? 1u : 0u;
                    lo = uint32_t(li) - d;
                }
            }
        }
        in_len[i] = li;
        out_len[i] = lo;
    }
}

struct MapInLen {
    const int32_t* v;
    __device__ long long operator()(long long i) const { return v[i]; }
};
struct MapOutLen {
    const uint32_t* v;
    __device__ long long operator()(long long i) const { return v[i]; }
};
// off[i] = the scan's offset; off[n] = the total (the Fin functors below)
struct MapInOffsets {
    int32_t* off;
    __device__ void operator()(long long i, long long o, long long) const { off[i] = int32_t(o); }
};
struct MapInFin {
    int32_t* off;
    long long n;
    RunStatus* status;
    __device__ void operator()(long long total) const {
        off[n] = total >= INT32_MAX ? INT32_MAX : int32_t(total);
        if (total >= INT32_MAX) atomicOr(&status->flags, kFlagTooLong);
    }
};
// ... and, BytesToChars (out_begins != nullptr), the element's own offsets: [0, 0) for an element no row covers
struct MapOutOffsets {
    int32_t* off;
    const uint8_t* covered;
    int32_t* out_begins;
    int32_t* out_ends;
    __device__ void operator()(long long i, long long o, long long len) const {
        off[i] = int32_t(o);
        if (!out_begins) return;
        const bool c = covered[i] != 0;
        out_begins[i] = c ? int32_t(o) : 0;
        out_ends[i] = c ? int32_t(o + len) : 0;
    }
};
struct MapOutFin {
    int32_t* off;
    long long n, cap;
    RunStatus* status;
    __device__ void operator()(long long total) const {
        off[n] = total >= INT32_MAX ? INT32_MAX : int32_t(total);
        status->n_out = off[n];
        if (total >= INT32_MAX) atomicOr(&status->flags, kFlagTooLong);
        else if (total > cap) atomicOr(&status->flags, kFlagOutCapacity);
    }
};

// largest i in [lo, hi] with off[i] <= v (off[lo] <= v holds)
__device__ __forceinline__ int last_at_or_below(const int32_t* off, int lo, int hi, long long v) {
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// sum over the block; every thread calls it and receives it
__device__ __forceinline__ int block_sum(int v, int* wave_part) {
    const int w = wave_sum(v);
    __syncthreads();   // (wave_part may still be read from the call before)
    if (lane_id() == 0) wave_part[wave_in_block()] = w;
    __syncthreads();
    int t = 0;
    for (int k = 0; k < kWavesPerBlock; ++k) t += wave_part[k];
    return t;
}

// The write pass of both maps: a lane per input byte.  The covered elements' bytes, in element order, form one stretch of
// in_off[n] bytes; a block takes kMapBlockBytes of it at a time, kBlockThreads at a round.  The output is that stretch with every
// wide byte grown to two (TO_CHARS) or every continuation byte dropped, so a byte's place is its own position plus the growth in
// front of it: what the element scan gives for the block's first element (out_off - in_off), the growth of that element's bytes in
// front of the block (counted by the block: an element is a word or a piece, not a document), and a prefix count over the block.
// Elements longer than a block and blocks over hundreds of elements take the same path; a lane finds its element by a binary
// search among the block's.
// !TO_CHARS checks what it reads: any byte outside the 256 images is kFlagRange (the rule is local, string_ops header section).
// Whatever the bytes are, a store stays inside the output: a byte's place is the count of non-continuation bytes in front of it.
constexpr int kMapBlockBytes = 2048;
template <bool TO_CHARS>
static __global__ __launch_bounds__(kBlockThreads) void map_write_kernel(MapIn m, const int32_t* in_off, const int32_t* out_off,
                                                                         uint8_t* out, RunStatus* status, uint32_t skip_flags) {
    __shared__ int s_first, s_last, s_stop;
    __shared__ int s_part[kWavesPerBlock];
    // One thread reads the flags for the block: !TO_CHARS raises kFlagRange itself, so waves that each read the word could disagree
    // while another block is flagging a byte -- some would leave, and the rest would pass the barriers below without them.
    if (threadIdx.x == 0) s_stop = (status->flags & skip_flags) != 0;
    __syncthreads();
    if (s_stop) return;
    const long long total = in_off[m.n];
    const int tid = int(threadIdx.x);
    for (long long v0 = (long long)blockIdx.x * kMapBlockBytes; v0 < total; v0 += (long long)gridDim.x * kMapBlockBytes) {
        const long long v_last = v0 + kMapBlockBytes - 1 < total - 1 ? v0 + kMapBlockBytes - 1 : total - 1;
        __syncthreads();
        if (tid == 0) s_first = last_at_or_below(in_off, 0, int(m.n) - 1, v0);
        if (tid == kWave) s_last = last_at_or_below(in_off, 0, int(m.n) - 1, v_last);
        __syncthreads();
        const int i_first = s_first, i_last = s_last;
        // the growth in front of the block
        int head = 0;
        {
            const int head_len = int(v0 - in_off[i_first]);
            const uint8_t* s = m.chars + m.begins[i_first];
            if (!TO_CHARS) {
                for (int k = tid; k < head_len; k += kBlockThreads) head -= utf8_cont(s[k]) ? 1 : 0;
            } else if (!(m.skips && m.skips[i_first])) {
                for (int k = tid; k < head_len; k += kBlockThreads) head += b2c_one_byte(s[k]) ? 0 : 1;
            }
        }
        long long grow = (long long)out_off[i_first] - in_off[i_first] + block_sum(head, s_part);
        for (int r = 0; r < kMapBlockBytes / kBlockThreads; ++r) {
            const long long v = v0 + r * kBlockThreads + tid;
            const bool active = v <= v_last;
            int d = 0, k = 0, len = 0;
            uint32_t c = 0;
            bool raw = false;
            const uint8_t* s = nullptr;
            if (active) {
                const int i = last_at_or_below(in_off, i_first, i_last, v);
                k = int(v - in_off[i]);
                len = in_off[i + 1] - in_off[i];
                s = m.chars + m.begins[i];
                c = s[k];
                raw = TO_CHARS && m.skips && m.skips[i];
                d = TO_CHARS ? ((raw || b2c_one_byte(c)) ? 0 : 1) : (utf8_cont(c) ? -1 : 0);
            }
            const int incl = wave_incl_sum(d);
            __syncthreads();
            if (lane_id() == kWave - 1) s_part[wave_in_block()] = incl;
            __syncthreads();
            int before = 0, round = 0;
            for (int w = 0; w < kWavesPerBlock; ++w) {
                if (w < wave_in_block()) before += s_part[w];
                round += s_part[w];
            }
            if (active) {
                uint8_t* p = out + (v + grow + before + incl - d);
                if (TO_CHARS) {
                    if (d == 0) *p = uint8_t(c);
                    else {
                        const uint32_t cp = b2c_code_point(c);
                        p[0] = uint8_t(0xC0u | (cp >> 6));
                        p[1] = uint8_t(0x80u | (cp & 63u));
                    }
                } else if (c < 128u) {
                    *p = uint8_t(c);
                } else if (c2b_lead(c)) {
                    const uint32_t c2 = k + 1 < len ? s[k + 1] : 0u;
                    const int byte = utf8_cont(c2) ? c2b_byte(((c & 31u) << 6) | (c2 & 63u)) : -1;
                    if (byte < 0) atomicOr(&status->flags, kFlagRange);
                    else *p = uint8_t(byte);
                } else if (!(utf8_cont(c) && k > 0 && c2b_lead(s[k - 1]))) {
                    atomicOr(&status->flags, kFlagRange);
                }
            }
            grow += round;
        }
    }
}

// CharsToBytes: a row's string is its elements' text back to back -- [off[first element], off[one past its last)), off[n] = the total
static __global__ __launch_bounds__(kBlockThreads) void fused_rows_kernel(const int32_t* rb, const int32_t* re, long long n_rows,
                                                                          const int32_t* off, int32_t* out_begins, int32_t* out_ends,
                                                                          const RunStatus* status, uint32_t skip_flags) {
    if (status->flags & skip_flags) return;
    const long long stride = (long long)gridDim.x * kBlockThreads;
    for (long long j = (long long)blockIdx.x * kBlockThreads + threadIdx.x; j < n_rows; j += stride) {
        out_begins[j] = off[rb[j]];
        out_ends[j] = off[re[j]];
    }
}

// ------------------------------------------------------------------------------- ContribStringSplit
// A wave per element walks it 64 positions at a time; a lane per byte tests "the delimiter starts here" and the ballot is the
// chunk's occurrences.  A delimiter without a border (no proper prefix that is also a suffix) cannot overlap itself: every
// occurrence is a cut.  With a border (`aa`, `abab`) an occurrence inside the cut before it is none: the wave goes through the
// chunk's occurrences from the left, the end of the last cut carried from chunk to chunk -- string_view::find's leftmost-first rule.
constexpr int kSplitMaxRank = 8;
struct SplitIn {
    const int32_t* begins;
    const int32_t* ends;
    const uint8_t* chars;
    long long n, n_chars;
    const uint8_t* delim;
    int dlen;
    int bordered, skip_empty;
    int rank;
    long long stride[kSplitMaxRank];   // row-major strides of the input shape
};
// every lane of the wave calls this; returns the cuts among positions [base, base + 64), the same value in every lane
__device__ __forceinline__ unsigned long long split_cuts(const SplitIn& p, const uint8_t* s, int len, int base, int& cut_end) {
    const int k = base + lane_id();
    bool occ = k <= len - p.dlen;
    for (int j = 0; occ && j < p.dlen; ++j) occ = s[k + j] == p.delim[j];
    unsigned long long m = __ballot(occ);
    if (!p.bordered) return m;
    unsigned long long cuts = 0;
    while (m) {
        const int bit = __ffsll(m) - 1;
        m &= m - 1;
        if (base + bit >= cut_end) {
            cuts |= 1ull << bit;
            cut_end = base + bit + p.dlen;
        }
    }
    return cuts;
}
__device__ __forceinline__ int top_bit(unsigned long long m) { return 63 - __clzll(m); }   // m != 0

// tokens kept (-> the values' scan), bytes kept (-> the chars' scan), and the largest token count before skipping
struct SplitCount {
    SplitIn p;
    int32_t* tok_cnt;
    int32_t* byte_cnt;
    RunStatus* status;
    __device__ void operator()(long long i) const {
        const long long b = p.begins[i], e = p.ends[i];
        int n_tok = 0, kept = 0, bytes = 0;
        if (b < 0 || e < b || e > p.n_chars) {
            if (lane_id() == 0) atomicOr(&status->flags, kFlagRange);
        } else if (p.dlen == 0) {
            n_tok = kept = bytes = int(e - b);
        } else {
            const uint8_t* s = p.chars + b;
            const int len = int(e - b);
            int cuts = 0, prev_end = 0, cut_end = 0;
            for (int base = 0; base < len; base += kWave) {
                const unsigned long long cm = split_cuts(p, s, len, base, cut_end);
                if (!cm) continue;
                const unsigned long long below = cm & lanemask_lt();
                const int my_prev_end = below ? base + top_bit(below) + p.dlen : prev_end;
                const bool mine = (cm >> lane_id()) & 1ull;
                kept += __popcll(__ballot(mine && base + lane_id() != my_prev_end));
                cuts += __popcll(cm);
                prev_end = base + top_bit(cm) + p.dlen;
            }
            n_tok = cuts + 1;
            kept = p.skip_empty ? kept + (prev_end != len ? 1 : 0) : n_tok;
            bytes = len - cuts * p.dlen;
        }
        if (lane_id() == 0) {
            tok_cnt[i] = kept;
            byte_cnt[i] = bytes;
            if (n_tok > 0) atomicMax(&status->n_items, n_tok);
        }
    }
};
struct SplitValuesFin {
    RunStatus* status;
    long long cap;
    __device__ void operator()(long long total) const {
        status->n_exact = total >= INT32_MAX ? INT32_MAX : int32_t(total);
        if (total >= INT32_MAX) atomicOr(&status->flags, kFlagTooLong);
        else if (total > cap) atomicOr(&status->flags, kFlagOutCapacity);
    }
};
struct SplitCharsFin {
    RunStatus* status;
    long long cap;
    __device__ void operator()(long long total) const {
        status->n_out = total >= INT32_MAX ? INT32_MAX : int32_t(total);
        if (total >= INT32_MAX) atomicOr(&status->flags, kFlagTooLong);
        else if (total > cap) atomicOr(&status->flags, kFlagOutCapacity);
    }
};
struct SplitOut {
    int64_t* indices;   // [N][rank + 1]
    int32_t* begins;
    int32_t* ends;
    uint8_t* chars;
};
// The same walk behind the scans: an element's bytes outside its cuts go, in order, to byte_off[i] on; the token in front of every
// cut, and the one behind the last, take the next value slots from tok_off[i] on.
struct SplitWrite {
    SplitIn p;
    const int32_t* tok_off;
    const int32_t* byte_off;
    SplitOut o;
    __device__ void value(long long slot, long long i, int t, int begin, int len) const {
        o.begins[slot] = begin;
        o.ends[slot] = begin + len;
        int64_t* idx = o.indices + slot * (p.rank + 1);
        long long r = i;
        for (int d = 0; d < p.rank; ++d) {
            idx[d] = r / p.stride[d];
            r %= p.stride[d];
        }
        idx[p.rank] = t;
    }
    __device__ void operator()(long long i) const {
        const long long b = p.begins[i];
        const int len = int(p.ends[i] - b);   // (checked by the count pass: a flagged call does not get here)
        const uint8_t* s = p.chars + b;
        const long long slot0 = tok_off[i];
        const int byte0 = byte_off[i];
        if (p.dlen == 0) {
            for (int k = lane_id(); k < len; k += kWave) {
                o.chars[byte0 + k] = s[k];
                value(slot0 + k, i, k, byte0 + k, 1);
            }
            return;
        }
        int cuts = 0, kept = 0, prev_end = 0, cut_end = 0;
        for (int base = 0; base < len; base += kWave) {
            const unsigned long long cm = split_cuts(p, s, len, base, cut_end);
            const int k = base + lane_id();
            const bool mine = (cm >> lane_id()) & 1ull;
            const unsigned long long below = cm & lanemask_lt(), upto = below | (mine ? 1ull << lane_id() : 0ull);
            const int my_prev_end = below ? base + top_bit(below) + p.dlen : prev_end;
            // this lane's byte: dropped inside the last cut at or in front of it
            const int last_end = upto ? base + top_bit(upto) + p.dlen : prev_end;
            if (k < len && k >= last_end) o.chars[byte0 + k - (cuts + __popcll(upto)) * p.dlen] = s[k];
            // this lane's cut: the token in front of it
            const bool keep = mine && !(p.skip_empty && k == my_prev_end);
            const unsigned long long km = __ballot(keep);
            if (keep) {
                const int t = cuts + __popcll(below);
                value(slot0 + kept + rank_below(km), i, t, byte0 + my_prev_end - t * p.dlen, k - my_prev_end);
            }
            kept += __popcll(km);
            if (cm) {
                cuts += __popcll(cm);
                prev_end = base + top_bit(cm) + p.dlen;
            }
        }
        if (lane_id() == 0 && !(p.skip_empty && prev_end == len))
            value(slot0 + kept, i, cuts, byte0 + prev_end - cuts * p.dlen, len - prev_end);
    }
};

// ------------------------------------------------------------------------------- ContribStringJoin
// Output o = (outer index, inner index) joins the elements base + a * inner, a < axis_size: inner == 1 is the last axis, anything
// else a strided one.  A wave per output, 64 elements of the axis at a time.
struct JoinIn {
    const int32_t* begins;
    const int32_t* ends;
    const uint8_t* chars;
    long long n_chars;
    const uint8_t* sep;
    int slen;
    long long axis_size, inner;
    __device__ long long base_of(long long o) const { return (o / inner) * axis_size * inner + o % inner; }
};
struct JoinCount {
    JoinIn p;
    long long* lens;
    RunStatus* status;
    __device__ void operator()(long long o) const {
        const long long base = p.base_of(o);
        long long sum = 0;
        bool bad = false;
        for (long long a = lane_id(); a < p.axis_size; a += kWave) {
            const long long b = p.begins[base + a * p.inner], e = p.ends[base + a * p.inner];
            if (b < 0 || e < b || e > p.n_chars) bad = true;
            else sum += e - b;
        }
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        if (__ballot(bad) && lane_id() == 0) atomicOr(&status->flags, kFlagRange);
        if (lane_id() == 0) lens[o] = sum + (p.axis_size > 0 ? (p.axis_size - 1) * p.slen : 0);
    }
};
struct JoinLen {
    const long long* lens;
    __device__ long long operator()(long long o) const { return lens[o]; }
};
struct JoinOffsets {
    int32_t* out_begins;
    int32_t* out_ends;
    __device__ void operator()(long long o, long long off, long long len) const {
        out_begins[o] = int32_t(off);
        out_ends[o] = int32_t(off + len);
    }
};
__device__ __forceinline__ void wave_copy(const uint8_t* src, uint8_t* dst, int len) {
    for (int k = lane_id(); k < len; k += kWave) dst[k] = src[k];
}
struct JoinWrite {
    JoinIn p;
    const int32_t* out_begins;
    uint8_t* out;
    __device__ void operator()(long long o) const {
        const long long base = p.base_of(o);
        int at = out_begins[o];
        for (long long a0 = 0; a0 < p.axis_size; a0 += kWave) {
            const long long a = a0 + lane_id();
            int b = 0, len = 0;
            if (a < p.axis_size) {
                b = p.begins[base + a * p.inner];
                len = p.ends[base + a * p.inner] - b;
            }
            const int piece = a < p.axis_size ? len + (a > 0 ? p.slen : 0) : 0;   // the separator in front, then the text
            const int incl = wave_incl_sum(piece);
            const int mine = at + incl - piece;
            const int here = int(p.axis_size - a0 < kWave ? p.axis_size - a0 : kWave);
            for (int j = 0; j < here; ++j) {
                int dst = wave_readlane(mine, j);
                if (a0 + j > 0) {
                    wave_copy(p.sep, out + dst, p.slen);
                    dst += p.slen;
                }
                wave_copy(p.chars + wave_readlane(b, j), out + dst, wave_readlane(len, j));
            }
            at += wave_readlane(incl, kWave - 1);
        }
    }
};

}  // namespace ovtk
