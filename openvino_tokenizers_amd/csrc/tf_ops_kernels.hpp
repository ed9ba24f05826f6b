// tf_ops_kernels.hpp -- the three ops only the reference's TensorFlow front end creates (src/tensorflow_translators.cpp):
// StringToHashBucket (src/string_to_hash_bucket.cpp:10-220), EqualStr (src/equal_str.cpp:29-61) and RaggedToRagged
// (src/ragged_to_ragged.cpp:43-98).  All three are integer work over begins / ends / chars, a lane per element.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"

namespace ovtk {

// ------------------------------------------------------------------------------- unaligned fetches
// 4 / 8 / 16 bytes at ANY byte address, little endian.  gfx950 serves an unaligned global load in hardware: the packed types make the
// compiler emit one global_load_dword / _dwordx2 / _dwordx4 instead of assuming an alignment the strings do not have.  The emulator
// build keeps the memcpy form.  Every caller passes an address whose bytes lie inside its string.
struct __attribute__((packed, aligned(1))) RawU32 { uint32_t v; };
struct __attribute__((packed, aligned(1))) RawU64 { uint64_t v; };
struct __attribute__((packed, aligned(1))) RawU128 { uint64_t lo, hi; };
__device__ __forceinline__ uint32_t fetch_u32(const uint8_t* p) {
#ifdef OVTK_SIMT_EMULATOR
    uint32_t v;
    __builtin_memcpy(&v, p, sizeof v);
    return v;
#else
    return reinterpret_cast<const RawU32*>(p)->v;
#endif
}
__device__ __forceinline__ uint64_t fetch_u64(const uint8_t* p) {
#ifdef OVTK_SIMT_EMULATOR
    uint64_t v;
    __builtin_memcpy(&v, p, sizeof v);
    return v;
#else
    return reinterpret_cast<const RawU64*>(p)->v;
#endif
}
// the 64 bytes at p as eight words (four 16-byte loads)
struct HashBlock { uint64_t d[8]; };
__device__ __forceinline__ HashBlock fetch_block(const uint8_t* p) {
    HashBlock b;
#ifdef OVTK_SIMT_EMULATOR
    __builtin_memcpy(b.d, p, sizeof b.d);
#else
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const RawU128 q = reinterpret_cast<const RawU128*>(p)[k];
        b.d[2 * k] = q.lo;
        b.d[2 * k + 1] = q.hi;
    }
#endif
    return b;
}

// ------------------------------------------------------------------------------- StringToHashBucket
// FarmHash Fingerprint64 (farmhashna::Hash64), the function behind TensorFlow's StringToHashBucketFast.  Unsigned 64-bit arithmetic
// with wrap-around throughout; the length enters as an unsigned 64-bit number; single bytes are read as uint8_t.
constexpr uint64_t kFarmK0 = 0xc3a5c85c97cb3127ull, kFarmK1 = 0xb492b66fbe98f273ull, kFarmK2 = 0x9ae16a3b2f90404full;
__device__ __forceinline__ uint64_t farm_rot(uint64_t v, int s) { return (v >> s) | (v << (64 - s)); }   // s in 1..63
__device__ __forceinline__ uint64_t farm_mix(uint64_t v) { return v ^ (v >> 47); }
__device__ __forceinline__ uint64_t farm_len16(uint64_t u, uint64_t v, uint64_t mul) {
    uint64_t a = (u ^ v) * mul;
    a ^= a >> 47;
    uint64_t b = (v ^ a) * mul;
    b ^= b >> 47;
    return b * mul;
}
__device__ __forceinline__ uint64_t farm_short(const uint8_t* s, uint64_t len) {   // 0..16 bytes
    const uint64_t mul = kFarmK2 + len * 2;
    if (len >= 8) {
        const uint64_t a = fetch_u64(s) + kFarmK2, b = fetch_u64(s + len - 8);
        return farm_len16(farm_rot(b, 37) * mul + a, (farm_rot(a, 25) + b) * mul, mul);
    }
    if (len >= 4) return farm_len16(len + (uint64_t(fetch_u32(s)) << 3), fetch_u32(s + len - 4), mul);
    if (len > 0) {   // 1..3 bytes, one at a time: a 4-byte fetch would leave the string
        const uint32_t a = s[0], b = s[len >> 1], c = s[len - 1];
        const uint32_t y = a + (b << 8), z = uint32_t(len) + (c << 2);
        return farm_mix(y * kFarmK2 ^ z * kFarmK0) * kFarmK2;
    }
    return kFarmK2;
}
__device__ __forceinline__ uint64_t farm_17_32(const uint8_t* s, uint64_t len) {
    const uint64_t mul = kFarmK2 + len * 2;
    const uint64_t a = fetch_u64(s) * kFarmK1, b = fetch_u64(s + 8), c = fetch_u64(s + len - 8) * mul, d = fetch_u64(s + len - 16) * kFarmK2;
    return farm_len16(farm_rot(a + b, 43) + farm_rot(c, 30) + d, a + farm_rot(b + kFarmK2, 18) + c, mul);
}
__device__ __forceinline__ uint64_t farm_33_64(const uint8_t* s, uint64_t len) {
    const uint64_t mul = kFarmK2 + len * 2;
    const uint64_t a = fetch_u64(s) * kFarmK2, b = fetch_u64(s + 8), c = fetch_u64(s + len - 8) * mul, d = fetch_u64(s + len - 16) * kFarmK2;
    const uint64_t y = farm_rot(a + b, 43) + farm_rot(c, 30) + d;
    const uint64_t z = farm_len16(y, a + farm_rot(b + kFarmK2, 18) + c, mul);
    const uint64_t e = fetch_u64(s + 16) * mul, f = fetch_u64(s + 24);
    const uint64_t g = (y + fetch_u64(s + len - 32)) * mul, h = (z + fetch_u64(s + len - 24)) * mul;
    return farm_len16(farm_rot(e + f, 43) + farm_rot(g, 30) + h, e + farm_rot(f + a, 18) + g, mul);
}
// The state of the loop over 64-byte blocks and one round of it.  The rounds inside the loop run with mul = k1, times = 1; the round
// over the string's last 64 bytes with the mul the loop's state gives and times = 9.
struct FarmState { uint64_t x, y, z, v0, v1, w0, w1; };
__device__ __forceinline__ void farm_weak32(const uint64_t* d, uint64_t a, uint64_t b, uint64_t& first, uint64_t& second) {
    a += d[0];
    b = farm_rot(b + a + d[3], 21);
    const uint64_t c = a;
    a += d[1] + d[2];
    b += farm_rot(a, 44);
    first = a + d[3];
    second = b + c;
}
__device__ __forceinline__ void farm_round(FarmState& t, const HashBlock& k, uint64_t mul, uint64_t times) {
    uint64_t x = farm_rot(t.x + t.y + t.v0 + k.d[1], 37) * mul;
    uint64_t y = farm_rot(t.y + t.v1 + k.d[6], 42) * mul;
    x ^= t.w1 * times;
    y += t.v0 * times + k.d[5];
    const uint64_t z = farm_rot(t.z + t.w0, 33) * mul;
    farm_weak32(k.d, t.v1 * mul, x + t.w0, t.v0, t.v1);
    farm_weak32(k.d + 4, z + t.w1, y + k.d[2], t.w0, t.w1);
    t.x = z;   // (x and z change places)
    t.y = y;
    t.z = x;
}
// A lane streams its own string: the next block's loads are issued before the round over the current one.  The last round reads
// [len - 64, len), which overlaps the block before wherever len is no multiple of 64; no fetch leaves [s, s + len).
__device__ __forceinline__ uint64_t farm_long(const uint8_t* s, uint64_t len) {   // > 64 bytes
    constexpr uint64_t seed = 81;
    FarmState t;
    t.y = seed * kFarmK1 + 113;
    t.z = farm_mix(t.y * kFarmK2 + 113) * kFarmK2;
    t.x = seed * kFarmK2 + fetch_u64(s);
    t.v0 = t.v1 = t.w0 = t.w1 = 0;
    const uint64_t n_blocks = (len - 1) / 64;   // >= 1; behind them 1..64 bytes are left
    const uint8_t* const last = s + (len - 64);
    HashBlock cur = fetch_block(s);
    for (uint64_t k = 1; k <= n_blocks; ++k) {
        const HashBlock next = fetch_block(k < n_blocks ? s + 64 * k : last);
        farm_round(t, cur, kFarmK1, 1);
        cur = next;
    }
    const uint64_t mul = kFarmK1 + ((t.z & 0xff) << 1);
    t.w0 += (len - 1) & 63;
    t.v0 += t.w0;
    t.w0 += t.v0;
    farm_round(t, cur, mul, 9);
    return farm_len16(farm_len16(t.v0, t.w0, mul) + farm_mix(t.y) * kFarmK0 + t.z, farm_len16(t.v1, t.w1, mul) + t.x, mul);
}
__device__ __forceinline__ uint64_t farm_fingerprint64(const uint8_t* s, uint64_t len) {
    if (len <= 16) return farm_short(s, len);
    if (len <= 32) return farm_17_32(s, len);
    if (len <= 64) return farm_33_64(s, len);
    return farm_long(s, len);
}

// A lane per string.  num_buckets is any value in 1 .. 2^63 - 1: the modulo is unsigned, 64 bits wide, by a run-time value (the
// compiler's expansion: gfx950 has no 64-bit divide); a power of two is a mask.
static __global__ __launch_bounds__(kBlockThreads) void string_hash_kernel(const int32_t* begins, const int32_t* ends, const uint8_t* chars,
                                                                           long long n, long long n_chars, uint64_t num_buckets,
                                                                           int64_t* out, RunStatus* status) {
    const bool pow2 = (num_buckets & (num_buckets - 1)) == 0;
    const long long stride = (long long)gridDim.x * kBlockThreads;
    for (long long i = (long long)blockIdx.x * kBlockThreads + threadIdx.x; i < n; i += stride) {
        const long long b = begins[i], e = ends[i];
        if (b < 0 || e < b || e > n_chars) {   // string_to_hash_bucket.cpp:215 asserts begins <= ends
            atomicOr(&status->flags, kFlagRange);
            continue;
        }
        const uint64_t h = farm_fingerprint64(chars + b, uint64_t(e - b));
        out[i] = int64_t(pow2 ? h & (num_buckets - 1) : h % num_buckets);
    }
}

// ------------------------------------------------------------------------------- EqualStr
// Element i compares string (i < n1 ? i : 0) of the first operand with string (i < n2 ? i : 0) of the second (equal_str.cpp:48-49:
// the reference's rule, not NumPy's).  Lengths first, then eight bytes at a time, then the last bytes.  Against one constant (n2 == 1)
// the second operand's offsets and bytes are the same addresses in every lane: one cache line serves the wave.
struct EqualOperand {
    const int32_t* begins;
    const int32_t* ends;
    const uint8_t* chars;
    long long n, n_chars;
};
static __global__ __launch_bounds__(kBlockThreads) void equal_str_kernel(EqualOperand a, EqualOperand b, long long n, int32_t* out,
                                                                         RunStatus* status) {
    const long long stride = (long long)gridDim.x * kBlockThreads;
    for (long long i = (long long)blockIdx.x * kBlockThreads + threadIdx.x; i < n; i += stride) {
        const long long ia = i < a.n ? i : 0, ib = i < b.n ? i : 0;
        const long long ab = a.begins[ia], ae = a.ends[ia], bb = b.begins[ib], be = b.ends[ib];
        if (ab < 0 || ae < ab || ae > a.n_chars || bb < 0 || be < bb || be > b.n_chars) {
            atomicOr(&status->flags, kFlagRange);
            continue;
        }
        const long long len = ae - ab;
        bool eq = len == be - bb;
        if (eq) {
            const uint8_t *p = a.chars + ab, *q = b.chars + bb;
            long long k = 0;
            for (; eq && k + 8 <= len; k += 8) eq = fetch_u64(p + k) == fetch_u64(q + k);
            for (; eq && k < len; ++k) eq = p[k] == q[k];
        }
        out[i] = eq ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------- RaggedToRagged
// Sorted row ids -> begins / ends per row: the parallel form of ragged_to_ragged.cpp:56-95.  A lane per id compares it with the id
// before: the first id of a run writes its row's begin, the end of the run before, and owns the empty rows between the two (they
// are [i, i), i = this run's start); the last id writes its row's end and owns the rows behind it.  Owned rows are filled by the
// whole wave, 64 rows a step; a stretch of more than kLongGap rows goes to a list that gap_fill_kernel works through with the grid
// (stretches are disjoint: a batch has at most batch_size / kLongGap + 2 of them).
// The first id >= batch_size stands where the reference leaves its loop: the rows behind the last run in range are [s, s) with s
// that run's START (the reference's value), the run's own row -- unwritten there -- is [s, j).
// A negative id: kFlagRange.  An id below the one before: kFlagUnsorted; nothing is promised about the outputs then, but every
// store stays inside [0, batch_size): a lane writes only where 0 <= prev <= cur holds for its own pair.
constexpr int kLongGap = 4096;
struct GapList {
    int32_t* entries;   // [cap][3]: first row, rows, value
    int32_t cap;
    int32_t* count;
};
// every lane of the wave calls this together; rows == 0: this lane owns nothing
__device__ __forceinline__ void wave_fill_rows(int first, int rows, int value, int32_t* begins, int32_t* ends, const GapList& gl) {
    if (rows > kLongGap) {
        const int slot = atomicAdd(gl.count, 1);
        if (slot < gl.cap) {   // (more than cap: unsorted ids, reported by the lane that saw them)
            gl.entries[3 * slot] = first;
            gl.entries[3 * slot + 1] = rows;
            gl.entries[3 * slot + 2] = value;
        }
        rows = 0;
    }
    unsigned long long owners = __ballot(rows > 0);
    while (owners) {
        const int src = __ffsll(owners) - 1;
        owners &= owners - 1;
        const int f = wave_readlane(first, src), c = wave_readlane(rows, src), v = wave_readlane(value, src);
        for (int k = lane_id(); k < c; k += kWave) {
            begins[f + k] = v;
            ends[f + k] = v;
        }
    }
}
static __global__ __launch_bounds__(kBlockThreads) void rowids_to_ragged_kernel(const int32_t* rowids, int n, int batch, int32_t* begins,
                                                                                int32_t* ends, GapList gl, RunStatus* status) {
    const long long stride = (long long)gridDim.x * kBlockThreads;
    for (long long base = (long long)blockIdx.x * kBlockThreads; base < n; base += stride) {   // (block-uniform: every lane reaches the ballots)
        const long long at = base + threadIdx.x;
        int f1 = 0, c1 = 0, v1 = 0, f2 = 0, c2 = 0, v2 = 0;
        if (at < n) {
            const int i = int(at);
            const int cur = rowids[i], prev = i > 0 ? rowids[i - 1] : -1;
            if (cur < 0) atomicOr(&status->flags, kFlagRange);
            else if (i > 0 && prev > cur) atomicOr(&status->flags, kFlagUnsorted);
            else if (i > 0 && prev < 0) { /* reported by the lane before */ }
            else if (cur < batch) {
                if (cur != prev) {   // a run starts
                    begins[cur] = i;
                    if (prev >= 0) ends[prev] = i;
                    f1 = prev + 1;
                    c1 = cur - prev - 1;
                    v1 = i;
                }
                if (i == n - 1) {
                    ends[cur] = n;
                    f2 = cur + 1;
                    c2 = batch - 1 - cur;
                    v2 = n;
                }
            } else if (i == 0) {   // no id in range: every row is [0, 0)
                c1 = batch;
            } else if (prev < batch) {   // the first id out of range
                int lo = 0, hi = i;   // s: the first index of prev's run
                while (lo < hi) {
                    const int mid = lo + (hi - lo) / 2;
                    if (rowids[mid] < prev) lo = mid + 1;
                    else hi = mid;
                }
                ends[prev] = i;
                f1 = prev + 1;
                c1 = batch - 1 - prev;
                v1 = lo;
            }
        }
        wave_fill_rows(f1, c1, v1, begins, ends, gl);
        wave_fill_rows(f2, c2, v2, begins, ends, gl);
    }
}
static __global__ __launch_bounds__(kBlockThreads) void gap_fill_kernel(GapList gl, int32_t* begins, int32_t* ends) {
    const int count = *gl.count < gl.cap ? *gl.count : gl.cap;
    const long long stride = (long long)gridDim.x * kBlockThreads;
    for (int g = 0; g < count; ++g) {
        const int f = gl.entries[3 * g], c = gl.entries[3 * g + 1], v = gl.entries[3 * g + 2];
        for (long long k = (long long)blockIdx.x * kBlockThreads + threadIdx.x; k < c; k += stride) {
            begins[f + k] = v;
            ends[f + k] = v;
        }
    }
}

}  // namespace ovtk
