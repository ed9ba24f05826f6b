// api_charsmap.cpp -- C-ABI entry points of CharsMapNormalization / NormalizeUnicode / CaseFold.  Compiled as HIP (hipcc -x hip).
// Reference behaviour replaced: src/charsmap_normalization.cpp:34-69, src/normalize_unicode.cpp:32-62, src/case_fold.cpp:34-73,
// src/utils.cpp:178-234 (evaluate_normalization_helper).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "charsmap_handle.hpp"
#include "charsmap_kernels.hpp"
#include "ops_kernels.hpp"
#include "runtime.hpp"

using namespace ovtk;

namespace {

int charsmap_begin_status(Workspace& ws, hipStream_t s, RunStatus** st) {
    if (!ws.host_status) return set_error(OVTK_E_HIP, "pinned host allocation failed");
    if (int rc = ws.status.ensure(sizeof(RunStatus))) return rc;
    *st = ws.status.as<RunStatus>();
    OVTK_HIP(hipMemsetAsync(*st, 0, sizeof(RunStatus), s));
    return OVTK_OK;
}

int charsmap_check_strings(const ovtk_strings* s, const ovtk_strings_out* out, const char* what) {
    if (!s || !out) return set_error(OVTK_E_ARG, std::string(what) + ": null argument");
    if (s->n < 0 || s->n_chars < 0 || out->chars_capacity < 0) return set_error(OVTK_E_ARG, std::string(what) + ": negative size");
    if (s->n >= INT32_MAX || s->n_chars >= INT32_MAX) return set_error(OVTK_E_ARG, std::string(what) + ": tensor sizes must fit int32 offsets");
    return OVTK_OK;
}

uint32_t unit_offset(uint32_t u) { return (u >> 10) << ((u & 0x200u) >> 6); }

// The record of the replacement s[0, len) (charsmap_kernels.hpp: cm_pack).
uint2 replacement_record(const uint8_t* s, uint32_t len, bool symbol_is_unit) {
    uint32_t ls = 0, ns = 0, tail = 0;
    while (ls < len && s[ls] == ' ') ++ls;
    for (uint32_t k = 0; k < len; ++k) ns += s[k] == ' ';
    uint32_t q = len;
    for (;;) {
        if (q >= 1 && s[q - 1] == ' ') q -= 1;
        else if (symbol_is_unit && q >= 3 && s[q - 3] == 0xE2 && s[q - 2] == 0x96 && s[q - 1] == 0x81) q -= 3;
        else break;
        ++tail;
    }
    return uint2{cm_pack(len, ls, ns, len > 0 && s[len - 1] == ' ', q == 0), tail};
}

}  // namespace

extern "C" {

int ovtk_charsmap_create(const uint8_t* blob, int64_t blob_len, const ovtk_charsmap_params* p, int device, ovtk_charsmap** out) {
    if (!p || !out || blob_len < 0 || (blob_len > 0 && !blob)) return set_error(OVTK_E_ARG, "charsmap: bad argument");
    if (int rc = use_device(device)) return rc;
    auto h = std::make_unique<ovtk_charsmap>();
    h->device = device;
    h->dev.add_dummy = p->add_dummy_prefix != 0;
    h->dev.remove_extra = p->remove_extra_whitespaces != 0;
    h->dev.escape = p->escape_whitespaces != 0;
    int64_t ratio = 1;
    if (blob_len > 0) {
        if (blob_len < 4) return set_error(OVTK_E_UNSUPPORTED, "charsmap: the blob is shorter than its size field");
        uint32_t trie_size = 0;
        std::memcpy(&trie_size, blob, 4);
        if (int64_t(trie_size) + 4 > blob_len) return set_error(OVTK_E_UNSUPPORTED, "charsmap: the blob's trie size reaches past its end");
        if (trie_size % 4 != 0 || trie_size == 0) return set_error(OVTK_E_UNSUPPORTED, "charsmap: the blob's trie size is not a positive multiple of 4");
        const uint32_t n_units = trie_size / 4;
        std::vector<uint32_t> units(n_units);
        std::memcpy(units.data(), blob + 4, trie_size);
        const uint8_t* strings = blob + 4 + trie_size;
        const int64_t n_strings = blob_len - 4 - trie_size;
        if (n_strings >= INT32_MAX) return set_error(OVTK_E_UNSUPPORTED, "charsmap: more than 2^31 bytes of replacement strings");
        std::vector<uint2> meta(size_t(std::max<int64_t>(n_strings, 1)), uint2{cm_pack(0, 0, 0, false, true), 0});
        // every key, as the kernel will walk to it: the bytes keys start with, the values, the largest replacement / key ratio
        struct Node { uint32_t pos, depth; };
        std::vector<Node> stack;
        if (unit_offset(units[0]) < n_units) stack.push_back(Node{unit_offset(units[0]), 0});
        const bool both = h->dev.remove_extra && h->dev.escape;
        uint64_t steps = 0;
        while (!stack.empty()) {
            const Node at = stack.back();
            stack.pop_back();
            if (++steps > 256ull * n_units + 4096 || at.depth > 4096) return set_error(OVTK_E_UNSUPPORTED, "charsmap: the walk over the blob's unit array does not end (a cycle)");
            for (uint32_t c = 0; c < 256; ++c) {
                const uint32_t child = at.pos ^ c;
                if (child >= n_units || (units[child] & 0x800000FFu) != c) continue;
                const uint32_t u = units[child], next = child ^ unit_offset(u);
                if (next >= n_units) continue;   // (where the kernel's walk stops too)
                if (at.depth == 0) h->dev.first[c >> 6] |= 1ull << (c & 63);
                if ((u >> 8) & 1u) {
                    const uint32_t value = units[next] & 0x7FFFFFFFu;
                    const void* nul = int64_t(value) < n_strings ? std::memchr(strings + value, 0, size_t(n_strings - value)) : nullptr;
                    if (!nul) return set_error(OVTK_E_UNSUPPORTED, "charsmap: a key's value points outside the replacement strings");
                    const uint32_t len = uint32_t(static_cast<const uint8_t*>(nul) - (strings + value));
                    if (len > uint32_t(kCmMaxRepBytes)) return set_error(OVTK_E_UNSUPPORTED, "charsmap: a replacement is longer than 1 023 bytes");
                    const uint8_t* r = strings + value;
                    if (both && ((len >= 1 && r[len - 1] == 0xE2) || (len >= 2 && r[len - 2] == 0xE2 && r[len - 1] == 0x96)))
                        return set_error(OVTK_E_UNSUPPORTED, "charsmap: a replacement ends in the first bytes of U+2581 (unsupported with remove_extra_whitespaces and escape_whitespaces)");
                    meta[value] = replacement_record(r, len, h->dev.escape != 0);
                    ratio = std::max<int64_t>(ratio, (int64_t(len) + at.depth) / (at.depth + 1));   // ceil(len / key bytes)
                }
                stack.push_back(Node{next, at.depth + 1});
            }
        }
        if (int rc = h->units.upload(units.data(), size_t(trie_size))) return rc;
        const uint8_t none = 0;
        if (int rc = h->strings.upload(n_strings ? strings : &none, size_t(std::max<int64_t>(n_strings, 1)))) return rc;
        if (int rc = h->meta.upload(meta.data(), meta.size() * sizeof(uint2))) return rc;
        h->dev.units = h->units.as<uint32_t>();
        h->dev.n_units = n_units;
        h->dev.strings = h->strings.as<uint8_t>();
        h->dev.meta = h->meta.as<uint2>();
        h->dev.n_strings = uint32_t(n_strings);
        OVTK_HIP(hipStreamSynchronize(nullptr));
    }
    h->per_byte = std::max<int64_t>(3, ratio * (h->dev.escape ? 3 : 1));
    *out = h.release();
    return OVTK_OK;
}

void ovtk_charsmap_destroy(ovtk_charsmap* h) { delete h; }

int64_t ovtk_charsmap_bound(ovtk_charsmap* h, int64_t n, int64_t n_chars) {
    if (!h || n < 0 || n_chars < 0) return -1;
    return n_chars * h->per_byte + 3 * n;
}

int ovtk_charsmap_run(ovtk_charsmap* h, const ovtk_strings* in, const uint8_t* skips, ovtk_strings_out* out, int mem, void* stream) {
    if (!h) return set_error(OVTK_E_ARG, "charsmap: null handle");
    if (int rc = charsmap_check_strings(in, out, "charsmap")) return rc;
    if (mem != OVTK_MEM_HOST && mem != OVTK_MEM_DEVICE) return set_error(OVTK_E_ARG, "mem must be OVTK_MEM_HOST or OVTK_MEM_DEVICE");
    if (int rc = use_device(h->device)) return rc;
    out->n_chars = 0;
    if (in->n == 0) return OVTK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WorkspaceLease ws(h->device);
    RunStatus* st = nullptr;
    if (int rc = charsmap_begin_status(*ws.ws, s, &st)) return rc;
    const int32_t *b = nullptr, *e = nullptr;
    const uint8_t *c = nullptr, *sk = nullptr;
    if (int rc = in_source(ws->in_begins, in->begins, size_t(in->n) * 4, mem, s, &b)) return rc;
    if (int rc = in_source(ws->in_ends, in->ends, size_t(in->n) * 4, mem, s, &e)) return rc;
    if (int rc = in_source(ws->in_chars, in->chars, size_t(in->n_chars), mem, s, &c)) return rc;
    if (skips)
        if (int rc = in_source(ws->in_skips, skips, size_t(in->n), mem, s, &sk)) return rc;
    int32_t *d_b = nullptr, *d_e = nullptr;
    uint8_t* d_c = nullptr;
    if (int rc = out_target(ws->out_c, out->begins, size_t(in->n) * 4, mem, &d_b)) return rc;
    if (int rc = out_target(ws->out_d, out->ends, size_t(in->n) * 4, mem, &d_e)) return rc;
    if (int rc = out_target(ws->out_e, out->chars, size_t(std::max<int64_t>(out->chars_capacity, 1)), mem, &d_c)) return rc;
    if (int rc = ws->gen[6].ensure(size_t(in->n) * 4)) return rc;
    int32_t* lens = ws->gen[6].as<int32_t>();
    if ((in->n + kTileElems - 1) / kTileElems > INT32_MAX) return set_error(OVTK_E_UNSUPPORTED, "too many strings for one call; split it");
    if (int rc = ws->tiles.ensure(scan_tiles_bytes(in->n))) return rc;
    OVTK_LAUNCH(ws->marks, "check_strings", check_strings_kernel, grid_for_elems(in->n), kBlockThreads, s, b, e, (long long)in->n,
                (long long)in->n_chars, st);
    // a wave per string counts -> scan of the filed lengths -> a wave per string writes
    const int wave_grid = int(std::min<long long>((in->n + kTileThreads / kWave - 1) / (kTileThreads / kWave), (long long)device_cu_count(h->device) * 16));
    OVTK_LAUNCH(ws->marks, "charsmap_count", each_wave_kernel<CmRow<false>>, wave_grid, kTileThreads, s, (long long)in->n,
                (CmRow<false>{h->dev, b, e, c, (long long)in->n_chars, sk, lens, nullptr, nullptr}), (const RunStatus*)st, kFlagRange);
    launch_scan(ws->marks, "charsmap_offsets", s, in->n, FiledLen{lens}, RowOffsets{d_b, d_e, 0},
                CharsFin{st, (long long)std::min<int64_t>(out->chars_capacity, INT32_MAX - 1)}, ws->tiles.as<long long>(), st, kFlagRange);
    OVTK_LAUNCH(ws->marks, "charsmap_write", each_wave_kernel<CmRow<true>>, wave_grid, kTileThreads, s, (long long)in->n,
                (CmRow<true>{h->dev, b, e, c, (long long)in->n_chars, sk, lens, d_b, d_c}), (const RunStatus*)st, kFlagOutCapacity | kFlagRange);
    if (int rc = finish_status(*ws.ws, s)) return rc;
    if (ws->host_status->flags & kFlagRange) return set_error(OVTK_E_RANGE, "input begins/ends index outside the chars tensor");
    if (ws->host_status->flags & kFlagOutCapacity) {
        out->n_chars = ws->host_status->n_out;
        if (ws->host_status->n_out >= INT32_MAX - 1) return set_error(OVTK_E_UNSUPPORTED, "CharsMapNormalization: the output reaches 2^31 bytes; split the call");
        return set_error(OVTK_E_CAPACITY, "CharsMapNormalization: output chars buffer too small (" + std::to_string(ws->host_status->n_out) +
                                              " bytes, capacity " + std::to_string(out->chars_capacity) + ")");
    }
    out->n_chars = ws->host_status->n_out;
    int err = 0;
    err = err ? err : copy_back(out->begins, d_b, size_t(in->n) * 4, mem, s);
    err = err ? err : copy_back(out->ends, d_e, size_t(in->n) * 4, mem, s);
    err = err ? err : copy_back(out->chars, d_c, size_t(out->n_chars), mem, s);
    if (err) return err;
    if (mem == OVTK_MEM_HOST) OVTK_HIP(hipStreamSynchronize(s));
    return OVTK_OK;
}

int ovtk_case_fold_ascii(const ovtk_strings* in, int lower, ovtk_strings_out* out, int mem, int device, void* stream) {
    if (int rc = charsmap_check_strings(in, out, "case_fold")) return rc;
    if (mem != OVTK_MEM_HOST && mem != OVTK_MEM_DEVICE) return set_error(OVTK_E_ARG, "mem must be OVTK_MEM_HOST or OVTK_MEM_DEVICE");
    if (int rc = use_device(device)) return rc;
    out->n_chars = 0;
    if (in->n == 0) return OVTK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WorkspaceLease ws(device);
    RunStatus* st = nullptr;
    if (int rc = charsmap_begin_status(*ws.ws, s, &st)) return rc;
    const int32_t *b = nullptr, *e = nullptr;
    const uint8_t* c = nullptr;
    if (int rc = in_source(ws->in_begins, in->begins, size_t(in->n) * 4, mem, s, &b)) return rc;
    if (int rc = in_source(ws->in_ends, in->ends, size_t(in->n) * 4, mem, s, &e)) return rc;
    if (int rc = in_source(ws->in_chars, in->chars, size_t(in->n_chars), mem, s, &c)) return rc;
    int32_t *d_b = nullptr, *d_e = nullptr;
    uint8_t* d_c = nullptr;
    if (int rc = out_target(ws->out_c, out->begins, size_t(in->n) * 4, mem, &d_b)) return rc;
    if (int rc = out_target(ws->out_d, out->ends, size_t(in->n) * 4, mem, &d_e)) return rc;
    if (int rc = out_target(ws->out_e, out->chars, size_t(std::max<int64_t>(out->chars_capacity, 1)), mem, &d_c)) return rc;
    if ((in->n + kTileElems - 1) / kTileElems > INT32_MAX) return set_error(OVTK_E_UNSUPPORTED, "too many strings for one call; split it");
    if (int rc = ws->tiles.ensure(scan_tiles_bytes(in->n))) return rc;
    OVTK_LAUNCH(ws->marks, "check_strings", check_strings_kernel, grid_for_elems(in->n), kBlockThreads, s, b, e, (long long)in->n,
                (long long)in->n_chars, st);
    launch_scan(ws->marks, "case_fold_offsets", s, in->n, CaseFoldLen{b, e, (long long)in->n_chars}, RowOffsets{d_b, d_e, 0},
                CharsFin{st, (long long)std::min<int64_t>(out->chars_capacity, INT32_MAX - 1)}, ws->tiles.as<long long>(), st, kFlagRange);
    const int wave_grid = int(std::min<long long>((in->n + kTileThreads / kWave - 1) / (kTileThreads / kWave), (long long)device_cu_count(device) * 16));
    const CaseFoldWrite fold{b, e, c, d_b, d_c, lower ? 0x41u : 0x61u, lower ? 0x5Au : 0x7Au, lower ? 32 : -32};
    OVTK_LAUNCH(ws->marks, "case_fold_write", each_wave_kernel<CaseFoldWrite>, wave_grid, kTileThreads, s, (long long)in->n, fold,
                (const RunStatus*)st, kFlagOutCapacity | kFlagRange);
    if (int rc = finish_status(*ws.ws, s)) return rc;
    if (ws->host_status->flags & kFlagRange) return set_error(OVTK_E_RANGE, "input begins/ends index outside the chars tensor");
    out->n_chars = ws->host_status->n_out;
    if (ws->host_status->flags & kFlagOutCapacity)
        return set_error(OVTK_E_CAPACITY, "CaseFold: output chars buffer too small (" + std::to_string(ws->host_status->n_out) + " bytes)");
    int err = 0;
    err = err ? err : copy_back(out->begins, d_b, size_t(in->n) * 4, mem, s);
    err = err ? err : copy_back(out->ends, d_e, size_t(in->n) * 4, mem, s);
    err = err ? err : copy_back(out->chars, d_c, size_t(out->n_chars), mem, s);
    if (err) return err;
    if (mem == OVTK_MEM_HOST) OVTK_HIP(hipStreamSynchronize(s));
    return OVTK_OK;
}

}  // extern "C"
