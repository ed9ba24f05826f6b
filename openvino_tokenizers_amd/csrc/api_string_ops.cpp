// api_string_ops.cpp -- C-ABI entry points of BytesToChars, CharsToBytes, ContribStringSplit and ContribStringJoin; stateless.
// Compiled as HIP (hipcc -x hip).
// Reference behaviour replaced: src/bytes_to_chars.cpp:284-339, src/chars_to_bytes.cpp:31-68, src/contrib_string_ops.cpp:225-343
// and :62-199.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "runtime.hpp"
#include "string_ops_kernels.hpp"

using namespace ovtk;

namespace {

constexpr uint32_t kStopFlags = kFlagOutCapacity | kFlagRange | kFlagOverlap | kFlagTooLong;

int so_begin_status(Workspace& ws, hipStream_t s, RunStatus** st) {
    if (!ws.host_status) return set_error(OVTK_E_HIP, "pinned host allocation failed");
    if (int rc = ws.status.ensure(sizeof(RunStatus))) return rc;
    *st = ws.status.as<RunStatus>();
    OVTK_HIP(hipMemsetAsync(*st, 0, sizeof(RunStatus), s));
    return OVTK_OK;
}

int so_check_mem(int mem) {
    if (mem != OVTK_MEM_HOST && mem != OVTK_MEM_DEVICE) return set_error(OVTK_E_ARG, "mem must be OVTK_MEM_HOST or OVTK_MEM_DEVICE");
    return OVTK_OK;
}

int so_check_strings(const ovtk_strings* s, const char* what) {
    if (!s) return set_error(OVTK_E_ARG, std::string(what) + ": null argument");
    if (s->n < 0 || s->n_chars < 0) return set_error(OVTK_E_ARG, std::string(what) + ": negative size");
    if (s->n >= INT32_MAX || s->n_chars >= INT32_MAX) return set_error(OVTK_E_ARG, std::string(what) + ": tensor sizes must fit int32 offsets");
    if (s->n > 0 && (!s->begins || !s->ends)) return set_error(OVTK_E_ARG, std::string(what) + ": null begins / ends");
    return OVTK_OK;
}

int wave_grid(long long n, int device) {
    return int(std::max<long long>(1, std::min<long long>((n + kTileThreads / kWave - 1) / (kTileThreads / kWave), (long long)device_cu_count(device) * 16)));
}

// what the kernels' flags mean to the caller; out->n_chars = the bytes the call needs (also with OVTK_E_CAPACITY).
// checks_text: the op refuses bytes outside the map's 256 characters with the same flag (CharsToBytes)
int so_report(const RunStatus& st, const char* op, ovtk_strings_out* out, bool checks_text = false) {
    const std::string name(op);
    if (st.flags & kFlagRange)
        return set_error(OVTK_E_RANGE, name + ": an offset outside its tensor or end < begin" + (checks_text ? ", or a byte outside the 256 characters of the map" : ""));
    if (st.flags & kFlagOverlap) return set_error(OVTK_E_UNSUPPORTED, name + ": a row begins before the row in front of it ended");
    if (st.flags & kFlagTooLong) return set_error(OVTK_E_UNSUPPORTED, name + ": the text would reach 2^31 bytes; split the call");
    out->n_chars = st.n_out;
    if (st.flags & kFlagOutCapacity)
        return set_error(OVTK_E_CAPACITY, name + ": output chars buffer too small (" + std::to_string(st.n_out) + " bytes, capacity " + std::to_string(out->chars_capacity) + ")");
    return OVTK_OK;
}

// BytesToChars (to_chars) and CharsToBytes: rows -> covered elements -> count -> two scans (the elements' places in the input
// stretch and in the output) -> a lane per input byte writes.
template <bool TO_CHARS>
int map_call(const char* op, const ovtk_ragged_strings* in, const uint8_t* skips, ovtk_strings_out* out, int mem, int device, void* stream) {
    if (int rc = check_rows(in)) return rc;
    if (int rc = so_check_mem(mem)) return rc;
    if (!out || out->chars_capacity < 0) return set_error(OVTK_E_ARG, std::string(op) + ": bad output");
    const long long n = in->strings.n, n_rows = in->n_rows, n_result = TO_CHARS ? n : n_rows;
    if ((n_rows > 0 && (!in->ragged_begins || !in->ragged_ends)) || (n > 0 && (!in->strings.begins || !in->strings.ends)))
        return set_error(OVTK_E_ARG, std::string(op) + ": null offsets");
    if (n_result > 0 && (!out->begins || !out->ends)) return set_error(OVTK_E_ARG, std::string(op) + ": null output offsets");
    if (int rc = use_device(device)) return rc;
    out->n_chars = 0;
    if (n_result == 0) return OVTK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WorkspaceLease ws(device);
    RunStatus* st = nullptr;
    if (int rc = so_begin_status(*ws.ws, s, &st)) return rc;
    RowsIn d{};
    if (int rc = stage_input(*ws.ws, in, TO_CHARS ? skips : nullptr, mem, s, d)) return rc;
    int e = 0;
    e = e ? e : ws->gen[0].ensure(size_t(n) + 1);
    e = e ? e : ws->gen[1].ensure(size_t(n) * 4 + 4);
    e = e ? e : ws->gen[2].ensure(size_t(n) * 4 + 4);
    e = e ? e : ws->gen[3].ensure(size_t(n + 1) * 4);
    e = e ? e : ws->gen[4].ensure(size_t(n + 1) * 4);
    e = e ? e : ws->tiles.ensure(scan_tiles_bytes(n));
    if (e) return e;
    uint8_t* covered = ws->gen[0].as<uint8_t>();
    int32_t* in_len = ws->gen[1].as<int32_t>();
    uint32_t* out_len = ws->gen[2].as<uint32_t>();
    int32_t* in_off = ws->gen[3].as<int32_t>();
    int32_t* out_off = ws->gen[4].as<int32_t>();
    int32_t *d_b = nullptr, *d_e = nullptr;
    uint8_t* d_c = nullptr;
    if (int rc = out_target(ws->out_a, out->begins, size_t(n_result) * 4, mem, &d_b)) return rc;
    if (int rc = out_target(ws->out_b, out->ends, size_t(n_result) * 4, mem, &d_e)) return rc;
    if (int rc = out_target(ws->out_c, out->chars, size_t(out->chars_capacity), mem, &d_c)) return rc;
    const long long cap = std::min<long long>(out->chars_capacity, INT32_MAX - 1);

    if (n > 0) OVTK_HIP(hipMemsetAsync(covered, 0, size_t(n), s));
    OVTK_LAUNCH(ws->marks, "ragged_cover", ragged_cover_kernel, wave_grid(n_rows, device), kBlockThreads, s, d.ragged_begins, d.ragged_ends, n_rows, n,
                covered, st);
    const MapIn m{d.begins, d.ends, d.chars, covered, TO_CHARS ? d.skips : nullptr, n, (long long)in->strings.n_chars};
    OVTK_LAUNCH(ws->marks, "map_count", map_count_kernel<TO_CHARS>, grid_for_elems(n), kBlockThreads, s, m, in_len, out_len, st);
    launch_scan(ws->marks, "map_in_offsets", s, n, MapInLen{in_len}, MapInOffsets{in_off}, MapInFin{in_off, n, st}, ws->tiles.as<long long>(), st,
                kFlagRange | kFlagOverlap | kFlagTooLong);
    launch_scan(ws->marks, "map_out_offsets", s, n, MapOutLen{out_len}, MapOutOffsets{out_off, covered, TO_CHARS ? d_b : nullptr, TO_CHARS ? d_e : nullptr},
                MapOutFin{out_off, n, cap, st}, ws->tiles.as<long long>(), st, kStopFlags);
    const int grid = int(std::max<long long>(1, std::min<long long>(in->strings.n_chars / kMapBlockBytes + 1, (long long)device_cu_count(device) * 8)));
    OVTK_LAUNCH(ws->marks, TO_CHARS ? "bytes_to_chars" : "chars_to_bytes", map_write_kernel<TO_CHARS>, grid, kBlockThreads, s, m, (const int32_t*)in_off,
                (const int32_t*)out_off, d_c, st, kStopFlags);
    if (!TO_CHARS)
        OVTK_LAUNCH(ws->marks, "fused_rows", fused_rows_kernel, grid_for_elems(n_rows), kBlockThreads, s, d.ragged_begins, d.ragged_ends, n_rows,
                    (const int32_t*)out_off, d_b, d_e, (const RunStatus*)st, kStopFlags);
    if (int rc = finish_status(*ws.ws, s)) return rc;
    if (int rc = so_report(*ws->host_status, op, out, !TO_CHARS)) return rc;
    e = 0;
    e = e ? e : copy_back(out->begins, d_b, size_t(n_result) * 4, mem, s);
    e = e ? e : copy_back(out->ends, d_e, size_t(n_result) * 4, mem, s);
    e = e ? e : copy_back(out->chars, d_c, size_t(out->n_chars), mem, s);
    if (e) return e;
    if (mem == OVTK_MEM_HOST) OVTK_HIP(hipStreamSynchronize(s));
    return OVTK_OK;
}

// shape (host memory) -> its element count; < 0: a negative dimension or more than int32 offsets can address
long long shape_elements(const int64_t* shape, int rank) {
    long long n = 1;
    for (int d = 0; d < rank; ++d) {
        if (shape[d] < 0 || shape[d] >= INT32_MAX) return -1;
        n *= shape[d];
        if (n >= INT32_MAX) {   // (a zero further on still makes the tensor empty)
            for (int k = d + 1; k < rank; ++k)
                if (shape[k] == 0) return 0;
            return -1;
        }
    }
    return n;
}

}  // namespace

extern "C" {

int ovtk_bytes_to_chars(const ovtk_ragged_strings* in, const uint8_t* skips, ovtk_strings_out* out, int mem, int device, void* stream) {
    return map_call<true>("BytesToChars", in, skips, out, mem, device, stream);
}

int ovtk_chars_to_bytes(const ovtk_ragged_strings* in, ovtk_strings_out* out, int mem, int device, void* stream) {
    return map_call<false>("CharsToBytes", in, nullptr, out, mem, device, stream);
}

// ------------------------------------------------------------------------------- ContribStringSplit
int ovtk_contrib_string_split(const ovtk_strings* in, const int64_t* shape, int rank, const uint8_t* delim, int64_t delim_len, int skip_empty,
                              ovtk_string_split_out* out, int mem, int device, void* stream) {
    if (int rc = so_check_strings(in, "contrib_string_split input")) return rc;
    if (int rc = so_check_mem(mem)) return rc;
    if (rank < 0 || (rank > 0 && !shape)) return set_error(OVTK_E_ARG, "contrib_string_split: bad shape");
    if (rank > kSplitMaxRank) return set_error(OVTK_E_UNSUPPORTED, "ContribStringSplit: input ranks 0..8 are supported");
    if (delim_len < 0 || delim_len >= INT32_MAX || (delim_len > 0 && !delim)) return set_error(OVTK_E_ARG, "contrib_string_split: bad delimiter");
    if (!out || !out->dense_shape || out->values_capacity < 0 || out->chars_capacity < 0) return set_error(OVTK_E_ARG, "contrib_string_split: bad output");
    if (shape_elements(shape, rank) != in->n) return set_error(OVTK_E_ARG, "contrib_string_split: the shape does not have the tensor's element count");
    if (int rc = use_device(device)) return rc;
    for (int d = 0; d < rank; ++d) out->dense_shape[d] = shape[d];
    out->dense_shape[rank] = 0;
    out->n_values = 0;
    out->n_chars = 0;
    const long long n = in->n;
    if (n == 0) return OVTK_OK;
    const int dlen = int(delim_len);
    // a border: a proper prefix of the delimiter that is also its suffix (the prefix function's last value)
    std::vector<int> pi(size_t(std::max(dlen, 1)), 0);
    for (int k = 1; k < dlen; ++k) {
        int j = pi[k - 1];
        while (j > 0 && delim[k] != delim[j]) j = pi[j - 1];
        pi[k] = delim[k] == delim[j] ? j + 1 : j;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    WorkspaceLease ws(device);
    RunStatus* st = nullptr;
    if (int rc = so_begin_status(*ws.ws, s, &st)) return rc;
    SplitIn p{};
    if (int rc = in_source(ws->in_begins, in->begins, size_t(n) * 4, mem, s, &p.begins)) return rc;
    if (int rc = in_source(ws->in_ends, in->ends, size_t(n) * 4, mem, s, &p.ends)) return rc;
    if (int rc = in_source(ws->in_chars, in->chars, size_t(in->n_chars), mem, s, &p.chars)) return rc;
    if (int rc = ws->gen[0].upload(delim, size_t(dlen), s)) return rc;   // (the delimiter: host memory)
    p.n = n;
    p.n_chars = in->n_chars;
    p.delim = ws->gen[0].as<uint8_t>();
    p.dlen = dlen;
    p.bordered = dlen > 1 && pi[size_t(dlen) - 1] > 0;
    p.skip_empty = skip_empty != 0;
    p.rank = rank;
    for (int d = rank - 1; d >= 0; --d) p.stride[d] = d == rank - 1 ? 1 : p.stride[d + 1] * shape[d + 1];
    int e = 0;
    for (int k = 1; k <= 4; ++k) e = e ? e : ws->gen[k].ensure(size_t(n) * 4);
    e = e ? e : ws->tiles.ensure(scan_tiles_bytes(n));
    if (e) return e;
    int32_t *tok_cnt = ws->gen[1].as<int32_t>(), *byte_cnt = ws->gen[2].as<int32_t>(), *tok_off = ws->gen[3].as<int32_t>(), *byte_off = ws->gen[4].as<int32_t>();
    SplitOut o{};
    const size_t idx_bytes = size_t(out->values_capacity) * size_t(rank + 1) * 8;
    if (int rc = out_target(ws->out_a, out->indices, idx_bytes, mem, &o.indices)) return rc;
    if (int rc = out_target(ws->out_b, out->begins, size_t(out->values_capacity) * 4, mem, &o.begins)) return rc;
    if (int rc = out_target(ws->out_c, out->ends, size_t(out->values_capacity) * 4, mem, &o.ends)) return rc;
    if (int rc = out_target(ws->out_d, out->chars, size_t(out->chars_capacity), mem, &o.chars)) return rc;
    const int grid = wave_grid(n, device);
    OVTK_LAUNCH(ws->marks, "split_count", each_wave_kernel<SplitCount>, grid, kTileThreads, s, n, SplitCount{p, tok_cnt, byte_cnt, st}, (const RunStatus*)nullptr, 0u);
    launch_scan(ws->marks, "split_value_offsets", s, n, MapInLen{tok_cnt}, MapInOffsets{tok_off}, SplitValuesFin{st, std::min<long long>(out->values_capacity, INT32_MAX - 1)},
                ws->tiles.as<long long>(), st, kStopFlags);
    launch_scan(ws->marks, "split_char_offsets", s, n, MapInLen{byte_cnt}, MapInOffsets{byte_off}, SplitCharsFin{st, std::min<long long>(out->chars_capacity, INT32_MAX - 1)},
                ws->tiles.as<long long>(), st, kStopFlags);
    OVTK_LAUNCH(ws->marks, "string_split", each_wave_kernel<SplitWrite>, grid, kTileThreads, s, n, SplitWrite{p, tok_off, byte_off, o}, (const RunStatus*)st, kStopFlags);
    if (int rc = finish_status(*ws.ws, s)) return rc;
    const RunStatus& h = *ws->host_status;
    if (h.flags & kFlagRange) return set_error(OVTK_E_RANGE, "ContribStringSplit: end < begin, or an offset outside the chars tensor");
    if (h.flags & kFlagTooLong) return set_error(OVTK_E_UNSUPPORTED, "ContribStringSplit: 2^31 values or bytes; split the call");
    out->n_values = h.n_exact;
    out->n_chars = h.n_out;
    out->dense_shape[rank] = h.n_items;
    if (h.flags & kFlagOutCapacity)
        return set_error(OVTK_E_CAPACITY, "ContribStringSplit: output buffers too small (" + std::to_string(h.n_exact) + " values, " + std::to_string(h.n_out) + " bytes)");
    e = 0;
    e = e ? e : copy_back(out->indices, o.indices, size_t(out->n_values) * size_t(rank + 1) * 8, mem, s);
    e = e ? e : copy_back(out->begins, o.begins, size_t(out->n_values) * 4, mem, s);
    e = e ? e : copy_back(out->ends, o.ends, size_t(out->n_values) * 4, mem, s);
    e = e ? e : copy_back(out->chars, o.chars, size_t(out->n_chars), mem, s);
    if (e) return e;
    if (mem == OVTK_MEM_HOST) OVTK_HIP(hipStreamSynchronize(s));
    return OVTK_OK;
}

// ------------------------------------------------------------------------------- ContribStringJoin
int ovtk_contrib_string_join(const ovtk_strings* in, const int64_t* shape, int rank, const uint8_t* sep, int64_t sep_len, int64_t axis, ovtk_strings_out* out,
                             int64_t* n_out, int mem, int device, void* stream) {
    if (int rc = so_check_strings(in, "contrib_string_join input")) return rc;
    if (int rc = so_check_mem(mem)) return rc;
    if (rank < 0 || (rank > 0 && !shape)) return set_error(OVTK_E_ARG, "contrib_string_join: bad shape");
    if (sep_len < 0 || sep_len >= INT32_MAX || (sep_len > 0 && !sep)) return set_error(OVTK_E_ARG, "contrib_string_join: bad separator");
    if (!out || !n_out || out->chars_capacity < 0) return set_error(OVTK_E_ARG, "contrib_string_join: bad output");
    if (shape_elements(shape, rank) != in->n) return set_error(OVTK_E_ARG, "contrib_string_join: the shape does not have the tensor's element count");
    long long outer = 1, axis_size = 1, inner = 1;   // (rank 0: the one string)
    if (rank > 0) {
        if (axis < 0) axis += rank;
        if (axis < 0 || axis >= rank) return set_error(OVTK_E_ARG, "ContribStringJoin axis out of range");   // contrib_string_ops.cpp:91
        axis_size = shape[axis];
        for (int d = 0; d < rank; ++d) {   // (saturating: with an axis of size 0 the other dimensions are not bounded by the element count)
            if (d == axis) continue;
            long long& side = d < axis ? outer : inner;
            side = std::min<long long>(side * shape[d], INT32_MAX);
        }
    }
    const long long n_result = outer * inner;
    if (n_result >= INT32_MAX) return set_error(OVTK_E_ARG, "contrib_string_join: tensor sizes must fit int32 offsets");
    if (int rc = use_device(device)) return rc;
    *n_out = n_result;
    out->n_chars = 0;
    if (n_result == 0) return OVTK_OK;
    if (!out->begins || !out->ends) return set_error(OVTK_E_ARG, "contrib_string_join: null output offsets");
    hipStream_t s = static_cast<hipStream_t>(stream);
    WorkspaceLease ws(device);
    RunStatus* st = nullptr;
    if (int rc = so_begin_status(*ws.ws, s, &st)) return rc;
    JoinIn p{};
    if (int rc = in_source(ws->in_begins, in->begins, size_t(in->n) * 4, mem, s, &p.begins)) return rc;
    if (int rc = in_source(ws->in_ends, in->ends, size_t(in->n) * 4, mem, s, &p.ends)) return rc;
    if (int rc = in_source(ws->in_chars, in->chars, size_t(in->n_chars), mem, s, &p.chars)) return rc;
    if (int rc = ws->gen[0].upload(sep, size_t(sep_len), s)) return rc;   // (the separator: host memory)
    p.n_chars = in->n_chars;
    p.sep = ws->gen[0].as<uint8_t>();
    p.slen = int(sep_len);
    p.axis_size = axis_size;
    p.inner = inner;
    if (int rc = ws->gen[1].ensure(size_t(n_result) * sizeof(long long))) return rc;
    if (int rc = ws->tiles.ensure(scan_tiles_bytes(n_result))) return rc;
    long long* lens = ws->gen[1].as<long long>();
    int32_t *d_b = nullptr, *d_e = nullptr;
    uint8_t* d_c = nullptr;
    if (int rc = out_target(ws->out_a, out->begins, size_t(n_result) * 4, mem, &d_b)) return rc;
    if (int rc = out_target(ws->out_b, out->ends, size_t(n_result) * 4, mem, &d_e)) return rc;
    if (int rc = out_target(ws->out_c, out->chars, size_t(out->chars_capacity), mem, &d_c)) return rc;
    const int grid = wave_grid(n_result, device);
    OVTK_LAUNCH(ws->marks, "join_count", each_wave_kernel<JoinCount>, grid, kTileThreads, s, n_result, JoinCount{p, lens, st}, (const RunStatus*)nullptr, 0u);
    launch_scan(ws->marks, "join_offsets", s, n_result, JoinLen{lens}, JoinOffsets{d_b, d_e}, SplitCharsFin{st, std::min<long long>(out->chars_capacity, INT32_MAX - 1)},
                ws->tiles.as<long long>(), st, kStopFlags);
    OVTK_LAUNCH(ws->marks, "string_join", each_wave_kernel<JoinWrite>, grid, kTileThreads, s, n_result, JoinWrite{p, d_b, d_c}, (const RunStatus*)st, kStopFlags);
    if (int rc = finish_status(*ws.ws, s)) return rc;
    if (int rc = so_report(*ws->host_status, "ContribStringJoin", out)) return rc;
    int e = 0;
    e = e ? e : copy_back(out->begins, d_b, size_t(n_result) * 4, mem, s);
    e = e ? e : copy_back(out->ends, d_e, size_t(n_result) * 4, mem, s);
    e = e ? e : copy_back(out->chars, d_c, size_t(out->n_chars), mem, s);
    if (e) return e;
    if (mem == OVTK_MEM_HOST) OVTK_HIP(hipStreamSynchronize(s));
    return OVTK_OK;
}

}  // extern "C"
