// api_tf_ops.cpp -- C-ABI entry points of the three stateless ops of the reference's TensorFlow front end: StringToHashBucket,
// EqualStr, RaggedToRagged.  Compiled as HIP (hipcc -x hip).
// Reference behaviour replaced: src/string_to_hash_bucket.cpp:204-220 (hash64 :128-182), src/equal_str.cpp:29-61,
// src/ragged_to_ragged.cpp:43-98.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "api_common.hpp"
#include "runtime.hpp"
#include "tf_ops_kernels.hpp"

using namespace ovtk;

namespace {

int tf_check_strings(const ovtk_strings* s, const char* what) {
    if (!s) return set_error(OVTK_E_ARG, std::string(what) + ": null argument");
    if (s->n < 0 || s->n_chars < 0) return set_error(OVTK_E_ARG, std::string(what) + ": negative size");
    if (s->n >= INT32_MAX || s->n_chars >= INT32_MAX) return set_error(OVTK_E_ARG, std::string(what) + ": tensor sizes must fit int32 offsets");
    if (s->n > 0 && (!s->begins || !s->ends)) return set_error(OVTK_E_ARG, std::string(what) + ": null begins / ends");
    return OVTK_OK;
}

int tf_begin_status(Workspace& ws, hipStream_t s, RunStatus** st) {
    if (!ws.host_status) return set_error(OVTK_E_HIP, "pinned host allocation failed");
    if (int rc = ws.status.ensure(sizeof(RunStatus))) return rc;
    *st = ws.status.as<RunStatus>();
    OVTK_HIP(hipMemsetAsync(*st, 0, sizeof(RunStatus), s));
    return OVTK_OK;
}

// one string tensor on the device: the caller's pointers, or staged copies in the three buffers given
int stage_strings(const ovtk_strings* in, DevBuf& sb, DevBuf& se, DevBuf& sc, int mem, hipStream_t s, const int32_t** b, const int32_t** e,
                  const uint8_t** c) {
    if (int rc = in_source(sb, in->begins, size_t(in->n) * 4, mem, s, b)) return rc;
    if (int rc = in_source(se, in->ends, size_t(in->n) * 4, mem, s, e)) return rc;
    return in_source(sc, in->chars, size_t(in->n_chars), mem, s, c);
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------- StringToHashBucket
int ovtk_string_to_hash_bucket(const ovtk_strings* in, int64_t num_buckets, int64_t* out, int mem, int device, void* stream) {
    if (int rc = tf_check_strings(in, "string_to_hash_bucket input")) return rc;
    if (num_buckets <= 0) return set_error(OVTK_E_ARG, "num_buckets attribute must be positive");   // string_to_hash_bucket.cpp:199
    if (mem != OVTK_MEM_HOST && mem != OVTK_MEM_DEVICE) return set_error(OVTK_E_ARG, "mem must be OVTK_MEM_HOST or OVTK_MEM_DEVICE");
    if (in->n > 0 && !out) return set_error(OVTK_E_ARG, "string_to_hash_bucket: null output");
    if (int rc = use_device(device)) return rc;
    if (in->n == 0) return OVTK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WorkspaceLease ws(device);
    RunStatus* st = nullptr;
    if (int rc = tf_begin_status(*ws.ws, s, &st)) return rc;
    const int32_t *b = nullptr, *e = nullptr;
    const uint8_t* c = nullptr;
    if (int rc = stage_strings(in, ws->in_begins, ws->in_ends, ws->in_chars, mem, s, &b, &e, &c)) return rc;
    int64_t* d_out = nullptr;
    if (int rc = out_target(ws->out_a, out, size_t(in->n) * 8, mem, &d_out)) return rc;
    OVTK_LAUNCH(ws->marks, "string_hash", string_hash_kernel, grid_for_elems(in->n), kBlockThreads, s, b, e, c, (long long)in->n,
                (long long)in->n_chars, uint64_t(num_buckets), d_out, st);
    if (int rc = finish_status(*ws.ws, s)) return rc;
    if (ws->host_status->flags & kFlagRange) return set_error(OVTK_E_RANGE, "string_to_hash_bucket: begins > ends, or an offset outside the chars tensor");
    if (int rc = copy_back(out, d_out, size_t(in->n) * 8, mem, s)) return rc;
    if (mem == OVTK_MEM_HOST) OVTK_HIP(hipStreamSynchronize(s));
    return OVTK_OK;
}

// ------------------------------------------------------------------------------- EqualStr
int ovtk_equal_str(const ovtk_strings* a, const ovtk_strings* b, int32_t* out, int64_t capacity, int64_t* n_out, int mem, int device,
                   void* stream) {
    if (int rc = tf_check_strings(a, "equal_str first operand")) return rc;
    if (int rc = tf_check_strings(b, "equal_str second operand")) return rc;
    if (!n_out || capacity < 0) return set_error(OVTK_E_ARG, "equal_str: bad output");
    if (mem != OVTK_MEM_HOST && mem != OVTK_MEM_DEVICE) return set_error(OVTK_E_ARG, "mem must be OVTK_MEM_HOST or OVTK_MEM_DEVICE");
    const int64_t n = (a->n == 0 || b->n == 0) ? 0 : std::max(a->n, b->n);   // equal_str.cpp:42
    *n_out = n;
    if (capacity < n)
        return set_error(OVTK_E_CAPACITY, "EqualStr: output buffer too small (" + std::to_string(n) + " elements, capacity " + std::to_string(capacity) + ")");
    if (n > 0 && !out) return set_error(OVTK_E_ARG, "equal_str: null output");
    if (int rc = use_device(device)) return rc;
    if (n == 0) return OVTK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WorkspaceLease ws(device);
    RunStatus* st = nullptr;
    if (int rc = tf_begin_status(*ws.ws, s, &st)) return rc;
    EqualOperand da{nullptr, nullptr, nullptr, a->n, a->n_chars}, db{nullptr, nullptr, nullptr, b->n, b->n_chars};
    if (int rc = stage_strings(a, ws->in_begins, ws->in_ends, ws->in_chars, mem, s, &da.begins, &da.ends, &da.chars)) return rc;
    if (int rc = stage_strings(b, ws->gen[0], ws->gen[1], ws->gen[2], mem, s, &db.begins, &db.ends, &db.chars)) return rc;
    int32_t* d_out = nullptr;
    if (int rc = out_target(ws->out_a, out, size_t(n) * 4, mem, &d_out)) return rc;
    OVTK_LAUNCH(ws->marks, "equal_str", equal_str_kernel, grid_for_elems(n), kBlockThreads, s, da, db, (long long)n, d_out, st);
    if (int rc = finish_status(*ws.ws, s)) return rc;
    if (ws->host_status->flags & kFlagRange) return set_error(OVTK_E_RANGE, "equal_str: begins / ends index outside their chars tensor");
    if (int rc = copy_back(out, d_out, size_t(n) * 4, mem, s)) return rc;
    if (mem == OVTK_MEM_HOST) OVTK_HIP(hipStreamSynchronize(s));
    return OVTK_OK;
}

// ------------------------------------------------------------------------------- RaggedToRagged
int ovtk_ragged_to_ragged(const int32_t* rowids, int64_t n_rowids, int32_t batch_size, int32_t* out_begins, int32_t* out_ends, int mem,
                          int device, void* stream) {
    if (n_rowids < 0 || n_rowids >= INT32_MAX || (n_rowids > 0 && !rowids)) return set_error(OVTK_E_ARG, "ragged_to_ragged: bad rowids");
    if (batch_size < 0) return set_error(OVTK_E_ARG, "ragged_to_ragged: negative first_dim_size");
    if (batch_size > 0 && (!out_begins || !out_ends)) return set_error(OVTK_E_ARG, "ragged_to_ragged: null output");
    if (mem != OVTK_MEM_HOST && mem != OVTK_MEM_DEVICE) return set_error(OVTK_E_ARG, "mem must be OVTK_MEM_HOST or OVTK_MEM_DEVICE");
    if (int rc = use_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t rows_bytes = size_t(batch_size) * 4;
    if (n_rowids == 0) {   // every row is [0, 0): nothing to launch
        if (batch_size == 0) return OVTK_OK;
        if (mem == OVTK_MEM_HOST) {
            std::memset(out_begins, 0, rows_bytes);
            std::memset(out_ends, 0, rows_bytes);
        } else {
            OVTK_HIP(hipMemsetAsync(out_begins, 0, rows_bytes, s));
            OVTK_HIP(hipMemsetAsync(out_ends, 0, rows_bytes, s));
        }
        return OVTK_OK;
    }
    WorkspaceLease ws(device);
    RunStatus* st = nullptr;
    if (int rc = tf_begin_status(*ws.ws, s, &st)) return rc;
    const int32_t* ids = nullptr;
    if (int rc = in_source(ws->in_begins, rowids, size_t(n_rowids) * 4, mem, s, &ids)) return rc;
    int32_t *d_b = nullptr, *d_e = nullptr;
    if (int rc = out_target(ws->out_a, out_begins, std::max<size_t>(rows_bytes, 4), mem, &d_b)) return rc;
    if (int rc = out_target(ws->out_b, out_ends, std::max<size_t>(rows_bytes, 4), mem, &d_e)) return rc;
    GapList gl{nullptr, batch_size / kLongGap + 2, &st->n_items};   // (the status block is zeroed: the list starts empty)
    if (int rc = ws->gen[0].ensure(size_t(gl.cap) * 3 * sizeof(int32_t))) return rc;
    gl.entries = ws->gen[0].as<int32_t>();
    OVTK_LAUNCH(ws->marks, "rowids_to_ragged", rowids_to_ragged_kernel, grid_for_elems(n_rowids), kBlockThreads, s, ids, int(n_rowids),
                int(batch_size), d_b, d_e, gl, st);
    if (batch_size > kLongGap) {   // (a shorter batch has no stretch that long)
        const int grid = std::max(1, std::min((batch_size + kBlockThreads - 1) / kBlockThreads, device_cu_count(device) * 4));
        OVTK_LAUNCH(ws->marks, "rowids_gap_fill", gap_fill_kernel, grid, kBlockThreads, s, gl, d_b, d_e);
    }
    if (int rc = finish_status(*ws.ws, s)) return rc;
    const uint32_t f = ws->host_status->flags;
    if (f & kFlagRange) return set_error(OVTK_E_RANGE, "row id must be non-negative");   // ragged_to_ragged.cpp:61
    if (f & kFlagUnsorted) return set_error(OVTK_E_ARG, "ragged_to_ragged: row ids must not decrease");
    if (int rc = copy_back(out_begins, d_b, rows_bytes, mem, s)) return rc;
    if (int rc = copy_back(out_ends, d_e, rows_bytes, mem, s)) return rc;
    if (mem == OVTK_MEM_HOST) OVTK_HIP(hipStreamSynchronize(s));
    return OVTK_OK;
}

}  // extern "C"
