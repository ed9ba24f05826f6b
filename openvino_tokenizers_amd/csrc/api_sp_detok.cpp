// api_sp_detok.cpp -- C-ABI entry points of SentencepieceDetokenizer and SentencepieceStreamDetokenizer.  Compiled as HIP (hipcc -x hip).
// Reference behaviour replaced: src/sentence_piece.cpp:395-433 (ids below GetPieceSize() through SentencePieceProcessor::Decode),
// :478-523 (the pieces as they are, <0xHH> as one byte).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "runtime.hpp"
#include "sp_detok_kernels.hpp"
#include "sp_model.hpp"

using namespace ovtk;

namespace {

// One op's device tables (sp_detok_kernels.hpp).
struct SdTable {
    DevBuf pieces, begins, chars;
    int64_t longest = 0;   // bytes of the longest text a token can give
    bool any_byte = false, any_strip = false;
    int build(const std::vector<std::string>& text, const std::vector<uint32_t>& flags) {
        std::vector<uint4> pc(text.size());
        std::vector<int32_t> tb(text.size());
        std::string blob;
        for (size_t i = 0; i < text.size(); ++i) {
            const std::string& t = text[i];
            uint32_t w[3] = {0, 0, 0};
            std::memcpy(w, t.data(), std::min<size_t>(t.size(), size_t(kSdInline)));
            pc[i] = uint4{w[0], w[1], w[2], uint32_t(t.size()) | kSdInVocab | flags[i]};
            tb[i] = int32_t(blob.size());
            if (t.size() > size_t(kSdInline)) blob += t;
            longest = std::max<int64_t>(longest, (flags[i] & kSdByte) ? 3 : int64_t(t.size()));
            any_byte |= (flags[i] & kSdByte) != 0;
            any_strip |= (flags[i] & kSdStrip) != 0;
        }
        blob.append(16, '\0');
        if (int rc = pieces.upload(pc.data(), pc.size() * sizeof(uint4))) return rc;
        if (int rc = begins.upload(tb.data(), tb.size() * sizeof(int32_t))) return rc;
        return chars.upload(blob.data(), blob.size());
    }
};

}  // namespace

struct ovtk_sp_detokenizer {
    int device = 0;
    int32_t vocab_size = 0;
    SdTable decode, stream;
    std::string stream_refusal;   // non-empty: why the stream op does not run with this model
};

namespace {

int sd_begin_status(Workspace& ws, hipStream_t s, RunStatus** st) {
    if (!ws.host_status) return set_error(OVTK_E_HIP, "pinned host allocation failed");
    if (int rc = ws.status.ensure(sizeof(RunStatus))) return rc;
    *st = ws.status.as<RunStatus>();
    OVTK_HIP(hipMemsetAsync(*st, 0, sizeof(RunStatus), s));
    return OVTK_OK;
}

int sd_check_args(ovtk_sp_detokenizer* h, const int32_t* ids, int64_t batch, int64_t seq_len, int stream_mode, ovtk_strings_out* out) {
    if (!h || !out) return set_error(OVTK_E_ARG, "sp_detokenizer: null argument");
    if (batch < 0 || seq_len < 0 || out->chars_capacity < 0) return set_error(OVTK_E_ARG, "sp_detokenizer: negative size");
    if (batch * std::max<int64_t>(seq_len, 1) >= INT32_MAX) return set_error(OVTK_E_ARG, "sp_detokenizer: batch * seq_len must fit int32; split the call");
    if (batch * seq_len > 0 && !ids) return set_error(OVTK_E_ARG, "sp_detokenizer: null ids");
    if (stream_mode && !h->stream_refusal.empty()) return set_error(OVTK_E_UNSUPPORTED, h->stream_refusal);
    return OVTK_OK;
}

// first-token pass (Decode with stripping only) -> count -> scan -> write, all on `s`; ids, outputs and st are device memory.
int sd_passes(ovtk_sp_detokenizer* h, Workspace& ws, hipStream_t s, const int32_t* d_ids, int64_t batch, int64_t seq, int stream_mode, int32_t* d_b,
              int32_t* d_e, uint8_t* d_c, long long cap, RunStatus* st) {
    const SdTable& t = stream_mode ? h->stream : h->decode;
    const int n_seg = int((seq + kSegTokens - 1) / kSegTokens);
    const long long n_units = batch * n_seg;
    if (int rc = ws.gen[2].ensure(size_t(n_units) * sizeof(long long))) return rc;
    if (int rc = ws.gen[3].ensure(size_t(n_units) * sizeof(long long))) return rc;
    if (int rc = ws.gen[4].ensure(size_t(n_units) * sizeof(unsigned long long))) return rc;
    if (int rc = ws.gen[5].ensure(size_t(batch) * sizeof(int32_t))) return rc;
    if (int rc = ws.tiles.ensure(scan_tiles_bytes(n_units))) return rc;
    long long* unit_bytes = ws.gen[2].as<long long>();
    long long* unit_off = ws.gen[3].as<long long>();
    unsigned long long* unit_ctx = ws.gen[4].as<unsigned long long>();
    SpDetokDev d{d_ids, t.pieces.as<uint4>(), t.begins.as<int32_t>(), t.chars.as<uint8_t>(), h->vocab_size, t.any_byte ? 1 : 0, nullptr};
    const long long cus = device_cu_count(h->device);
    if (t.any_strip) {
        int32_t* row_first = ws.gen[5].as<int32_t>();
        OVTK_LAUNCH(ws.marks, "sp_detok_first", sp_detok_first_kernel, int(std::min<long long>((batch + kWavesPerBlock - 1) / kWavesPerBlock, cus * 8)),
                    kBlockThreads, s, d, int(seq), (long long)batch, row_first);
        d.row_first = row_first;
    }
    const int grid = int(std::min<long long>((n_units + kWavesPerBlock - 1) / kWavesPerBlock, cus * 8));
    OVTK_LAUNCH(ws.marks, "sp_detok_count", sp_detok_kernel<false>, grid, kBlockThreads, s, d, int(seq), n_seg, n_units, unit_bytes, unit_ctx,
                (const long long*)nullptr, (uint8_t*)nullptr, st);
    launch_scan(ws.marks, "sp_detok_scan", s, n_units, UnitLen{unit_bytes}, UnitApply{unit_off, n_seg, d_b, d_e}, CharsFin{st, cap},
                ws.tiles.as<long long>(), st, kFlagOutCapacity | kFlagRange);
    OVTK_LAUNCH(ws.marks, "sp_detok_write", sp_detok_kernel<true>, grid, kBlockThreads, s, d, int(seq), n_seg, n_units, unit_bytes, unit_ctx,
                (const long long*)unit_off, d_c, st);
    return OVTK_OK;
}

// What the status block of a finished call says: out->n_chars, the call's code.
int sd_report(const RunStatus& st, ovtk_strings_out* out) {
    out->n_chars = 0;
    if (st.flags & kFlagRange) return set_error(OVTK_E_RANGE, "sp_detokenizer: a negative id (SentencePieceProcessor::Decode fails with OUT_OF_RANGE)");
    out->n_chars = st.n_out;   // (on E_CAPACITY: what the call needs, INT32_MAX = more than int32 offsets reach)
    if (st.flags & kFlagOutCapacity)
        return set_error(OVTK_E_CAPACITY, "sp_detokenizer: output chars buffer too small or beyond int32 offsets (" + std::to_string(st.n_out) + " bytes needed)");
    return OVTK_OK;
}

struct SdRun final : ovtk::PendingStrings {
    explicit SdRun(int device) : ws(device) {}
    WorkspaceLease ws;
    int finish(ovtk_strings_out* out) override {
        OVTK_HIP(hipEventSynchronize(ws->done));
        ws->marks.settled();
        Profiler::get().resolve(ws->marks);
        OVTK_HIP(hipGetLastError());
        return sd_report(*ws->host_status, out);
    }
};

}  // namespace

extern "C" {

int ovtk_sp_detokenizer_create(const uint8_t* model, int64_t model_len, int device, ovtk_sp_detokenizer** out) {
    if (!out || model_len < 0 || (model_len > 0 && !model)) return set_error(OVTK_E_ARG, "sp_detokenizer: bad argument");
    SpModel m;
    std::string why;
    if (!sp_model_parse(model, size_t(model_len), m, &why)) return set_error(OVTK_E_ARG, "sp_detokenizer: the model is truncated or malformed (in " + why + ")");
    if (m.pieces.empty()) return set_error(OVTK_E_ARG, "sp_detokenizer: the model has no pieces");
    // what this library does not run (never an approximation)
    if (m.treat_whitespace_as_suffix)
        return set_error(OVTK_E_UNSUPPORTED, "SentencepieceDetokenizer: treat_whitespace_as_suffix (Decode then strips at the other end)");
    if (!m.denormalizer_charsmap.empty()) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceDetokenizer: a denormalizer_spec with a precompiled_charsmap");
    if (int64_t(m.pieces.size()) >= 4194303) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceDetokenizer: more than 4 194 302 pieces");
    const std::string unk_surface = m.has_unk_surface ? m.unk_surface : std::string(" \xE2\x81\x87 ");
    if (unk_surface.size() > 1023) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceDetokenizer: an unk_surface longer than 1 023 bytes");
    if (unk_surface.empty())   // (whether an unknown piece without text ends the start-of-sentence state was never put to sentencepiece)
        return set_error(OVTK_E_UNSUPPORTED, "SentencepieceDetokenizer: an unk_surface that is present and empty");
    const bool strip = m.add_dummy_prefix || m.remove_extra_whitespaces;
    static const std::string kSpace = "\xE2\x96\x81";
    const size_t n = m.pieces.size();
    std::vector<std::string> text(n), raw(n);
    std::vector<uint32_t> flags(n, 0u), none(n, 0u);
    std::string stream_refusal;
    for (size_t i = 0; i < n; ++i) {
        const SpPiece& pc = m.pieces[i];
        if (pc.piece.size() > 1023) return set_error(OVTK_E_UNSUPPORTED, "SentencepieceDetokenizer: a piece is longer than 1 023 bytes");
        // ---- the stream op (:507-514): the piece as it is; six bytes of the shape <0x..> are PieceToByte's one byte
        raw[i] = pc.piece;
        const std::string& p = pc.piece;
        auto hex = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; };
        const bool byte_shape = p.size() == 6 && p[0] == '<' && p[1] == '0' && p[2] == 'x' && p[5] == '>';
        const int byte_value = byte_shape && hex(p[3]) >= 0 && hex(p[4]) >= 0 ? hex(p[3]) * 16 + hex(p[4]) : -1;
        if (byte_shape) {
            if (byte_value < 0 && stream_refusal.empty())
                stream_refusal = "SentencepieceStreamDetokenizer: piece " + std::to_string(i) + " has the shape <0x..> without two upper-case hex digits";
            raw[i] = std::string(1, char(byte_value < 0 ? 0xFF : byte_value));
        }
        // ---- Decode
        switch (pc.type) {
        case kSpControl: break;   // nothing, and the start-of-sentence state goes on
        case kSpUnknown:
            text[i] = unk_surface;
            flags[i] = kSdEndsStart;
            break;
        case kSpByte:
            if (byte_value < 0) return set_error(OVTK_E_ARG, "sp_detokenizer: a BYTE piece that is not <0xHH>");
            text[i] = std::string(1, char(byte_value));
            flags[i] = kSdByte | kSdEndsStart | uint32_t(byte_value) << kSdByteShift;
            break;
        default: {   // NORMAL, USER_DEFINED, UNUSED: every space symbol is one space
            std::string& t = text[i];
            for (size_t k = 0; k < p.size();) {
                if (p.compare(k, 3, kSpace) == 0) {
                    t += ' ';
                    k += 3;
                } else {
                    t += p[k++];
                }
            }
            const bool leading = p.compare(0, 3, kSpace) == 0;
            if (strip && leading) flags[i] |= kSdStrip;
            // with remove_extra_whitespaces the state lasts until something non-empty came out: a lone space symbol does not end it
            if (!(m.remove_extra_whitespaces && p == kSpace)) flags[i] |= kSdEndsStart;
        }
        }
    }
    if (int rc = use_device(device)) return rc;
    auto h = std::make_unique<ovtk_sp_detokenizer>();
    h->device = device;
    h->vocab_size = int32_t(n);
    h->stream_refusal = stream_refusal;
    if (int rc = h->decode.build(text, flags)) return rc;
    if (int rc = h->stream.build(raw, none)) return rc;
    h->decode.longest = std::max<int64_t>(h->decode.longest, 3);
    OVTK_HIP(hipStreamSynchronize(nullptr));
    *out = h.release();
    return OVTK_OK;
}

void ovtk_sp_detokenizer_destroy(ovtk_sp_detokenizer* h) { delete h; }

int64_t ovtk_sp_detokenizer_bound(ovtk_sp_detokenizer* h, int64_t batch, int64_t seq_len) {
    if (!h || batch < 0 || seq_len < 0) return -1;
    return batch * seq_len * std::max(h->decode.longest, h->stream.longest);
}

int ovtk_sp_detokenizer_run(ovtk_sp_detokenizer* h, const int32_t* ids, int64_t batch, int64_t seq_len, int stream_mode, ovtk_strings_out* out,
                            int mem, void* stream) {
    if (int rc = sd_check_args(h, ids, batch, seq_len, stream_mode, out)) return rc;
    if (mem != OVTK_MEM_HOST && mem != OVTK_MEM_DEVICE) return set_error(OVTK_E_ARG, "mem must be OVTK_MEM_HOST or OVTK_MEM_DEVICE");
    if (int rc = use_device(h->device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    out->n_chars = 0;
    if (batch == 0) return OVTK_OK;
    WorkspaceLease ws(h->device);
    RunStatus* st = nullptr;
    if (int rc = sd_begin_status(*ws.ws, s, &st)) return rc;
    int32_t *d_b = nullptr, *d_e = nullptr;
    uint8_t* d_c = nullptr;
    if (int rc = out_target(ws->out_c, out->begins, size_t(batch) * 4, mem, &d_b)) return rc;
    if (int rc = out_target(ws->out_d, out->ends, size_t(batch) * 4, mem, &d_e)) return rc;
    if (int rc = out_target(ws->out_e, out->chars, size_t(std::max<int64_t>(out->chars_capacity, 1)), mem, &d_c)) return rc;
    if (seq_len == 0) {
        OVTK_HIP(hipMemsetAsync(d_b, 0, size_t(batch) * 4, s));
        OVTK_HIP(hipMemsetAsync(d_e, 0, size_t(batch) * 4, s));
    } else {
        const int32_t* d_ids = nullptr;
        if (int rc = in_source(ws->gen[0], ids, size_t(batch * seq_len) * 4, mem, s, &d_ids)) return rc;
        if (int rc = sd_passes(h, *ws.ws, s, d_ids, batch, seq_len, stream_mode, d_b, d_e, d_c,
                               (long long)std::min<int64_t>(out->chars_capacity, INT32_MAX - 1), st))
            return rc;
    }
    if (int rc = finish_status(*ws.ws, s)) return rc;
    if (int rc = sd_report(*ws->host_status, out)) return rc;
    int e = 0;
    e = e ? e : copy_back(out->begins, d_b, size_t(batch) * 4, mem, s);
    e = e ? e : copy_back(out->ends, d_e, size_t(batch) * 4, mem, s);
    e = e ? e : copy_back(out->chars, d_c, size_t(out->n_chars), mem, s);
    if (e) return e;
    if (mem == OVTK_MEM_HOST) OVTK_HIP(hipStreamSynchronize(s));
    return OVTK_OK;
}

int ovtk_sp_detokenizer_enqueue(ovtk_sp_detokenizer* h, const int32_t* ids, int64_t batch, int64_t seq_len, int stream_mode, ovtk_strings_out* out,
                                void* stream, ovtk_pending** pending) {
    if (!pending) return set_error(OVTK_E_ARG, "null argument");
    *pending = nullptr;
    if (int rc = sd_check_args(h, ids, batch, seq_len, stream_mode, out)) return rc;
    if (int rc = use_device(h->device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto p = std::make_unique<ovtk_pending>();
    p->strings_out = *out;
    p->strings_out.n_chars = 0;
    if (batch > 0) {
        auto run = std::make_unique<SdRun>(h->device);
        Workspace& ws = *run->ws.ws;
        if (!ws.done) OVTK_HIP(hipEventCreateWithFlags(&ws.done, hipEventDisableTiming));
        RunStatus* st = nullptr;
        if (int rc = sd_begin_status(ws, s, &st)) return rc;
        if (seq_len == 0) {
            OVTK_HIP(hipMemsetAsync(out->begins, 0, size_t(batch) * 4, s));
            OVTK_HIP(hipMemsetAsync(out->ends, 0, size_t(batch) * 4, s));
        } else {
            if (int rc = sd_passes(h, ws, s, ids, batch, seq_len, stream_mode, out->begins, out->ends, out->chars,
                                   (long long)std::min<int64_t>(out->chars_capacity, INT32_MAX - 1), st))
                return rc;
        }
        OVTK_HIP(hipMemcpyAsync(ws.host_status, ws.status.as<RunStatus>(), sizeof(RunStatus), hipMemcpyDeviceToHost, s));
        OVTK_HIP(hipEventRecord(ws.done, s));
        p->strings = std::move(run);
    }
    *pending = p.release();
    return OVTK_OK;
}

int ovtk_sp_detokenizer_finish(ovtk_pending* pending, ovtk_strings_out* out) {
    if (!pending) return set_error(OVTK_E_ARG, "null argument");
    std::unique_ptr<ovtk_pending> p(pending);   // released whatever happens
    const int rc = p->strings ? p->strings->finish(&p->strings_out) : OVTK_OK;
    if (out) *out = p->strings_out;
    return rc;
}

}  // extern "C"
