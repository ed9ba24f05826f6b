// api_unigram.cpp -- C-ABI entry points of UnigramTokenizer.  Compiled as HIP (hipcc -x hip).
// Reference behaviour replaced: src/unigram_tokenizer.cpp:17-77 (evaluate), :92-131 (the table), :147-224 (tokenize_into).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "ops_kernels.hpp"
#include "runtime.hpp"
#include "tables.hpp"
#include "unigram_kernels.hpp"

using namespace ovtk;

struct ovtk_unigram {
    int device = 0;
    UnigramDev dev{};
    DevBuf root, buckets, scores;
    int byte_fallback = 0, fuse_unk = 0;   // stored as the reference stores them; evaluate() reads neither
};

namespace {

int unigram_begin_status(Workspace& ws, hipStream_t s, RunStatus** st) {
    if (!ws.host_status) return set_error(OVTK_E_HIP, "pinned host allocation failed");
    if (int rc = ws.status.ensure(sizeof(RunStatus))) return rc;
    *st = ws.status.as<RunStatus>();
    OVTK_HIP(hipMemsetAsync(*st, 0, sizeof(RunStatus), s));
    return OVTK_OK;
}

}  // namespace

extern "C" {

int ovtk_unigram_create(const ovtk_strings* vocab, const float* scores, const ovtk_unigram_params* p, int device, ovtk_unigram** out) {
    if (!vocab || !p || !out) return set_error(OVTK_E_ARG, "unigram: null argument");
    if (vocab->n < 0 || vocab->n_chars < 0) return set_error(OVTK_E_ARG, "unigram vocab: negative size");
    if (vocab->n >= INT32_MAX || vocab->n_chars >= INT32_MAX) return set_error(OVTK_E_ARG, "unigram vocab: tensor sizes must fit int32 offsets");
    if (vocab->n > 0 && !scores) return set_error(OVTK_E_ARG, "unigram: null scores");
    if (vocab->n >= int64_t(kUniUnkCode)) return set_error(OVTK_E_UNSUPPORTED, "unigram: more than 4 194 302 vocabulary entries");
    if (int rc = use_device(device)) return rc;
    auto h = std::make_unique<ovtk_unigram>();
    h->device = device;
    h->byte_fallback = p->byte_fallback;
    h->fuse_unk = p->fuse_unk;
    TrieHost t;
    float min_score = FLT_MAX;   // src/unigram_tokenizer.cpp:118-122: over the scores given
    for (int64_t i = vocab->n - 1; i >= 0; --i) {   // (downwards: of equal strings the LOWEST id stays, this library's choice)
        const int64_t b = vocab->begins[i], e = vocab->ends[i];
        if (b < 0 || e < b || e > vocab->n_chars) return set_error(OVTK_E_RANGE, "unigram: vocab begins/ends outside the chars tensor");
        if (e - b > kUniMaxTokenBytes) return set_error(OVTK_E_UNSUPPORTED, "unigram: a vocabulary entry is longer than 1 023 bytes");
        min_score = std::min(min_score, scores[i]);
        if (e > b) t.add(vocab->chars + b, size_t(e - b), int32_t(i));   // (an empty string never matches, this library's choice)
    }
    TrieBucketsHost tb;
    if (!tb.build(t)) return set_error(OVTK_E_UNSUPPORTED, "unigram: the vocabulary's trie has more than 8 million nodes");
    if (int rc = h->root.upload(tb.root.data(), tb.root.size() * sizeof(I2))) return rc;
    if (int rc = h->buckets.upload(tb.buckets.data(), tb.buckets.size() * sizeof(TrieBucket))) return rc;
    const float none = 0.0f;
    if (int rc = h->scores.upload(vocab->n ? scores : &none, size_t(std::max<int64_t>(vocab->n, 1)) * sizeof(float))) return rc;
    h->dev.trie = TrieBucketsDev{h->root.as<I2>(), h->buckets.as<TrieBucket>(), tb.bucket_mask, tb.bucket_shift};
    h->dev.scores = h->scores.as<float>();
    h->dev.unk_score = float(double(min_score) - 10.0);   // :81, :157: one rounding to float32
    h->dev.unk_token_id = p->unk_token_id;
    OVTK_HIP(hipStreamSynchronize(nullptr));
    *out = h.release();
    return OVTK_OK;
}

void ovtk_unigram_destroy(ovtk_unigram* h) { delete h; }

int ovtk_unigram_run(ovtk_unigram* h, const ovtk_ragged_strings* in, ovtk_ragged_i32_out* out, int mem, void* stream) {
    if (!h || !in || !out) return set_error(OVTK_E_ARG, "null argument");
    if (int rc = check_rows(in)) return rc;
    if (out->data_capacity < 0) return set_error(OVTK_E_ARG, "unigram: bad size");
    if (mem != OVTK_MEM_HOST && mem != OVTK_MEM_DEVICE) return set_error(OVTK_E_ARG, "mem must be OVTK_MEM_HOST or OVTK_MEM_DEVICE");
    if (int rc = use_device(h->device)) return rc;
    out->n_rows = in->n_rows;
    out->n_data = 0;
    if (in->n_rows == 0) return OVTK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WorkspaceLease ws(h->device);
    RunStatus* st = nullptr;
    if (int rc = unigram_begin_status(*ws.ws, s, &st)) return rc;
    UniWork w{};
    if (int rc = in_source(ws->in_rb, in->ragged_begins, size_t(in->n_rows) * 4, mem, s, &w.ragged_begins)) return rc;
    if (int rc = in_source(ws->in_re, in->ragged_ends, size_t(in->n_rows) * 4, mem, s, &w.ragged_ends)) return rc;
    if (int rc = in_source(ws->in_begins, in->strings.begins, size_t(in->strings.n) * 4, mem, s, &w.begins)) return rc;
    if (int rc = in_source(ws->in_ends, in->strings.ends, size_t(in->strings.n) * 4, mem, s, &w.ends)) return rc;
    if (int rc = in_source(ws->in_chars, in->strings.chars, size_t(in->strings.n_chars), mem, s, &w.chars)) return rc;
    w.n_rows = in->n_rows;
    w.n_strings = in->strings.n;
    w.n_chars = in->strings.n_chars;
    w.dev = h->dev;
    w.status = st;
    int32_t *d_b = nullptr, *d_e = nullptr, *d_i = nullptr;
    if (int rc = out_target(ws->out_a, out->begins, size_t(in->n_rows) * 4, mem, &d_b)) return rc;
    if (int rc = out_target(ws->out_b, out->ends, size_t(in->n_rows) * 4, mem, &d_e)) return rc;
    if (int rc = out_target(ws->out_c, out->data, size_t(std::max<int64_t>(out->data_capacity, 1)) * 4, mem, &d_i)) return rc;
    const size_t n_str = size_t(std::max<int64_t>(in->strings.n, 1));
    if (int rc = ws->gen[0].ensure(n_str * 8)) return rc;
    if (int rc = ws->gen[1].ensure(n_str * 4)) return rc;
    if (int rc = ws->gen[2].ensure(n_str * 4)) return rc;
    if (int rc = ws->gen[3].ensure(size_t(in->n_rows) * 4)) return rc;
    w.node_off = ws->gen[0].as<long long>();
    w.str_cnt = ws->gen[1].as<int32_t>();
    w.str_over = ws->gen[2].as<int32_t>();
    w.row_len = ws->gen[3].as<int32_t>();
    if ((std::max<int64_t>(in->n_rows, in->strings.n) + kTileElems - 1) / kTileElems > INT32_MAX)
        return set_error(OVTK_E_UNSUPPORTED, "too many rows for one call; split it");
    if (int rc = ws->tiles.ensure(scan_tiles_bytes(std::max<int64_t>(in->n_rows, in->strings.n)))) return rc;
    const int wave_grid = int(std::min<long long>((in->n_rows + kTileThreads / kWave - 1) / (kTileThreads / kWave), (long long)device_cu_count(h->device) * 32));
    // a string's stretch is its bytes + 1 nodes; strings that overlap in the chars tensor need more than it has bytes: second attempt
    int64_t cap = in->strings.n_chars + in->strings.n + 1;
    uint32_t f = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (attempt) {
            if (int rc = unigram_begin_status(*ws.ws, s, &st)) return rc;
            w.status = st;
        }
        if (cap >= INT32_MAX - 1) return set_error(OVTK_E_UNSUPPORTED, "UnigramTokenizer: too much text for one call; split it");
        if (int rc = ws->gen[4].ensure(size_t(cap) * sizeof(int32_t))) return rc;
        if (int rc = ws->gen[5].ensure(size_t(cap) * sizeof(UniEdgeList))) return rc;
        if (int rc = ws->gen[6].ensure(size_t(cap) * sizeof(UniNode))) return rc;
        if (int rc = ws->stage.ensure(size_t(cap) * sizeof(int32_t))) return rc;
        w.owner = ws->gen[4].as<int32_t>();
        w.lists = ws->gen[5].as<UniEdgeList>();
        w.nodes = ws->gen[6].as<UniNode>();
        w.ids = ws->stage.as<int32_t>();
        w.cap = cap;
        launch_scan(ws->marks, "unigram_stretch", s, in->strings.n, UniStretch{w}, UniStretchApply{w}, UniStretchFin{st, (long long)cap},
                    ws->tiles.as<long long>(), st, 0u);
        const unsigned edge_grid = unsigned((cap + kTileThreads - 1) / kTileThreads);
        OVTK_LAUNCH(ws->marks, "unigram_edges", unigram_edges_kernel, edge_grid, kTileThreads, s, w);
        if (in->strings.n > 0)
            OVTK_LAUNCH(ws->marks, "unigram_relax", each_kernel<UniRelax>, unsigned((in->strings.n + kTileThreads - 1) / kTileThreads), kTileThreads, s,
                        (long long)in->strings.n, UniRelax{w}, (const RunStatus*)st, kFlagRange | kFlagStageOverflow);
        OVTK_LAUNCH(ws->marks, "unigram_rows", each_kernel<UniRowCount>, unsigned((in->n_rows + kTileThreads - 1) / kTileThreads), kTileThreads, s,
                    (long long)in->n_rows, UniRowCount{w}, (const RunStatus*)st, kFlagRange | kFlagStageOverflow);
        launch_scan(ws->marks, "unigram_offsets", s, in->n_rows, FiledLen{w.row_len}, RowOffsets{d_b, d_e, 0},
                    CharsFin{st, (long long)std::min<int64_t>(out->data_capacity, INT32_MAX - 1)}, ws->tiles.as<long long>(), st,
                    kFlagRange | kFlagStageOverflow);
        OVTK_LAUNCH(ws->marks, "unigram_gather", each_wave_kernel<UniGather>, wave_grid, kTileThreads, s, (long long)in->n_rows, UniGather{w, d_b, d_i},
                    (const RunStatus*)st, kFlagOutCapacity | kFlagRange | kFlagStageOverflow);
        if (int rc = finish_status(*ws.ws, s)) return rc;
        f = ws->host_status->flags;
        if (!(f & kFlagStageOverflow)) break;
        if (ws->host_status->stage_need >= INT32_MAX - 1)
            return set_error(OVTK_E_UNSUPPORTED, "UnigramTokenizer: the strings add up to 2^31 bytes or more; split the call");
        if (attempt) return set_error(OVTK_E_HIP, "UnigramTokenizer: workspace sizing did not converge");
        cap = ws->host_status->stage_need;
    }
    if (f & kFlagRange) return set_error(OVTK_E_RANGE, "input begins/ends index outside their tensors");
    if (f & kFlagOutCapacity) return set_error(OVTK_E_CAPACITY, "UnigramTokenizer: output ids buffer too small");
    out->n_data = ws->host_status->n_out;
    int err = 0;
    err = err ? err : copy_back(out->begins, d_b, size_t(in->n_rows) * 4, mem, s);
    err = err ? err : copy_back(out->ends, d_e, size_t(in->n_rows) * 4, mem, s);
    err = err ? err : copy_back(out->data, d_i, size_t(out->n_data) * 4, mem, s);
    if (err) return err;
    if (mem == OVTK_MEM_HOST) OVTK_HIP(hipStreamSynchronize(s));
    return OVTK_OK;
}

}  // extern "C"
