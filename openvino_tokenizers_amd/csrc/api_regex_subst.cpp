// api_regex_subst.cpp -- C-ABI entry points of RegexNormalization.  Compiled as HIP (hipcc -x hip).
// Reference behaviour replaced: src/regex_normalization.cpp:127-153 (evaluate), src/utils.cpp:315-382 (PCRE2Wrapper::substitute),
// src/utils.cpp:178-234 (evaluate_normalization_helper).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "ops_kernels.hpp"
#include "regex_subst.hpp"
#include "regex_subst_kernels.hpp"
#include "runtime.hpp"

using namespace ovtk;

struct ovtk_regex_normalization {
    int device = 0;
    SubstDev dev{};
    struct Tables { DevBuf trans, ascii, index, blocks, ctx; };
    std::vector<std::unique_ptr<Tables>> tables;
    DevBuf alts, segs, lits, match_class, class_lits;
    int64_t grow_char = 1, grow_row = 0, quirk_row = 0;   // the output bound, see ovtk_regex_normalization_bound
};

extern "C" {

int ovtk_regex_normalization_create(const ovtk_regex_normalization_params* p, ovtk_regex_normalization** out) {
    if (!p || !out || p->pattern_len < 0 || p->replace_len < 0 || (p->pattern_len > 0 && !p->pattern) || (p->replace_len > 0 && !p->replace))
        return set_error(OVTK_E_ARG, "regex_normalization: bad argument");
    SubstPlan plan;
    std::string err;
    if (int rc = build_subst_plan(std::string(p->pattern ? p->pattern : "", size_t(p->pattern_len)),
                                  std::string(p->replace ? p->replace : "", size_t(p->replace_len)), p->global_replace != 0, plan, err))
        return set_error(rc, err);
    if (int rc = use_device(p->device)) return rc;
    auto h = std::make_unique<ovtk_regex_normalization>();
    h->device = p->device;
    SubstDev& d = h->dev;
    d.identity = plan.identity ? 1 : 0;
    d.global = plan.global ? 1 : 0;
    d.all_anchored = plan.all_anchored ? 1 : 0;
    d.tmpl_len = plan.tmpl_len;
    if (!plan.identity) {
        // (measurements and tests: the general walk for a pattern the class path would take)
        const char* force = std::getenv("OVTK_REGEX_NORM_GENERAL");
        if (force && force[0] == '1') plan.class_path = false;
        std::vector<SubstAltDev> alts(plan.alts.size());
        std::vector<SubstSegDev> segs;
        d.n_segs = int32_t(plan.alts[0].segs.size());
        for (size_t a = 0; a < plan.alts.size(); ++a) {
            const RegexProgram& prog = plan.alts[a].prog;
            h->tables.push_back(std::make_unique<ovtk_regex_normalization::Tables>());
            auto& t = *h->tables.back();
            int e = 0;
            e = e ? e : t.trans.upload(prog.trans.data(), prog.trans.size() * sizeof(uint16_t));
            e = e ? e : t.ascii.upload(prog.ascii_class, sizeof prog.ascii_class);
            e = e ? e : t.index.upload(prog.cp_index.data(), prog.cp_index.size() * sizeof(uint16_t));
            e = e ? e : t.blocks.upload(prog.cp_blocks.data(), prog.cp_blocks.size());
            e = e ? e : t.ctx.upload(prog.ctx_next.data(), std::max<size_t>(prog.ctx_next.size(), 1));
            if (e) return e;
            SubstAltDev& A = alts[a];
            std::memset(&A, 0, sizeof A);
            RegexDev& r = A.R;
            r.trans = t.trans.as<uint16_t>();
            r.ascii_class = t.ascii.as<uint8_t>();
            r.cp_index = t.index.as<uint16_t>();
            r.cp_blocks = t.blocks.as<uint8_t>();
            r.ctx_next = t.ctx.as<uint8_t>();
            r.n_syms = prog.n_syms;
            r.n_states = prog.n_states;
            r.sym_eot = prog.sym_eot;
            r.sym_final_nl = prog.sym_final_nl;
            r.n_ctx = prog.n_ctx;
            r.behind_chars = prog.behind_chars;
            r.cp_blocks_bytes = int32_t(prog.cp_blocks.size());
            std::memcpy(r.start, prog.start, sizeof r.start);
            std::memcpy(A.start_nonempty, prog.start_nonempty, sizeof A.start_nonempty);
            A.rc_min = plan.alts[a].rc_min;
            A.rc_max = plan.alts[a].rc_max;
            A.has_unset = plan.alts[a].has_unset ? 1 : 0;
            A.seg_first = int32_t(segs.size());
            for (const SubstSeg& s : plan.alts[a].segs) segs.push_back(SubstSegDev{s.kind, s.a, s.b});
        }
        const std::string class_lits = plan.class_pre + plan.class_suf;
        const SubstSegDev none{0, 0, 0};
        const uint8_t zero = 0;
        int e = 0;
        e = e ? e : h->alts.upload(alts.data(), alts.size() * sizeof(SubstAltDev));
        e = e ? e : h->segs.upload(segs.empty() ? &none : segs.data(), std::max<size_t>(segs.size(), 1) * sizeof(SubstSegDev));
        e = e ? e : h->lits.upload(plan.lits.empty() ? reinterpret_cast<const char*>(&zero) : plan.lits.data(), std::max<size_t>(plan.lits.size(), 1));
        e = e ? e : h->match_class.upload(plan.match_class, sizeof plan.match_class);
        e = e ? e : h->class_lits.upload(class_lits.empty() ? reinterpret_cast<const char*>(&zero) : class_lits.data(), std::max<size_t>(class_lits.size(), 1));
        if (e) return e;
        OVTK_HIP(hipStreamSynchronize(nullptr));
        d.alts = h->alts.as<SubstAltDev>();
        d.n_alts = int32_t(alts.size());
        d.segs = h->segs.as<SubstSegDev>();
        d.lits = h->lits.as<uint8_t>();
        d.match_class = h->match_class.as<uint8_t>();
        d.class_lits = h->class_lits.as<uint8_t>();
        d.class_path = plan.class_path ? 1 : 0;
        d.class_has_ref = plan.class_has_ref ? 1 : 0;
        d.pre_len = int32_t(plan.class_pre.size());
        d.suf_len = int32_t(plan.class_suf.size());
        // every match emits the template's literal bytes and, per reference, at most the match; a string has at most one match per
        // character and one more: n_chars * (1 + refs + literals) + n * literals.  The reference's buffer cuts it off at
        // 4 * (len + rc * template_len) per string, beyond which the string comes back as it was.
        int rc_max = 1;
        for (const auto& a : plan.alts) rc_max = std::max(rc_max, a.rc_max);
        h->grow_char = 1 + plan.n_refs + plan.lit_total;
        h->grow_row = plan.lit_total;
        h->quirk_row = 4ll * rc_max * plan.tmpl_len;
    }
    *out = h.release();
    return OVTK_OK;
}

void ovtk_regex_normalization_destroy(ovtk_regex_normalization* h) { delete h; }

int64_t ovtk_regex_normalization_bound(ovtk_regex_normalization* h, int64_t n, int64_t n_chars) {
    if (!h || n < 0 || n_chars < 0) return -1;
    if (h->dev.identity) return n_chars;
    return std::min(n_chars * h->grow_char + n * h->grow_row, 4 * n_chars + n * h->quirk_row);
}

int ovtk_regex_normalization_run(ovtk_regex_normalization* h, const ovtk_strings* in, const uint8_t* skips, ovtk_strings_out* out, int mem,
                                 void* stream) {
    if (!h) return set_error(OVTK_E_ARG, "regex_normalization: null handle");
    if (!in || !out) return set_error(OVTK_E_ARG, "regex_normalization: null argument");
    if (in->n < 0 || in->n_chars < 0 || out->chars_capacity < 0) return set_error(OVTK_E_ARG, "regex_normalization: negative size");
    if (in->n >= INT32_MAX || in->n_chars >= INT32_MAX) return set_error(OVTK_E_ARG, "regex_normalization: tensor sizes must fit int32 offsets");
    if (mem != OVTK_MEM_HOST && mem != OVTK_MEM_DEVICE) return set_error(OVTK_E_ARG, "mem must be OVTK_MEM_HOST or OVTK_MEM_DEVICE");
    if (int rc = use_device(h->device)) return rc;
    out->n_chars = 0;
    if (in->n == 0) return OVTK_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WorkspaceLease ws(h->device);
    if (!ws->host_status) return set_error(OVTK_E_HIP, "pinned host allocation failed");
    if (int rc = ws->status.ensure(sizeof(RunStatus))) return rc;
    RunStatus* st = ws->status.as<RunStatus>();
    OVTK_HIP(hipMemsetAsync(st, 0, sizeof(RunStatus), s));
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
    if (int rc = ws->gen[7].ensure(size_t(in->n))) return rc;
    int32_t* lens = ws->gen[6].as<int32_t>();
    uint8_t* ident = ws->gen[7].as<uint8_t>();
    if ((in->n + kTileElems - 1) / kTileElems > INT32_MAX) return set_error(OVTK_E_UNSUPPORTED, "too many strings for one call; split it");
    if (int rc = ws->tiles.ensure(scan_tiles_bytes(in->n))) return rc;
    OVTK_LAUNCH(ws->marks, "check_strings", check_strings_kernel, grid_for_elems(in->n), kBlockThreads, s, b, e, (long long)in->n,
                (long long)in->n_chars, st);
    // count (class path: a wave per string; general path: a lane per string) -> scan of the filed lengths -> a wave per string writes
    const int wave_grid = int(std::min<long long>((in->n + kTileThreads / kWave - 1) / (kTileThreads / kWave), (long long)device_cu_count(h->device) * 16));
    const char* count_tag = h->dev.class_path ? "regex_norm_class_count" : "regex_norm_count";
    const char* write_tag = h->dev.class_path ? "regex_norm_class_write" : "regex_norm_write";
    if (h->dev.class_path || h->dev.identity)
        OVTK_LAUNCH(ws->marks, count_tag, each_wave_kernel<SubstRow<false>>, wave_grid, kTileThreads, s, (long long)in->n,
                    (SubstRow<false>{h->dev, b, e, c, (long long)in->n_chars, sk, lens, ident, nullptr, nullptr, st}), (const RunStatus*)st, kFlagRange);
    else   // counting copies nothing: a lane per row, every lane its own matcher
        OVTK_LAUNCH(ws->marks, count_tag, (each_kernel<SubstRow<false, true>>), int((in->n + kTileThreads - 1) / kTileThreads), kTileThreads, s, (long long)in->n,
                    (SubstRow<false, true>{h->dev, b, e, c, (long long)in->n_chars, sk, lens, ident, nullptr, nullptr, st}), (const RunStatus*)st, kFlagRange);
    launch_scan(ws->marks, "regex_norm_offsets", s, in->n, FiledLen{lens}, RowOffsets{d_b, d_e, 0},
                CharsFin{st, (long long)std::min<int64_t>(out->chars_capacity, INT32_MAX - 1)}, ws->tiles.as<long long>(), st, kFlagRange);
    OVTK_LAUNCH(ws->marks, write_tag, each_wave_kernel<SubstRow<true>>, wave_grid, kTileThreads, s, (long long)in->n,
                (SubstRow<true>{h->dev, b, e, c, (long long)in->n_chars, sk, lens, ident, d_b, d_c, st}), (const RunStatus*)st,
                kFlagOutCapacity | kFlagRange | kFlagSubstUndecided);
    if (int rc = finish_status(*ws.ws, s)) return rc;
    if (ws->host_status->flags & kFlagRange) return set_error(OVTK_E_RANGE, "input begins/ends index outside the chars tensor");
    if (ws->host_status->flags & kFlagSubstUndecided)
        return set_error(OVTK_E_UNSUPPORTED, "RegexNormalization: a string's result lies between the sizes of the reference's buffer for the fewest and the most "
                                             "groups its first match can set (4 * (len + rc * template_len)); which of them PCRE2 reports is not tracked on the device");
    if (ws->host_status->flags & kFlagOutCapacity) {
        out->n_chars = ws->host_status->n_out;
        if (ws->host_status->n_out >= INT32_MAX - 1) return set_error(OVTK_E_UNSUPPORTED, "RegexNormalization: the output reaches 2^31 bytes; split the call");
        return set_error(OVTK_E_CAPACITY, "RegexNormalization: output chars buffer too small (" + std::to_string(ws->host_status->n_out) +
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

}  // extern "C"
