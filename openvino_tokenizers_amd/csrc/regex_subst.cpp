// regex_subst.cpp -- see regex_subst.hpp.
#include "regex_subst.hpp"

#include <algorithm>

#include "../../include/ovtk_amd.h"

namespace ovtk {

std::string subst_fix_search_pattern(const std::string& pattern) {
    // the three patterns old converters wrote, and what the reference runs in their place (src/regex_normalization.cpp:32-36)
    static const char* const rewrites[][2] = {
        {R"( ([\\.\\?\\!,])| ('[ms])| (') | ('[rv]e)| (n't))", R"((?| ([\\.\\?\\!,])| ('[ms])| (') | ('[rv]e)| (n't)))"},
        {R"((^)(.))", R"((^)([\s\S]))"},
        {R"((^)(.+))", R"((^)([\s\S]))"},
    };
    for (const auto& r : rewrites)
        if (pattern == r[0]) return r[1];
    return pattern;
}

std::string subst_reformat_replace_pattern(std::string replace) {
    for (char i = '1'; i <= '9'; ++i) {
        const std::string from = std::string("\\") + i, to = std::string("$") + i;
        size_t pos = 0;
        while ((pos = replace.find(from, pos)) != std::string::npos) {
            replace.replace(pos, from.size(), to);
            pos += to.size();
        }
    }
    return replace;
}

namespace {

struct TemplatePart {
    bool is_group;
    std::string lit;
    int group;
};

// PCRE2's substitute syntax without PCRE2_SUBSTITUTE_EXTENDED (pcre2_substitute.c): literal bytes, `$$`, `$n`, `${n}`, `$name`,
// `${name}`.  0: parsed; 1: PCRE2 reports an error (the op is the identity); 2: syntax this library does not take.
int parse_template(const std::string& t, const RegexWithGroups& rx, std::vector<TemplatePart>& parts, std::string& why) {
    auto lit = [&](char c) {
        if (parts.empty() || parts.back().is_group) parts.push_back(TemplatePart{false, "", 0});
        parts.back().lit.push_back(c);
    };
    auto word = [](unsigned char c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_'; };
    for (size_t i = 0; i < t.size();) {
        if (t[i] != '$') {
            lit(t[i++]);
            continue;
        }
        if (++i >= t.size()) { why = "the template ends in `$`"; return 1; }
        if (t[i] == '$') {
            lit('$');
            ++i;
            continue;
        }
        bool braces = false;
        if (t[i] == '{') {
            braces = true;
            if (++i >= t.size()) { why = "the template ends in `${`"; return 1; }
        }
        if (t[i] == '*') { why = "`$*MARK` in the template"; return 2; }
        int group = -1;
        if (t[i] >= '0' && t[i] <= '9') {
            long long g = 0;
            for (; i < t.size() && t[i] >= '0' && t[i] <= '9'; ++i) {
                g = g * 10 + (t[i] - '0');
                if (g > rx.n_groups) { why = "the template refers to group " + std::to_string(g) + ", the pattern has " + std::to_string(rx.n_groups); return 1; }
            }
            group = int(g);
        } else {
            std::string name;
            for (; i < t.size() && word(static_cast<unsigned char>(t[i])); ++i) {
                name.push_back(t[i]);
                if (name.size() > 32) { why = "a group name in the template is longer than 32 characters"; return 1; }
            }
            if (name.empty()) { why = "`$` in the template is followed by neither a group nor `$`"; return 1; }
            for (const auto& n : rx.names)
                if (n.first == name) group = n.second;
            if (group < 0) { why = "the template refers to a group named `" + name + "`, the pattern has none"; return 1; }
        }
        if (braces) {
            if (i >= t.size() || t[i] != '}') { why = "`${` in the template without its `}`"; return 1; }
            ++i;
        }
        parts.push_back(TemplatePart{true, "", group});
    }
    return 0;
}

// Every match of `p` is exactly one character, decided by its class alone: from the start state a class leads either nowhere or to a
// state that reports the match at whatever comes next and then dies.  No context, no `$`, no empty match.
bool one_character_program(const RegexProgram& p, uint8_t* match_class) {
    if (p.invalid || p.n_ctx != 1 || p.sym_final_nl >= 0 || p.can_match_empty || p.n_classes > 256) return false;
    const size_t ns = size_t(p.n_syms);
    const uint16_t* start = &p.trans[size_t(p.start[0]) * ns];
    if (start[p.sym_eot] != 0) return false;
    bool any = false;
    for (int c = 0; c < p.n_classes; ++c) {
        match_class[c] = 0;
        if (start[c] & ~kRegexStateMask) return false;
        const int next = start[c] & kRegexStateMask;
        if (!next) continue;
        for (int sym = 0; sym < p.n_syms; ++sym)
            if (p.trans[size_t(next) * ns + size_t(sym)] != kRegexMatchBit) return false;   // a match that ended here, then dead
        match_class[c] = 1;
        any = true;
    }
    return any;
}

}  // namespace

int build_subst_plan(const std::string& pattern, const std::string& replace, bool global, SubstPlan& out, std::string& err) {
    out = SubstPlan{};
    out.global = global;
    const std::string tmpl = subst_reformat_replace_pattern(replace);
    out.tmpl_len = int(tmpl.size());
    RegexWithGroups rx;
    if (int rc = compile_regex_groups(subst_fix_search_pattern(pattern), rx, err)) return rc;
    if (rx.invalid) {
        out.identity = true;
        out.identity_why = "PCRE2 rejects the pattern (" + rx.whole.invalid_why + ")";
        return OVTK_OK;
    }
    std::vector<TemplatePart> parts;
    std::string why;
    const int t = parse_template(tmpl, rx, parts, why);
    if (t == 2) {
        err = "RegexNormalization: " + why + " is not supported";
        return OVTK_E_UNSUPPORTED;
    }
    if (t == 1) {
        out.identity = true;
        out.identity_why = why;
        return OVTK_OK;
    }
    // does a referenced group lie at the same place in every alternative?
    bool split = false;
    for (const TemplatePart& p : parts) {
        if (!p.is_group) continue;
        bool placed = false;
        for (const RegexAlternative& a : rx.alts) {
            const RegexGroupSpan& s = a.groups[size_t(p.group)];
            if (s.front == kGroupLook) {
                err = "RegexNormalization: the template refers to group " + std::to_string(p.group) +
                      ", which stands inside a look-around; its span is not part of the match (PCRE2 is not executed on the device)";
                return OVTK_E_UNSUPPORTED;
            }
            if (s.front == kGroupLoose) {
                err = "RegexNormalization: the template refers to group " + std::to_string(p.group) +
                      ", which stands under a quantifier or inside an inner alternation, or whose surroundings are not of a fixed length; "
                      "its span cannot be told from the match's start and end (PCRE2 is not executed on the device)";
                return OVTK_E_UNSUPPORTED;
            }
            placed = placed || s.front != kGroupUnset;
            const RegexGroupSpan& s0 = rx.alts[0].groups[size_t(p.group)];
            if (s.front != s0.front || s.back != s0.back) split = true;
        }
        if (!placed) {
            err = "RegexNormalization: the template refers to group " + std::to_string(p.group) + ", which no alternative of the pattern holds at a fixed place";
            return OVTK_E_UNSUPPORTED;
        }
    }
    // the segments (literal offsets are the same for every alternative)
    std::vector<int> lit_at;
    for (const TemplatePart& p : parts) {
        lit_at.push_back(int(out.lits.size()));
        if (!p.is_group) {
            out.lits += p.lit;
            out.lit_total += int(p.lit.size());
        } else {
            ++out.n_refs;
        }
    }
    auto fill = [&](const RegexAlternative& a, SubstPlan::Alt& to) {
        for (size_t k = 0; k < parts.size(); ++k) {
            if (!parts[k].is_group) to.segs.push_back(SubstSeg{0, lit_at[k], int(parts[k].lit.size())});
            else {
                const RegexGroupSpan& s = a.groups[size_t(parts[k].group)];
                if (s.front == kGroupUnset) to.has_unset = true;
                to.segs.push_back(SubstSeg{1, s.front == kGroupUnset ? 0 : s.front, s.back});
            }
        }
    };
    out.all_anchored = true;
    for (const RegexAlternative& a : rx.alts) out.all_anchored = out.all_anchored && a.anchored;
    if (split) {
        for (RegexAlternative& a : rx.alts) {
            SubstPlan::Alt to;
            fill(a, to);
            to.rc_min = a.rc_min;
            to.rc_max = a.rc_max;
            to.prog = std::move(a.prog);
            out.alts.push_back(std::move(to));
        }
    } else {
        SubstPlan::Alt to;
        fill(rx.alts[0], to);
        to.rc_min = rx.alts[0].rc_min;
        to.rc_max = rx.alts[0].rc_max;
        for (const RegexAlternative& a : rx.alts) {
            to.rc_min = std::min(to.rc_min, a.rc_min);
            to.rc_max = std::max(to.rc_max, a.rc_max);
        }
        to.prog = std::move(rx.whole);
        out.alts.push_back(std::move(to));
    }
    // the class path
    if (!split && global && out.n_refs <= 1 && one_character_program(out.alts[0].prog, out.match_class)) {
        bool whole_match = true;
        for (const SubstSeg& s : out.alts[0].segs) whole_match = whole_match && (s.kind == 0 || (s.a == 0 && s.b == 0));
        if (whole_match) {
            out.class_path = true;
            for (const TemplatePart& p : parts) {
                if (p.is_group) out.class_has_ref = true;
                else (out.class_has_ref ? out.class_suf : out.class_pre) += p.lit;
            }
        }
    }
    return OVTK_OK;
}

}  // namespace ovtk
