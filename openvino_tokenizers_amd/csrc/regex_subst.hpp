// regex_subst.hpp -- host side of RegexNormalization: the substitution plan.
//
// The reference hands pattern and template to pcre2_substitute (PCRE2Wrapper::substitute, src/utils.cpp:315-382; the op:
// src/regex_normalization.cpp).  PCRE2 is not run on the device; create() turns the two strings into
//   * the pattern's matcher tables (regex_compile.cpp: compile_regex_groups) -- ONE program for the whole pattern, or one per top-level
//     alternative where the template refers to a group whose place differs between the alternatives (or that some of them lack): the
//     match at a position is then the first alternative that matches there, which is PCRE2's choice because nothing follows a
//     top-level alternation;
//   * the template as segments: literal bytes, or the span of a group relative to the match (RegexGroupSpan);
//   * what the per-string quirks need: pcre2_match's return value for a first match (between rc_min and rc_max), which alternatives
//     leave a referenced group unset.
// A pattern PCRE2 rejects, a template with a syntax error or with a group the pattern does not have make the op the identity, as the
// reference's "any negative code gives the input back" does.  A group reference whose span is not fixed is OVTK_E_UNSUPPORTED.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "regex_compile.hpp"

namespace ovtk {

struct SubstSeg {
    int kind;   // 0: the literal bytes lits[a, a + b); 1: the group [match start + a characters, match end - b characters)
    int a, b;
};

struct SubstPlan {
    bool identity = false;            // every string comes back unchanged
    std::string identity_why;
    bool global = true;
    int tmpl_len = 0;                 // bytes of the reformatted template (the reference's buffer size counts them)
    std::string lits;
    int lit_total = 0, n_refs = 0;    // per match: literal bytes, group references (for the output bound)
    struct Alt {
        RegexProgram prog;
        std::vector<SubstSeg> segs;
        int rc_min = 1, rc_max = 1;
        bool has_unset = false;       // the template refers to a group a match of this alternative leaves unset
    };
    std::vector<Alt> alts;            // one (the whole pattern), or the top-level alternatives
    bool all_anchored = false;        // every alternative starts with `^` / `\A`: nothing can match behind offset 0
    // the class path: every match is exactly one character, decided by that character's class alone (read off the compiled tables)
    bool class_path = false;
    uint8_t match_class[256] = {};
    bool class_has_ref = false;       // the template holds the matched character ($0, or a group that equals the match) -- once
    std::string class_pre, class_suf; // the literal bytes in front of it and behind it (all of the template without one)
};

// The reference's two rewrites of its inputs (src/regex_normalization.cpp:19-53).
std::string subst_fix_search_pattern(const std::string& pattern);
std::string subst_reformat_replace_pattern(std::string replace);

// 0, or OVTK_E_UNSUPPORTED with `err`.
int build_subst_plan(const std::string& pattern, const std::string& replace, bool global, SubstPlan& out, std::string& err);

}  // namespace ovtk
