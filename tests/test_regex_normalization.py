"""RegexNormalization (csrc/regex_subst.cpp -> plan, csrc/regex_subst_kernels.hpp) vs pcre2_substitute as the reference calls it
(tests/pcre2_substitute.py over the system's libpcre2-8): whole begins / ends / chars arrays, no tolerance.  The reference's known
answers, every constructor of RegexNormalizationStep / RegexDecodingStep, pcre2_substitute's empty-match rule, the per-string identity
quirks (unset group, the 4 * (len + rc * template_len) buffer), skips / layout / capacity, the refusals, class path == general path,
and the steps inside a Pipeline.  The yardstick's PCRE2 is 10.39, the reference pins 10.46: the patterns and characters here mean the
same in both (\\p{Han} only over characters whose Script and Script_Extensions agree)."""
import ctypes as C
import json
import os
from pathlib import Path

import numpy as np
import pytest

from openvino_tokenizers_amd import _lib as L
from openvino_tokenizers_amd import pipeline as P
from openvino_tokenizers_amd.ops import RegexNormalization
from tests.pcre2_substitute import Substitute, normalize
from tests.test_regex_general import strings_for

KATS = json.loads((Path(__file__).parent / "golden" / "regex_normalization_kats.json").read_text())["rows"]
ALPHABET = [" ", "  ", "\t", "\n", "\r", "\x01", "​", "▁", "́", "元", "気", "'", ",", ".", "!", "?", "s", "m", "n", "t", "r", "e", "v", "a", "é", "x"]


def pack(strs):
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in strs]
    ends = np.cumsum([len(b) for b in bs], dtype=np.int64).astype(np.int32) if bs else np.zeros(0, np.int32)
    begins = np.concatenate([[0], ends[:-1]]).astype(np.int32) if bs else np.zeros(0, np.int32)
    return bs, begins, ends, np.frombuffer(b"".join(bs), np.uint8)


def u8(s):
    return np.frombuffer(s.encode() if isinstance(s, str) else s, np.uint8)


def run_op(backend, packed, pattern, replace, global_replace=True, skips=None, **kw):
    _, b, e, c = packed
    op = RegexNormalization(global_replace, lib=backend.lib)
    ins = backend.data([b, e, c]) + ([backend.data([np.asarray(skips, np.uint8)])[0]] if skips is not None else []) + [u8(pattern), u8(replace)]
    return [backend.host(x) for x in op.evaluate(ins, **kw)]


def same(got, ref, what):
    for k, name in enumerate(("begins", "ends", "chars")):
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        if g.shape != r.shape or not np.array_equal(g, r):
            n = min(len(got[0]), len(ref[0]))
            for i in range(n):   # the first string that differs, for the message
                gs, rs = bytes(got[2][got[0][i]:got[1][i]]), bytes(ref[2][ref[0][i]:ref[1][i]])
                assert gs == rs, f"{what}: string {i}: got {gs!r}, PCRE2 {rs!r}"
            raise AssertionError(f"{what}: {name} differ")


_REF = {}


def check(backend, pattern, replace, packed, global_replace=True, skips=None, key=None, fix_pattern=True):
    k = (pattern, replace, global_replace, key)
    if key is None or skips is not None or k not in _REF:
        ref = normalize(packed[0], pattern, replace, global_replace, skips, fix_pattern)
        if key is not None and skips is None:
            _REF[k] = ref
    else:
        ref = _REF[k]
    got = run_op(backend, packed, pattern, replace, global_replace, skips)
    same(got, ref, f"{pattern!r} -> {replace!r}")
    return got


_CORPUS = {}


def corpus(backend):
    """Item 2's strings: the alphabet's products, random short and medium rows, "", one long row, rows of 63 / 64 / 65 characters, and
    multi-byte characters across byte 64 and byte 2048."""
    name = "emu" if backend.name == "emu" else "gpu"
    if name not in _CORPUS:
        strs = strings_for(backend, ALPHABET, 17, n_emu=250, n_gpu=3000)
        rng = np.random.default_rng(4)
        strs += ["".join(rng.choice(ALPHABET, size=24000))]   # ~70 KB with the multi-byte characters
        strs += ["a" * 63, "a" * 64, "a" * 65, " " * 64, "元" * 63, "元" * 64, "元" * 65, "a" * 63 + "元", "a" * 62 + "元 ", "a" * 61 + "́元", "a" * 2047 + "元x",
                 "a" * 2046 + "元 ", " " * 2045 + "気元", "x" * 62 + "​" + " ", "a" * 63 + "é" * 3]
        _CORPUS[name] = pack(strs)
    return name, _CORPUS[name]


# ---------------------------------------------------------------------------------------------- 1. the reference's known answers
def test_known_answers_yardstick():
    assert len(KATS) == 14
    for r in KATS:
        assert Substitute(r["pattern"], r["replace"], r["global_replace"])(r["input"].encode()).decode() == r["expected"], r


def test_known_answers(backend):
    for r in KATS:
        got = run_op(backend, pack([r["input"]]), r["pattern"], r["replace"], r["global_replace"])
        assert bytes(got[2]).decode() == r["expected"], r
        assert list(got[0]) == [0] and list(got[1]) == [len(r["expected"].encode())]


# ---------------------------------------------------------------------------------------------- 2. every constructor
NORM = P.RegexNormalizationStep
DEC = P.RegexDecodingStep


class _Spec:   # the constructors build (pattern, template, global) without a library
    def __init__(self, regex_search_pattern, replace_term, global_replace=True, lib=None):
        self.args = (regex_search_pattern, replace_term, global_replace)


def _spec(cls, name, *args):
    return getattr(cls, name).__func__(_Spec, *args).args


CONSTRUCTORS = {
    "strip_accents": _spec(NORM, "strip_accents_regex"), "add_prefix_whitespace": _spec(NORM, "add_prefix_whitespace_regex"),
    "add_prefix_whitespace_to_not_whitespace": _spec(NORM, "add_prefix_whitespace_to_not_whitespace_regex"),
    "replace_whitespace": _spec(NORM, "replace_whitespace_regex"), "handle_chinese_chars": _spec(NORM, "handle_chinese_chars_regex"),
    "replace_spaces_metaspace": _spec(NORM, "replace_spaces_metaspace"), "prepend": _spec(NORM, "prepend_regex", "▁"),
    "prepend_with_check": _spec(NORM, "prepend_with_check_regex", "▁", "▁"), "del_control_chars": _spec(NORM, "del_control_chars_regex"),
    "strip": _spec(NORM, "clean_up_and_remove_extra_whitespaces_regex"), "strip_left": _spec(NORM, "strip_regex", True, False),
    "strip_right": _spec(NORM, "strip_regex", False, True),
    "clean_up_tokenization_spaces": _spec(DEC, "clean_up_tokenization_spaces"), "rstrip_space": _spec(DEC, "rstrip_space"),
    "strip_forward_space": _spec(DEC, "strip_forward_space"), "strip_forward_space_before_not_space": _spec(DEC, "strip_forward_space_before_not_space"),
    "replace_sp_spaces": _spec(DEC, "replace_sp_spaces"), "replace_end_of_word_suffix": _spec(DEC, "replace_end_of_word_suffix", "s"),
    "replace_continuing_subword_prefix": _spec(DEC, "replace_continuing_subword_prefix", "''"),
    "parse_strip_dict": _spec(DEC, "parse_strip_dict", {"content": " "}), "parse_replace_dict": _spec(DEC, "parse_replace_dict", {"pattern": {"String": "▁"}, "content": " "}),
}
CLASS_PATH = ["strip_accents", "replace_whitespace", "handle_chinese_chars", "replace_spaces_metaspace", "del_control_chars", "replace_sp_spaces"]


@pytest.mark.parametrize("name", list(CONSTRUCTORS))
def test_constructors(backend, name):
    pattern, replace, g = CONSTRUCTORS[name]
    key, packed = corpus(backend)
    check(backend, pattern, replace, packed, g, key=key)


# ---------------------------------------------------------------------------------------------- 3. semantics
SEMANTICS = [
    (r"\s*$", "X", True), (r"\s*", "X", True), (r"x*", "-", True), (r"^\s*|\s*$", "<>", True), ("", "-", True),   # the five empty-match rows
    (r"^", "<", True), (r"^a", "X", True), (r"^a*", "X", True), (r"\Aa|b", "X", True),                          # `^` matches once
    (r"(?<=a)a", "b", True), (r"(?<=x)a", "x", True), (r"(?<! )x", " ", True), (r"\bs", " ", True),           # look-behind sees the original text
    (r"a", "X", False), (r"\s+", "_", False), (r"x*", "-", False), (r"(a)|s", "$0$0", False),                   # non-global
    (r"a", "$$", True), (r"(a)(x)", "${2}x$0${1}", True), (r"(?<w>a)x", "$w-${w}", True), (r"(?P<first>.)(?<second>.)", "${second}$first", True),
    (r"x(a)|(s)s", "[$1]", True), (r"(?|x(a)|(s)s|m(e)n)", "<$1>", True), (r"a(s)x|as", "($0)", True), (r"(?:x(a)|(a)x)", "$0", True),   # geometry differs
    (r"ab|a", "<$0>", True), (r"a|ab", "<$0>", True), (r"as|a|s", "[$0]", True), (r"(?|(a)s|(a))", "{$1}", True),      # leftmost ties
    (r"a(?=s)", "A", True), (r"\s+(?!\S)", "_", True), (r"(a|x)(s)", "$2$1", True), (r"x(?:a|e)(s)", "$1", True), (r"([ae])\s(s)", "$2 $1", True),
    (r"(^ )([^ ])", "$2", True), (r"é|元", "$0$0", True), (r"(.)(.)(.)", "$3$2$1", True), (r"(?s)(.)$", "<$1>", True),
]
SEM_ALPHABET = ["a", "b", "x", "s", "e", "m", "n", " ", "\n", "é", "元", ""]


@pytest.mark.parametrize("pattern,replace,global_replace", SEMANTICS)
def test_semantics(backend, pattern, replace, global_replace):
    strs = strings_for(backend, SEM_ALPHABET, 3, n_emu=200, n_gpu=3000) + ["a  ", "a b", "axxb", "  a  ", "é元", "ab", "aa", "xa ss men", "asx as", "abab"]
    check(backend, pattern, replace, pack(strs), global_replace)


def test_empty_match_table(backend):
    """The rows the issue lists, as literal expectations (checked with PCRE2 10.39)."""
    for pattern, replace, subject, expected in [(r"\s*$", "X", "a  ", "aXX"), (r"\s*", "X", "a b", "XaXXbX"), (r"x*", "-", "axxb", "-a--b-"),
                                                (r"^\s*|\s*$", "<>", "  a  ", "<>a<><>"), ("", "-", "é元", "-é-元-")]:
        assert Substitute(pattern, replace)(subject.encode()).decode() == expected
        assert bytes(run_op(backend, pack([subject]), pattern, replace)[2]).decode() == expected


# ---------------------------------------------------------------------------------------------- 4. identity quirks
def test_unset_group_turns_the_string_back(backend):
    got = check(backend, r"(a)|b", "[$1]", pack(["ab", "aa", "b", "a", "xax", "xbx", ""]))
    assert bytes(got[2]) == b"ab" + b"[a][a]" + b"b" + b"[a]" + b"x[a]x" + b"xbx"


def test_unrewritten_clean_up_pattern(backend):
    """Without the (?| ) the reference's rewrite adds, groups 2..5 leave $1 unset: strings with 's come back whole."""
    pattern = r" ([\\.\\?\\!,])| ('[ms])| (') | ('[rv]e)| (n't)"
    strs = ["it 's , ok", "a , b .", "do n't !", "x ' y", "plain", " ,", "we 've , x"]
    packed = pack(strs)
    ref = normalize(packed[0], "(?:" + pattern + ")", "$1")   # (the same pattern, kept from the rewrite table)
    got = run_op(backend, packed, "(?:" + pattern + ")", "$1")
    same(got, ref, "un-rewritten clean-up")
    out = [bytes(got[2][got[0][i]:got[1][i]]).decode() for i in range(len(strs))]
    assert out[0] == "it 's , ok" and out[1] == "a, b." and out[5] == ","


@pytest.mark.parametrize("pattern,replace", [(r"(a)", "$2"), (r"a", "x$"), (r"a", "${1"), (r"a", "$w"), (r"a(", "x"), (r"a**", "x"), (r"[b-a]", "x")])
def test_identity_for_the_whole_op(backend, pattern, replace):
    packed = pack(["a", "banana", "", "xyz", "a" * 100])
    got = check(backend, pattern, replace, packed)
    assert bytes(got[2]) == b"".join(packed[0])


@pytest.mark.parametrize("template_len", [8, 10])
def test_buffer_bound(backend, template_len):
    """out_len + 1 > 4 * (len + rc * template_len) gives the subject back: both sides of the bound, among ordinary rows."""
    strs = ["a" * k for k in range(0, 14)] + ["a" * k + "b" for k in range(0, 14)] + ["hello", "banana", "b" * 40, "aaaaaaaa", "aaaaaaaab", "a" * 300, "ab" * 50]
    got = check(backend, "a", "X" * template_len, pack(strs))
    out = [bytes(got[2][got[0][i]:got[1][i]]) for i in range(len(strs))]
    if template_len == 8:
        assert out[strs.index("aaaaaaaa")] == b"aaaaaaaa" and out[strs.index("aaaaaaaab")] == b"X" * 64 + b"b"
    else:
        assert out[9] == b"a" * 9 and out[10] == b"a" * 10
    # a group that is set raises rc: (a) has rc 2
    check(backend, "(a)", "Y" * template_len, pack(strs))


def test_buffer_bound_with_open_rc(backend):
    """Unreferenced optional groups leave rc open: decided where both bounds agree, OVTK_E_UNSUPPORTED (nothing written) between them."""
    check(backend, "(x)?a", "XX", pack(["a", "xa", "aaa", "hello a", ""]))           # far below both bounds
    check(backend, "(x)?a", "X" * 40, pack(["a" * 50, "a" * 64]))                     # above both: 41 * len > 4 * (len + 2 * 40)
    with pytest.raises(L.OvtkError) as err:
        run_op(backend, pack(["a" * 5]), "(x)?a", "X" * 40)                          # 201 is above 4 * 45 and not above 4 * 85
    assert err.value.code == L.E_UNSUPPORTED


@pytest.mark.parametrize("pattern", [r"x(?=(a))", r"(?<=(x))a", r"(?=(x))x", r"x(?!(b))", r"(?=(x)(a))x"])
def test_buffer_bound_with_a_group_inside_a_look_around(backend, pattern):
    """PCRE2 sets the group of a look-around that held, and the first pcre2_match returns 1 + its number: the buffer is sized with it.
    Such a group raises the highest rc the plan reckons with, so a string is either decided as PCRE2 decides it or refused
    (OVTK_E_UNSUPPORTED) -- never decided with too small an rc."""
    decided = refused = 0
    for k in list(range(1, 34)):
        packed = pack(["xa" * k])
        try:
            got = run_op(backend, packed, pattern, "X" * 10)
        except L.OvtkError as err:
            assert err.code == L.E_UNSUPPORTED, (pattern, k)
            refused += 1
            continue
        same(got, normalize(packed[0], pattern, "X" * 10), f"{pattern!r} on 'xa' * {k}")
        decided += 1
    assert decided >= 5 and (refused >= 5 or pattern == r"x(?!(b))")
    with pytest.raises(L.OvtkError) as err:   # and a template cannot refer to it
        run_op(backend, pack(["xa"]), pattern, "<$1>")
    assert err.value.code == L.E_UNSUPPORTED and "look-around" in str(err.value)


# ---------------------------------------------------------------------------------------------- the host differential
def test_host_differential_fixed_sample():
    """A fixed sample of tools/fuzz_regex_subst_host.py: random patterns and templates, the plan run on the host by
    tools/regex_subst_host_check.cpp (the matcher tables + a plain C++ restatement of the kernel's loop) against the yardstick."""
    from tools import fuzz_regex_subst_host as F
    F.build()
    rng = np.random.default_rng(2026)
    strings = F.subjects(rng)
    seen = {"same": 0, "unsupported": 0}
    plans = set()
    for _ in range(300):
        case = F.gen_case(rng)
        verdict, info = F.run_case(*case, strings)
        assert verdict != "BAD", (case, info)
        seen[verdict] += 1
        plans.add(info.split(" undecided")[0])
    assert seen["same"] >= 200
    assert {"PLAN identity alts=0", "PLAN class alts=1", "PLAN general alts=1", "PLAN general alts=2"} <= plans


# ---------------------------------------------------------------------------------------------- 5. skips and layout
def test_skips_pass_through(backend):
    key, packed = corpus(backend)
    n = len(packed[0])
    skips = (np.arange(n) % 3 == 1)
    bs, b, e, c = packed
    op = RegexNormalization(True, lib=backend.lib)
    sk = backend.data([skips.astype(np.uint8)])[0]
    out = op.evaluate(backend.data([b, e, c]) + [sk, u8(r"\s"), u8("_")])
    assert len(out) == 4 and out[3] is sk
    same([backend.host(x) for x in out[:3]], normalize(bs, r"\s", "_", True, skips), "skips")
    check(backend, r"(a)|(e)", "<$1>", packed, skips=skips)   # (the general path, with strings that come back whole)


def test_scattered_input_layout(backend):
    """Begins that do not start at 0, strings not adjacent and out of order: the output is back to back from 0."""
    pieces = [b"..", b"hello world", b"--", b"a b c", b"__", b"  x  ", b"..", "元 気".encode(), b"!"]
    at = np.concatenate([[0], np.cumsum([len(x) for x in pieces])])
    chars = np.frombuffer(b"".join(pieces), np.uint8)
    order = [5, 1, 3, 7]   # out of order, with gaps between them
    b = np.array([at[k] for k in order] + [5], np.int32)
    e = np.array([at[k + 1] for k in order] + [5], np.int32)
    strs = [pieces[k] for k in order] + [b""]
    op = RegexNormalization(True, lib=backend.lib)
    for pattern, replace in [(r"\s", "_"), (r"(\S)\s", "$1$1")]:
        got = [backend.host(x) for x in op.__class__(True, lib=backend.lib).evaluate(backend.data([b, e, chars]) + [u8(pattern), u8(replace)])]
        same(got, normalize(strs, pattern, replace), "scattered")
    with pytest.raises(L.OvtkError) as err:
        op.evaluate(backend.data([b, np.array([at[6], at[2], at[4], 99, 5], np.int32), chars]) + [u8("a"), u8("b")])
    assert err.value.code == L.E_RANGE


def test_capacity_protocol(backend):
    packed = pack(["a b", "元 気 ", "", "no"])
    ref = normalize(packed[0], r"\s", "___")
    need = len(ref[2])
    lib = backend.lib
    op = RegexNormalization(True, lib=lib)
    op._ensure(r"\s", "___")
    _, b, e, c = packed
    ob, oe = np.full(4, -7, np.int32), np.full(4, -7, np.int32)
    for cap in (need - 1, 0):
        oc = np.full(need + 8, 0xEE, np.uint8)
        out = L.StringsOut(ob.ctypes.data, oe.ctypes.data, oc.ctypes.data, cap, 0)
        s = L.Strings(b.ctypes.data, e.ctypes.data, c.ctypes.data, len(b), len(c))
        assert lib.ovtk_regex_normalization_run(op._h, C.byref(s), None, C.byref(out), L.MEM_HOST, None) == L.E_CAPACITY
        assert out.n_chars == need and (oc == 0xEE).all() and (ob == -7).all() and (oe == -7).all()
    got = run_op(backend, packed, r"\s", "___", chars_capacity=need)
    same(got, ref, "exact capacity")
    assert op.bound(len(b), len(c)) >= need
    with pytest.raises(L.OvtkError) as err:
        run_op(backend, packed, r"\s", "___", chars_capacity=need - 1)
    assert err.value.code == L.E_CAPACITY


def test_empty_batch_and_input_count(backend):
    got = run_op(backend, pack([]), r"\s", "_")
    assert [len(x) for x in got] == [0, 0, 0]
    with pytest.raises(L.OvtkError, match="supported input sizes are 5 or 6, got"):
        RegexNormalization(lib=backend.lib).evaluate([np.zeros(0, np.int32)] * 4)


# ---------------------------------------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("pattern,replace", [(r"(a)+", "$1"), (r"x(a|(b))", "$2"), (r"(?:(a)|b)c", "$1"), (r"(a)\1", "x"), (r"a+(b)", "$1"), (r"(a)?b", "$1")])
def test_refusals(backend, pattern, replace):
    with pytest.raises(L.OvtkError) as err:
        run_op(backend, pack(["ab"]), pattern, replace)
    assert err.value.code == L.E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- 7. both paths agree
@pytest.mark.parametrize("name", CLASS_PATH)
def test_class_path_equals_general_path(backend, name, monkeypatch):
    """OVTK_REGEX_NORM_GENERAL=1 (read at create) sends a class-path pattern down the general walk."""
    pattern, replace, g = CONSTRUCTORS[name]
    key, packed = corpus(backend)
    fast = run_op(backend, packed, pattern, replace, g)
    monkeypatch.setenv("OVTK_REGEX_NORM_GENERAL", "1")
    general = run_op(backend, packed, pattern, replace, g)
    monkeypatch.delenv("OVTK_REGEX_NORM_GENERAL")
    same(general, fast, f"{name}: general vs class path")
    same(fast, normalize(packed[0], pattern, replace, g) if (pattern, replace, g, key) not in _REF else _REF[(pattern, replace, g, key)], name)


# ---------------------------------------------------------------------------------------------- 8. inside a Pipeline
def _texts(backend):
    rng = np.random.default_rng(8)
    words = ["hello", "woŕld", "元気", "it", "'s", ",", ".", "n't", "do", "\tTab", "\x01ctl", "é́", " ", "  ", "'re", "!", "we", "x​y"]
    n = 200 if backend.name == "emu" else 3000
    return [" ".join(rng.choice(words, size=int(k))) for k in rng.integers(0, 14, size=n)]


def test_bert_normalizers_in_front_of_the_fused_chain(backend):
    """\\s -> " ", control characters deleted, Han isolated, accents stripped, then RegexSplit x2 -> Wordpiece -> tail, fused."""
    from tools.harness import pack_strings
    from tools.make_tokenizers import load_tokenizer
    from tools.workloads import ragged_rows
    lib = backend.lib
    tok = load_tokenizer("bert_small")
    bs, b, e, c = pack(_texts(backend))
    rb, re_ = ragged_rows(len(bs))
    norm = [NORM.replace_whitespace_regex(lib=lib), NORM.del_control_chars_regex(lib=lib), NORM.handle_chinese_chars_regex(lib=lib), NORM.strip_accents_regex(lib=lib)]
    consts = list(pack_strings(tok["vocab"])) + [np.asarray(tok["unk_id"], np.int32)]
    chain = [P.RegexSplitStep(P.BERT_WS, "remove", lib=lib), P.RegexSplitStep(P.BERT_PUNCT, "isolate", lib=lib),
             P.WordPieceTokenizationStep(consts, tok["suffix_indicator"], tok["max_bytes_per_word"], lib=lib),
             P.TruncationStep(30, "left", lib=lib), P.CombineSegmentsStep(prefix=[101], suffix=[102], lib=lib), P.PaddingStep(pad_value=0, lib=lib)]
    state = backend.data([rb, re_, b, e, c]) + [None]
    # the normalizers alone, against the yardstick step by step
    vals = P.Pipeline(norm).run("strings", state)
    ref = bs
    for s in norm:
        rb_, re2, rc = normalize(ref, s.regex_search_pattern, s.replace_term, s.global_replace)
        ref = [bytes(rc[x:y]) for x, y in zip(rb_, re2)]
    same([backend.host(x) for x in vals[2:5]], pack(ref)[1:], "BERT normalizers")
    # ... and the whole chain: the fused form leaves the normalizers as steps and gives what the op-by-op chain gives
    pipe = P.Pipeline(norm + chain)
    fused = pipe.fused()
    assert [type(s).__name__ for s in fused.steps] == ["RegexNormalizationStep"] * 4 + ["FusedSplitWordpieceStep", "FusedEncodeTailStep"]
    a, f = pipe.run("strings", state), fused.run("strings", state)
    assert len(a) == len(f)
    for x, y in zip(a, f):
        assert np.array_equal(backend.host(x), backend.host(y))


def test_detokenizer_tail(backend):
    """VocabDecoder -> FuzeRagged -> the clean-up steps of a detokenizer, each against the yardstick."""
    from tests.util import BpeTok
    from tools.harness import pack_strings
    lib = backend.lib
    tok = BpeTok.load("gpt2_small")
    vocab = list(pack_strings(tok.vocab))
    ids = np.random.default_rng(3).integers(0, len(tok.vocab), size=(60, 21)).astype(np.int32)
    head = [P.VocabDecoderStep(vocab, skip_tokens=[0, 5], lib=lib), P.FuseStep(lib=lib)]
    tail = [DEC.replace_sp_spaces(lib=lib), DEC.clean_up_tokenization_spaces(lib=lib), DEC.strip_forward_space(lib=lib), DEC.rstrip_space(lib=lib)]
    text = [backend.host(x) for x in P.Pipeline(head).run("tokens", backend.data([ids]))]
    got = [backend.host(x) for x in P.Pipeline(head + tail).fused().run("tokens", backend.data([ids]))]
    ref = [bytes(text[2][x:y]) for x, y in zip(text[0], text[1])]
    for s in tail:
        rb_, re2, rc = normalize(ref, s.regex_search_pattern, s.replace_term)
        ref = [bytes(rc[x:y]) for x, y in zip(rb_, re2)]
    same(got, pack(ref)[1:], "detokenizer tail")
    # the same steps over plain text with the clean-up's cases in it
    bs, b, e, c = pack([" it 's , ok . ", "do n't ! ", "▁a▁b ' c 're"])
    vals = P.Pipeline(tail).run("text", backend.data([b, e, c]))
    ref = bs
    for s in tail:
        rb_, re2, rc = normalize(ref, s.regex_search_pattern, s.replace_term)
        ref = [bytes(rc[x:y]) for x, y in zip(rb_, re2)]
    same([backend.host(x) for x in vals], pack(ref)[1:], "clean-up over text")
