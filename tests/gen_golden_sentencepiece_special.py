"""Writes tests/golden/golden_sentencepiece_special.npz: SentencepieceTokenizer's 8-input form (src/sentence_piece.cpp:200-230,
:286-329) restated over the system's libpcre2-8 and the `sentencepiece` package, for the fixture models spm_bpe_bytes, spm_bpe_unk
and spm_unigram_nfkc.  Nothing is downloaded.  Run from the repository root:

    python tests/gen_golden_sentencepiece_special.py

reference_ids() is the op's loop: the reference's pattern string (quote_meta, `\\bTOK|TOK\\b` for a token of ASCII letters only),
compiled with PCRE2_UTF | PCRE2_UCP and searched from a cursor over the whole row; every part through SentencePieceProcessor.encode
(add_bos stays the processor's option); eos and reverse as the op applies them.  PCRE2 AND THE PACKAGE ARE THE AUTHORITY.
literal_cut() is the same search without PCRE2 -- leftmost position, first token in list order, the boundary rule -- which the GPU
path (csrc/sp_special_kernels.hpp) implements: the script asserts it equal to PCRE2 on every row, and that the rows reach what they
are there for; it fails otherwise.

The system PCRE2 is 10.39 (\\w = L | N | _, Unicode 14), the reference pins 10.46 (\\w = L | N | Mn | Pc, Unicode 16).  Every
character of these rows comes from SAFE below -- assigned long before Unicode 14, no Mn, no Pc but "_" -- which the script asserts
for the neighbours of every candidate of a letters-only token: the two versions cannot differ on them.
"""
import ctypes as C
import random
import sys
import unicodedata
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from pcre2_substitute import PCRE2_UCP, PCRE2_UTF, _lib as _pcre2   # noqa: E402

G = Path(__file__).resolve().parent / "golden"
MODELS = {"bpe_bytes": "spm_bpe_bytes.model", "bpe_unk": "spm_bpe_unk.model", "nfkc": "spm_unigram_nfkc.model"}
OPTIONS = {"plain": {}, "bos": {"add_bos": True}, "eos": {"add_eos": True}, "bos_eos": {"add_bos": True, "add_eos": True},
           "reverse": {"reverse": True}, "reverse_eos": {"reverse": True, "add_eos": True}, "reverse_bos": {"reverse": True, "add_bos": True}}
TOKEN_LISTS = {
    "ctl": [("</s>", 2), ("<s>", 1), ("<unk>", 0)],
    "chat": [("sop", 9001), ("eop", 9002), ("[INST]", 9003), ("<|x|>", 9004), ("a.b*c", 9005)],   # letters only; metacharacters quoted
    "prefix": [("<a>", 31), ("<a>x", 32), ("<b>x", 33), ("<b>", 34)],   # a prefix of a later token, and of an earlier one
    "dup": [("<d>", 11), ("<e>", 12), ("<d>", 13)],                     # insert() does not overwrite: the first id holds
    "none": [],
}

_pcre2.pcre2_get_ovector_pointer_8.restype = C.POINTER(C.c_size_t)
_pcre2.pcre2_get_ovector_pointer_8.argtypes = [C.c_void_p]


# ---------------------------------------------------------------------------------------------- the reference's loop
def quote_meta(tok: bytes) -> bytes:   # sentence_piece.cpp:76-91
    return b"".join(b"\\" + bytes([c]) if c in b".^$*+?()[]{}|\\" else bytes([c]) for c in tok)


def letters_only(tok: bytes) -> bool:   # std::isalpha in the "C" locale
    return all(65 <= c <= 90 or 97 <= c <= 122 for c in tok)


def pattern_of(tokens) -> bytes:   # :206-229
    alts = []
    for t in tokens:
        q = quote_meta(t)
        alts.append(b"\\b" + q + b"|" + q + b"\\b" if letters_only(t) else q)
    return b"|".join(alts)


class Search:
    """PCRE2Wrapper::match(sentence, cursor), src/utils.cpp:396-420."""

    def __init__(self, tokens):
        pat = pattern_of(tokens)
        err, off = C.c_int(0), C.c_size_t(0)
        self.code = _pcre2.pcre2_compile_8(pat, len(pat), PCRE2_UTF | PCRE2_UCP, C.byref(err), C.byref(off), None)
        assert self.code, (pat, err.value)
        self.md = _pcre2.pcre2_match_data_create_from_pattern_8(self.code, None)

    def __del__(self):
        if getattr(self, "md", None):
            _pcre2.pcre2_match_data_free_8(self.md)
        if getattr(self, "code", None):
            _pcre2.pcre2_code_free_8(self.code)

    def __call__(self, row: bytes, cursor: int):
        if _pcre2.pcre2_match_8(self.code, row, len(row), cursor, 0, self.md, None) < 0:
            return None
        ov = _pcre2.pcre2_get_ovector_pointer_8(self.md)
        return int(ov[0]), int(ov[1])


def pcre2_cut(row: bytes, tokens, search=None):
    """The loop of :286-329 -> [("part", bytes) | ("tok", index of the first token of that text)]."""
    search = search or Search(tokens)
    out, cursor = [], 0
    while True:
        m = search(row, cursor)
        if m is None or m[0] == m[1]:
            if cursor < len(row):
                out.append(("part", row[cursor:]))
            return out
        if cursor < m[0]:
            out.append(("part", row[cursor:m[0]]))
        out.append(("tok", list(tokens).index(row[m[0]:m[1]])))
        cursor = m[1]


# ---------------------------------------------------------------------------------------------- the same search without PCRE2
def word_10_46(cp: int) -> bool:   # \w under UCP, PCRE2 >= 10.43
    if cp > 0x10FFFF:
        return False
    cat = unicodedata.category(chr(cp))
    return cat[0] in "LN" or cat in ("Mn", "Pc")


def word_10_39(cp: int) -> bool:
    return cp <= 0x10FFFF and (unicodedata.category(chr(cp))[0] in "LN" or cp == 0x5F)


def char_at(s: bytes, pos: int):
    """The character at pos as the kernels decode it (lenient: split_device.hpp, seq_char) -> (code point or None, bytes)."""
    b = s[pos]
    if b < 0x80:
        return b, 1
    if b < 0xC0:
        return None, 1
    n = min(4 if b >= 0xF0 else 3 if b >= 0xE0 else 2, len(s) - pos)
    cp, k = b & (0xFF >> (n + 1)), 1
    while k < n and s[pos + k] & 0xC0 == 0x80:
        cp = (cp << 6) | (s[pos + k] & 0x3F)
        k += 1
    return cp, k


def word_before(s: bytes, p: int, word) -> bool:
    q = p - 1
    if s[q] < 0x80:
        return word(s[q])
    while q > 0 and p - q < 4 and s[q] & 0xC0 == 0x80:
        q -= 1
    cp, k = char_at(s, q)
    return q + k == p and cp is not None and word(cp)


def match_at(s: bytes, p: int, tokens, word):
    if s[p] & 0xC0 == 0x80:
        return None
    for i, t in enumerate(tokens):
        if not s.startswith(t, p):
            continue
        if letters_only(t):
            e = p + len(t)
            front = p == 0 or not word_before(s, p, word)
            cp = char_at(s, e)[0] if e < len(s) else None
            if not front and not (e == len(s) or cp is None or not word(cp)):
                continue
        return i
    return None


def literal_cut(row: bytes, tokens, word=word_10_46):
    out, cursor, p = [], 0, 0
    while p < len(row):
        i = match_at(row, p, tokens, word)
        if i is None:
            p += 1
            continue
        if cursor < p:
            out.append(("part", row[cursor:p]))
        out.append(("tok", list(tokens).index(tokens[i])))
        cursor = p = p + len(tokens[i])
    if cursor < len(row):
        out.append(("part", row[cursor:]))
    return out


def ids_of_cut(sp, cut, token_ids, add_bos=False, add_eos=False, reverse=False):
    """Every part encoded on its own (add_bos: the processor's extra option), the tokens' ids between them; eos and reverse by the op."""
    ids = []
    for kind, v in cut:
        ids += sp.encode(v, add_bos=add_bos) if kind == "part" else [token_ids[v]]
    if add_eos:
        ids.append(sp.eos_id())
    if reverse and len(ids) > 1:
        ids.reverse()
    return ids


def reference_ids(sp, row, tokens, token_ids, search=None, **opt):
    return ids_of_cut(sp, pcre2_cut(row, tokens, search), token_ids, **opt)


# ---------------------------------------------------------------------------------------------- the rows
WORDS = ["kato", "mire", "people", "sop", "eop", "soprano", "stop", "épée", "ünto", "αβγ", "джя", "12", "7", "x_y", "漢字", "😀", "a.b", "axb*c", "s",
         "INST", "[x]", "<", ">", "<s", "d>", "|x|"]
GLUE = [" ", " ", " ", "", "  ", ".", "_", "é", "1", "\t"]
SAFE = set("".join(WORDS + GLUE) + "".join(t for toks in TOKEN_LISTS.values() for t, _ in toks) + "kIHelo")


def make_rows(rng):
    """-> rows (bytes), the token list each row is for, {name: index} of the hand-made ones."""
    rows, lists, hand = [], [], {}

    def add(name, which, s):
        if name:
            hand[name] = len(rows)
        rows.append(s.encode())
        lists.append(which)

    add("people", "chat", "people sop eop")
    add("sopx", "chat", "sopx")
    add("xsop", "chat", "xsop")
    add("xsopx", "chat", "xsopx")
    add("at_start", "chat", "[INST] kato mire")
    add("at_end", "chat", "kato mire [INST]")
    add("whole_row", "chat", "[INST]")
    add("whole_row_letters", "chat", "eop")
    add("back_to_back", "chat", "kato<|x|>[INST]mire")
    add("spaces_between", "chat", "<|x|>  [INST]")
    add("empty", "chat", "")
    add("after_digit", "chat", "1sop 1sopx")
    add("after_underscore", "chat", "_sop _sopx")
    add("after_e_acute", "chat", "ésop ésopx")
    add("quoted_metacharacters", "chat", "a.b*c axb*c a.bc [INST")
    for k in (63, 64, 65):
        add(f"parts_{k}", "chat", ".sop" * (k - 1) + ".")
    add("long_part_behind_a_cut", "chat", "kato [INST]" + "k" * 140 + "<|x|>mire")
    add("ctl_wrapped", "ctl", "<s>kato mire</s>")
    add("ctl_unk", "ctl", "<unk>")
    add("ctl_back_to_back", "ctl", "kato</s><s>mire")
    add("ctl_empty", "ctl", "")
    add("prefix_orders", "prefix", "<a>x <b>x <a> <b>")
    add("prefix_empty", "prefix", "")
    add("dup_first_id", "dup", "<d> <e> <d>")
    add("dup_empty", "dup", "")
    add("none_text", "none", "<s>kato sop")
    add("none_empty", "none", "")
    add("none_spaces", "none", "  ")
    for which, toks in TOKEN_LISTS.items():
        names = [t for t, _ in toks]
        for _ in range(112):
            out = []
            for _ in range(rng.randint(0, 14)):
                out.append(rng.choice(names) if names and rng.random() < 0.3 else rng.choice(WORDS))
                out.append(rng.choice(GLUE))
            s = "".join(out)
            while len(s.encode()) > 300:
                s = s[:-1]
            add(None, which, s)
    return rows, lists, hand


def assert_safe_neighbours(row, tokens):
    """10.39 against 10.46: no character next to a candidate of a letters-only token on which the two could differ."""
    text = row.decode()
    assert set(text) <= SAFE, set(text) - SAFE
    for t in tokens:
        if not letters_only(t):
            continue
        p = row.find(t)
        while p >= 0:
            for cp in ([char_at(row, p + len(t))[0]] if p + len(t) < len(row) else []) + ([ord(row[:p].decode()[-1])] if p else []):
                cat = unicodedata.category(chr(cp))
                assert cat != "Mn" and cat != "Cn" and (cat != "Pc" or cp == 0x5F) and word_10_39(cp) == word_10_46(cp), (row, hex(cp))
            p = row.find(t, p + 1)


def main():
    import sentencepiece as spm
    for ch in SAFE:
        cat = unicodedata.category(ch)
        assert cat not in ("Mn", "Cn") and (cat != "Pc" or ch == "_"), (ch, cat)
    rows, lists, hand = make_rows(random.Random(20260117))
    assert 550 <= len(rows) <= 650 and max(map(len, rows)) <= 300
    toks = {k: [t.encode() for t, _ in v] for k, v in TOKEN_LISTS.items()}
    tids = {k: [i for _, i in v] for k, v in TOKEN_LISTS.items()}
    search = {k: Search(v) for k, v in toks.items()}
    cuts = []
    for row, which in zip(rows, lists):
        assert_safe_neighbours(row, toks[which])
        cut = pcre2_cut(row, toks[which], search[which])
        assert cut == literal_cut(row, toks[which], word_10_39) == literal_cut(row, toks[which], word_10_46), (row, which, cut)
        cuts.append(cut)

    # what the rows are there for
    P, T = (lambda s: ("part", s.encode())), (lambda k: ("tok", k))
    at = lambda name: cuts[hand[name]]   # noqa: E731
    assert at("people") == [P("people "), T(0), P(" "), T(1)]
    assert at("sopx") == [T(0), P("x")] and at("xsop") == [P("x"), T(0)] and at("xsopx") == [P("xsopx")]
    assert at("at_start")[0] == T(2) and at("at_end")[-1] == T(2) and at("whole_row") == [T(2)] and at("whole_row_letters") == [T(1)]
    assert at("back_to_back") == [P("kato"), T(3), T(2), P("mire")]
    assert at("spaces_between") == [T(3), P("  "), T(2)]
    assert at("after_digit") == [P("1"), T(0), P(" 1sopx")] and at("after_underscore") == [P("_"), T(0), P(" _sopx")]
    assert at("after_e_acute") == [P("é"), T(0), P(" ésopx")]
    assert at("quoted_metacharacters") == [T(4), P(" axb*c a.bc [INST")]
    for k in (63, 64, 65):
        assert sum(kind == "part" for kind, _ in at(f"parts_{k}")) == k
    assert any(kind == "part" and len(v) > 128 and b" " not in v for kind, v in at("long_part_behind_a_cut")[1:])
    assert at("prefix_orders") == [T(0), P("x "), T(2), P(" "), T(0), P(" "), T(3)]
    assert at("dup_first_id") == [T(0), P(" "), T(1), P(" "), T(0)]
    assert at("none_text") == [P("<s>kato sop")] and at("none_empty") == [] and at("empty") == []

    out = {"chars": np.frombuffer(b"".join(rows), np.uint8), "ends": np.cumsum([len(r) for r in rows]).astype(np.int32),
           "row_list": np.array(lists), "hand_names": np.array(sorted(hand)), "hand_index": np.array([hand[k] for k in sorted(hand)], np.int32),
           "list_names": np.array(list(TOKEN_LISTS))}
    for k in TOKEN_LISTS:
        out[f"tok_{k}_chars"] = np.frombuffer(b"".join(toks[k]), np.uint8)
        out[f"tok_{k}_ends"] = np.cumsum([len(t) for t in toks[k]]).astype(np.int32)
        out[f"tok_{k}_ids"] = np.array(tids[k], np.int32)
    for name, file in MODELS.items():
        sp = spm.SentencePieceProcessor(model_proto=(G / file).read_bytes())
        assert sp.get_piece_size() < 9001
        for opt, kw in OPTIONS.items():
            ids = [ids_of_cut(sp, cut, tids[which], **kw) for cut, which in zip(cuts, lists)]
            e = ids[hand["empty"]]
            assert e == ([sp.eos_id()] if kw.get("add_eos") else []), (opt, e)   # an empty row: no bos, the op's eos
            s = ids[hand["spaces_between"]]
            plain = [9004] + ([sp.bos_id()] if kw.get("add_bos") else []) + [9003] + ([sp.eos_id()] if kw.get("add_eos") else [])
            assert s == (plain[::-1] if kw.get("reverse") else plain), (opt, s)   # a part of spaces: no ids of its own, one bos
            flat = np.array([x for r in ids for x in r], np.int64)
            assert flat.min() >= 0 and flat.max() < 65536
            out[f"{name}_{opt}_ids"] = flat.astype(np.uint16)
            out[f"{name}_{opt}_ends"] = np.cumsum([len(x) for x in ids]).astype(np.int32)
    np.savez_compressed(G / "golden_sentencepiece_special.npz", **out)
    size = (G / "golden_sentencepiece_special.npz").stat().st_size
    assert size < 1_000_000, size
    print(f"{len(rows)} rows, {size} bytes")


if __name__ == "__main__":
    main()
