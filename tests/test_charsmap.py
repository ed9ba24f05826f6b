"""CharsMapNormalization / NormalizeUnicode / CaseFold (src/charsmap_normalization.cpp:34-69, src/normalize_unicode.cpp:32-62,
src/case_fold.cpp:34-73): the kernels against tests/charsmap_ref.py, the restatement against sentencepiece's own normalizer
(tests/golden/golden_charsmap.npz, written by tests/gen_golden_charsmap.py).  Every comparison is of whole begins / ends / chars
arrays, no tolerance anywhere."""
import ctypes as C
import struct
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O
from tests.charsmap_ref import CharsMapRef, case_fold_ascii, utf8_char_len
from tests.util import assert_same

G = Path(__file__).resolve().parent / "golden"
BLOBS = ("nfkc", "nmt_nfkc_cf", "small")
SYMBOL = "▁".encode("utf-8")


def flags_of(f):
    return dict(add_dummy_prefix=bool(f & 1), remove_extra_whitespaces=bool(f & 2), escape_whitespaces=bool(f & 4))


_golden_cache = {}


def golden():
    if not _golden_cache:
        z = np.load(G / "golden_charsmap.npz")
        ends = z["in_ends"]
        begins = np.concatenate([[0], ends[:-1]])
        data = bytes(z["in_chars"])
        strings = [data[x:y] for x, y in zip(begins, ends)]
        lens, out = z["out_lens"], bytes(z["out_chars"])
        offs = np.concatenate([[0], np.cumsum(lens.reshape(-1).astype(np.int64))])
        _golden_cache.update(strings=strings, blobs={k: bytes(z["blob_" + k]) for k in BLOBS}, lens=lens, out=out, offs=offs)
    return _golden_cache


def golden_out(g, i, j, f):
    at = (i * len(BLOBS) + j) * 8 + f
    return g["out"][g["offs"][at]:g["offs"][at + 1]]


def _op(backend, blob=None, form="", **flags):
    from openvino_tokenizers_amd.ops import CharsMapNormalization
    return CharsMapNormalization(lib=backend.lib, normalization_form=form, charsmap=blob if form else None, **flags)


def _check(backend, blob, strings, skips=None, what="", calls=1, **flags):
    """The op (charsmap as its last input) on `strings` == the restatement; returns the output strings."""
    flags = {**flags_of(0), **flags}   # (the op's defaults are the reference's: remove_extra_whitespaces is on there)
    b, e, c = O.pack_strings(strings)
    ref = CharsMapRef(blob, **flags)(b, e, c, skips)
    op = _op(backend, **flags)
    blob_in = np.frombuffer(blob, np.uint8)
    for call in range(calls):
        ins = backend.data([b, e, c]) + ([backend.data([np.asarray(skips, bool)])[0]] if skips is not None else []) + [blob_in]
        got = op.evaluate(ins)
        assert_same(list(ref), got[:3], backend.host, f"{what} {flags} call {call}")
    return [bytes(ref[2][x:y]) for x, y in zip(ref[0], ref[1])]


def make_blob(mapping):
    """A charsmap from {key: replacement}: a double array in Darts' unit layout (one block, base found by search), the replacement strings."""
    keys = sorted(mapping)
    strings, value_of = b"", {}
    for k in keys:
        value_of[k] = len(strings)
        strings += mapping[k] + b"\0"
    units, used, bases = {}, {0}, set()
    # node: (unit index that holds its label / leaf flag, prefix); children placed at base ^ c with base < 2^21 (offset = base ^ index, << 0 form)

    def place(index, prefix):
        kids = sorted({k[len(prefix)] for k in keys if k.startswith(prefix) and len(k) > len(prefix)})
        leaf = prefix in value_of
        labels = ([0] if leaf else []) + kids
        base = 0
        while True:
            base += 1
            if base not in bases and (base ^ index) < (1 << 21) and all((base ^ c) not in used for c in labels):   # (a base serves one node)
                break
        bases.add(base)
        for c in labels:
            used.add(base ^ c)
        units[index] = (units.get(index, 0) & 0x800000FF) | ((base ^ index) << 10) | (0x100 if leaf else 0)
        if leaf:
            units[base] = 0x80000000 | value_of[prefix]
        for c in kids:
            units[base ^ c] = c
            place(base ^ c, prefix + bytes([c]))

    place(0, b"")
    arr = np.zeros(max(units) + 1, "<u4")
    for i, u in units.items():
        arr[i] = u
    for i in range(len(arr)):   # unused slots must not look like children: a label no byte has
        if i not in units:
            arr[i] = 0x80000000
    return struct.pack("<I", 4 * len(arr)) + arr.tobytes() + strings


SMALL = {b"ab": b"", b"q": b"  ", b"xy": b" X", b"zz": b"Z ", b"w": b" ", b"abc": b"LONG", b"a": b"A", b"k": b"0123456789!", b"mnopqrstuvwx": b"#"}


# ---------------------------------------------------------------------------------------------- 1. the restatement against sentencepiece
def test_restatement_matches_sentencepiece():
    """Passes without the op: it pins the yardstick.  The golden is not soft: a quarter of the strings change under nfkc, a hundred hold
    malformed UTF-8, a hundred hit a key of more than one character."""
    g = golden()
    strings = g["strings"]
    assert len(strings) == 3000 and max(map(len, strings)) <= 512
    for j, name in enumerate(BLOBS):
        for f in range(8):
            ref = CharsMapRef(g["blobs"][name], **flags_of(f))
            for i, s in enumerate(strings):
                assert ref.normalize(s) == golden_out(g, i, j, f), (name, f, i)
    assert sum(golden_out(g, i, 0, 0) != s for i, s in enumerate(strings)) * 4 >= len(strings)
    nfkc = CharsMapRef(g["blobs"]["nfkc"])

    def malformed(s):
        p = 0
        while p < len(s):
            n = utf8_char_len(s, p)
            if not n:
                return True
            p += n
        return False

    def multi_char_key(s):
        p = 0
        while p < len(s):
            n, _ = nfkc.longest_match(s, p)
            if n and utf8_char_len(s, p) and utf8_char_len(s, p) < n:
                return True
            p += n or utf8_char_len(s, p) or 1
        return False

    assert sum(map(malformed, strings)) >= 100
    assert sum(map(multi_char_key, strings)) >= 100


# ---------------------------------------------------------------------------------------------- 2. the op against the golden
@pytest.mark.parametrize("name", BLOBS)
def test_kernel_matches_golden(backend, name):
    g = golden()
    j = BLOBS.index(name)
    pick = list(range(0, 3000, 20)) if backend.name == "emu" else list(range(3000))
    strings = [g["strings"][i] for i in pick]
    for f in range(8):
        got = _check(backend, g["blobs"][name], strings, what=f"golden {name}", **flags_of(f))
        assert got == [golden_out(g, i, j, f) for i in pick]


# ---------------------------------------------------------------------------------------------- 3. the rules one by one
ALL_FLAGS = [flags_of(f) for f in range(8)]


def test_own_blob_builder_is_a_charsmap():
    ref = CharsMapRef(make_blob(SMALL))
    assert ref.longest_match(b"abcd", 0) == (3, b"LONG") and ref.longest_match(b"abd", 0) == (2, b"") and ref.longest_match(b"b", 0) == (0, None)
    assert ref.normalize(b"k") == b"0123456789!" and ref.normalize(b"mnopqrstuvwx") == b"#"


def test_longest_match_beats_shorter(backend):
    blob = make_blob(SMALL)
    assert _check(backend, blob, [b"abcab a", b"aab", b"abc"], what="longest") == [b"LONG A", b"A", b"LONG"]


def test_invalid_bytes_become_replacement_one_byte_each(backend):
    bad = [b"\xc0\x80", b"\xe0\x80\x80x", b"\xed\xa0\x80", b"\xf5\x80\x80\x80", b"\xf4\x90\x80\x80", b"\x80\xbf", b"a\xffb", b"\xf0\x9f\x98",
           b"\xef\xbf\xbd", b"\xe3\x81\x82\xe3\x81", b"\xc2", b"\xf0\x9f\x98\x80"]
    out = _check(backend, b"", bad, what="invalid")
    assert out[0] == b"\xef\xbf\xbd" * 2 and out[6] == b"a\xef\xbf\xbdb" and out[8] == b"\xef\xbf\xbd" and out[11] == b"\xf0\x9f\x98\x80"
    for fl in ALL_FLAGS:
        _check(backend, golden()["blobs"]["nfkc"], bad, what="invalid nfkc", **fl)


def test_a_row_never_reads_the_next_rows_bytes(backend):
    """E3 81 | 82: cut off at the end of row 0, and the next row's first byte would complete it; 'a' | 'bc' likewise for the key abc."""
    blob = make_blob(SMALL)
    chars = np.frombuffer(b"\xe3\x81\x82abc", np.uint8)
    b, e = np.array([0, 2, 3], np.int32), np.array([2, 3, 6], np.int32)
    ref = CharsMapRef(blob)(b, e, chars)
    assert bytes(ref[2]) == b"\xef\xbf\xbd" * 3 + b"LONG"
    got = _op(backend).evaluate(backend.data([b, e, chars]) + [np.frombuffer(blob, np.uint8)])
    assert_same(list(ref), got, backend.host, "cut off")
    b, e = np.array([3, 4], np.int32), np.array([4, 6], np.int32)
    ref = CharsMapRef(blob)(b, e, chars)
    assert bytes(ref[2]) == b"Abc"
    assert_same(list(ref), _op(backend).evaluate(backend.data([b, e, chars]) + [np.frombuffer(blob, np.uint8)]), backend.host, "cut key")


def test_nul_bytes(backend):
    for fl in ALL_FLAGS:
        _check(backend, golden()["blobs"]["nmt_nfkc_cf"], [b"\0", b"a\0b", b"\0\0 \0", b"A\0"], what="NUL", **fl)
    assert _check(backend, b"", [b"a\0b"], what="NUL") == [b"a\0b"]


def test_empty_strings_and_empty_batch(backend):
    for fl in ALL_FLAGS:
        assert _check(backend, make_blob(SMALL), [b"", b"x", b"", b""], what="empty", **fl)[0] == b""
    op = _op(backend)
    z = np.zeros(0, np.int32)
    got = op.evaluate(backend.data([z, z, np.zeros(0, np.uint8)]) + [np.frombuffer(make_blob(SMALL), np.uint8)])
    assert [len(backend.host(x)) for x in got] == [0, 0, 0]


def test_all_space_rows(backend):
    blob = make_blob(SMALL)
    rows = [b" ", b"    ", b" w ", b"q", b"w", b" q w ", b"ab", b" ab ", b"abab"]
    for fl in ALL_FLAGS:
        out = _check(backend, blob, rows, what="spaces", **fl)
        if fl["remove_extra_whitespaces"]:
            assert out == [b""] * len(rows)
    assert _check(backend, blob, [b"ab"], what="dummy on empty", add_dummy_prefix=True, escape_whitespaces=True) == [SYMBOL]


def test_trailing_literal_symbol_quirk(backend):
    rows = [b"a " + SYMBOL, b"a" + SYMBOL * 2 + b" ", SYMBOL, b"a" + SYMBOL + b"b" + SYMBOL, SYMBOL + b"a"]
    out = _check(backend, b"", rows, what="quirk", remove_extra_whitespaces=True, escape_whitespaces=True)
    assert out == [b"a", b"a", b"", b"a" + SYMBOL + b"b", SYMBOL + b"a"]
    out = _check(backend, b"", rows, what="no quirk", remove_extra_whitespaces=True)
    assert out == [b"a " + SYMBOL, b"a" + SYMBOL * 2, SYMBOL, b"a" + SYMBOL + b"b" + SYMBOL, SYMBOL + b"a"]
    for fl in ALL_FLAGS:
        _check(backend, b"", rows, what="quirk", **fl)


def test_replacements_with_spaces(backend):
    blob = make_blob(SMALL)
    rows = [b"c xyd", b"cxyd", b"c xy", b"c ab d", b"cab d", b"zzxy", b"zz xy", b"zzq", b"c q d", b"xyzz", b"q zz", b"zz", b"c  ab  ab  d", b"wxy"]
    assert _check(backend, blob, rows[:4], what="spaces", remove_extra_whitespaces=True) == [b"c Xd", b"c Xd", b"c X", b"c d"]
    for fl in ALL_FLAGS:
        _check(backend, blob, rows, what="replacement spaces", **fl)


def test_more_than_32_nested_keys():
    """Of the keys that match at a position only the first 32 (the shortest) are looked at: sentencepiece's fixed result array."""
    blob = make_blob({b"z" * k: b"%d" % k for k in range(1, 40)})
    assert CharsMapRef(blob).normalize(b"z" * 39) == b"327"


def test_first_32_matches_only(backend):
    blob = make_blob({b"z" * k: b"%d" % k for k in range(1, 40)})
    assert _check(backend, blob, [b"z" * 39, b"z" * 70, b"zz"], what="32") == [b"327", b"32326", b"2"]


# ---------------------------------------------------------------------------------------------- 4. layout and calling forms
def test_gaps_order_skips_and_forms(backend):
    from openvino_tokenizers_amd.ops import CharsMapNormalization
    g = golden()
    blob = g["blobs"]["nmt_nfkc_cf"]
    chars = np.frombuffer(b"??HELLO  World!!" + "ｈｉ ①".encode() + b"##tail ", np.uint8)
    b = np.array([16, 2, 16, 9, 28, 2], np.int32)     # gaps, not monotone, one string twice, one empty
    e = np.array([26, 9, 16, 14, 33, 9], np.int32)
    skips = np.array([0, 1, 0, 0, 1, 0], bool)
    fl = dict(add_dummy_prefix=True, remove_extra_whitespaces=True, escape_whitespaces=True)
    blob_in = np.frombuffer(blob, np.uint8)
    ref3 = CharsMapRef(blob, **fl)(b, e, chars)
    assert ref3[0][0] == 0 and np.array_equal(ref3[0][1:], ref3[1][:-1])
    ref_sk = CharsMapRef(blob, **fl)(b, e, chars, skips)
    assert bytes(ref_sk[2][ref_sk[0][1]:ref_sk[1][1]]) == b"HELLO  "
    data = backend.data([b, e, chars])
    sk = backend.data([skips])[0]
    # 4 inputs, the last one u8: the charsmap; 5 inputs: skips + charsmap; twice with the same handle
    op = CharsMapNormalization(lib=backend.lib, **fl)
    for _ in range(2):
        assert_same(list(ref3), op.evaluate(data + [blob_in]), backend.host, "4 inputs")
    op = CharsMapNormalization(lib=backend.lib, **fl)
    got = op.evaluate(data + [sk, blob_in])
    assert_same(list(ref_sk), got[:3], backend.host, "5 inputs")
    assert len(got) == 4 and np.array_equal(backend.host(got[3]), skips)
    # a named form: 3 inputs, or 4 with skips; the table comes in as charsmap=
    op = CharsMapNormalization(lib=backend.lib, normalization_form="nfkc", case_fold=True, nmt=True, charsmap=blob, **fl)
    assert_same(list(ref3), op.evaluate(data), backend.host, "3 inputs")
    got = op.evaluate(data + [sk])
    assert_same(list(ref_sk), got[:3], backend.host, "4 inputs with skips")
    assert np.array_equal(backend.host(got[3]), skips)
    with pytest.raises(Exception, match="charsmap"):
        CharsMapNormalization(lib=backend.lib, normalization_form="nfkc")
    with pytest.raises(Exception, match="3, 4 or 5"):
        op.evaluate(data[:2])


def test_empty_blob_is_identity_with_repair(backend):
    rows = [b"plain", "ｈｉ ①".encode(), b"a\xffb\xc0\x80", b"  two  "]
    assert _check(backend, b"", rows, what="identity") == [b"plain", "ｈｉ ①".encode(), b"a\xef\xbf\xbdb\xef\xbf\xbd\xef\xbf\xbd", b"  two  "]


# ---------------------------------------------------------------------------------------------- 5. sizes and boundaries
def test_row_sizes_and_tile_boundaries(backend):
    blob = make_blob(SMALL)
    key = b"mnopqrstuvwx"   # 12 bytes -> "#"
    rows = [b"q", b"x" * 63, b"y" * 64, b"z" * 65, ("é" * 40).encode()[:63], ("é" * 40).encode()[:65], b"a" * 63 + "あ".encode() + b"b"]
    rows += [b"." * off + key + b"." * 30 for off in range(50, 71)]               # the key across the 64-byte boundary
    rows += [b" " * off + key + b"  " + key for off in range(250, 262)]          # ... and across the block's 256
    rows += [b"." * off + b"\xe3\x81\x82" * 3 + b"\xe3\x81" for off in range(58, 66)]
    rng = np.random.default_rng(5)
    alphabet = [b"a", b" ", b"ab", b"xy", b"zz", b"q", b"w", key, b"k", "é".encode(), "あ".encode(), b"\xff", b"\xe3\x81", SYMBOL]
    rows.append(b"".join(alphabet[i] for i in rng.integers(0, len(alphabet), 3000))[:8192])
    for fl in (ALL_FLAGS if backend.name != "emu" else [flags_of(0), flags_of(7), flags_of(2)]):
        _check(backend, blob, rows, what="sizes", **fl)


def test_one_megabyte_row(backend):
    blob = make_blob(SMALL)
    rng = np.random.default_rng(6)
    alphabet = [b"hello", b" ", b"  ", b"ab", b"xy", b"mnopqrstuvwx", "é".encode(), "あいう".encode(), b"\xff", SYMBOL, b"k"]
    big = b"".join(alphabet[i] for i in rng.integers(0, len(alphabet), 300000))[:1 << 20]
    assert len(big) == 1 << 20
    _check(backend, blob, [b"front", big, b"back "], what="1 MB", add_dummy_prefix=True, remove_extra_whitespaces=True, escape_whitespaces=True)


# ---------------------------------------------------------------------------------------------- 6. capacity
def test_capacity_and_bound(backend):
    from openvino_tokenizers_amd import _lib as L
    g = golden()
    blob = make_blob(SMALL)
    fl = dict(add_dummy_prefix=True, escape_whitespaces=True, remove_extra_whitespaces=False)
    rows = [b"k" * 100, b"a b c", b"k k"]   # k -> 11 bytes: the ratio-11 key
    b, e, c = O.pack_strings(rows)
    ref = CharsMapRef(blob, **fl)(b, e, c)
    need = len(ref[2])
    op = _op(backend, **fl)
    data = backend.data([b, e, c]) + [np.frombuffer(blob, np.uint8)]
    assert_same(list(ref), op.evaluate(data, chars_capacity=need), backend.host, "exact capacity")
    assert op.bound(len(rows), len(c)) >= need and op.bound(1, 100) >= 1100 + 3
    with pytest.raises(L.OvtkError) as err:
        op.evaluate(data, chars_capacity=need - 1)
    assert err.value.code == L.E_CAPACITY and str(need) in str(err.value)
    # nothing is written behind (or into) a buffer that is too small
    lib = backend.lib
    if backend.name != "hip-device":
        guard = np.full(need + 64, 0xAB, np.uint8)
        ob, oe = np.zeros(3, np.int32), np.zeros(3, np.int32)
        s = L.Strings(b.ctypes.data, e.ctypes.data, c.ctypes.data, 3, len(c))
        out = L.StringsOut(ob.ctypes.data, oe.ctypes.data, guard.ctypes.data, need - 1, 0)
        assert lib.ovtk_charsmap_run(op._h, C.byref(s), None, C.byref(out), L.MEM_HOST, None) == L.E_CAPACITY
        assert out.n_chars == need and np.all(guard == 0xAB)
    # the bound holds on the golden, every blob and flag combination
    strings = g["strings"]
    total_in = sum(map(len, strings))
    for j, name in enumerate(BLOBS):
        for f in (0, 5, 7):
            h = _op(backend, **flags_of(f))
            h.evaluate(backend.data(list(O.pack_strings(strings[:2]))) + [np.frombuffer(g["blobs"][name], np.uint8)])
            assert h.bound(len(strings), total_in) >= int(g["lens"][:, j, f].astype(np.int64).sum())


# ---------------------------------------------------------------------------------------------- 7. malformed blobs
def test_malformed_blobs_are_unsupported(backend):
    from openvino_tokenizers_amd import _lib as L
    good = make_blob(SMALL)
    size = struct.unpack_from("<I", good)[0]
    units = np.frombuffer(good, "<u4", size // 4, 4).copy()
    leaf = int(np.flatnonzero(((units & 0x80000000) != 0) & ((units & 0x7FFFFFFF) != 0))[0])   # (a value unit, not a filler)
    bad_value = units.copy()
    bad_value[leaf] = 0x80000000 | 0x00FFFFFF
    cases = {"size past the end": struct.pack("<I", len(good)) + good[4:], "size not a multiple of 4": struct.pack("<I", size - 2) + good[4:],
             "short": b"\x01\x00", "value outside": good[:4] + bad_value.tobytes() + good[4 + size:], "no NUL": good[:-1]}
    z = O.pack_strings([b"abc"])
    for what, blob in cases.items():
        with pytest.raises(L.OvtkError) as err:
            _op(backend).evaluate(backend.data(list(z)) + [np.frombuffer(blob, np.uint8)])
        assert err.value.code == L.E_UNSUPPORTED, what


# ---------------------------------------------------------------------------------------------- 8. CaseFold, NormalizeUnicode
def test_case_fold_and_normalize_unicode(backend):
    from openvino_tokenizers_amd.ops import CaseFold, NormalizeUnicode
    every = bytes(range(256))
    b, e, c = np.array([0, 256, 100], np.int32), np.array([256, 256, 130], np.int32), np.frombuffer(every, np.uint8)
    for lower in (True, False):
        want = b"".join(case_fold_ascii(every[x:y], lower) for x, y in zip(b, e))
        got = CaseFold(encoding="", lower=lower, lib=backend.lib).evaluate(backend.data([b, e, c]))
        assert_same([np.array([0, 256, 256], np.int32), np.array([256, 256, 286], np.int32), np.frombuffer(want, np.uint8)], got, backend.host, f"CaseFold lower={lower}")
    assert case_fold_ascii(b"aZ[`{@", True) == b"az[`{@" and case_fold_ascii(b"aZ[`{@", False) == b"AZ[`{@"
    g = golden()
    blob = g["blobs"]["nmt_nfkc_cf"]
    strings = g["strings"][:120]
    sb, se, sc = O.pack_strings(strings)
    skips = np.arange(len(strings)) % 5 == 0
    plain = CharsMapRef(blob)(sb, se, sc)
    assert_same(list(plain), CaseFold("utf-8", charsmap=blob, lib=backend.lib).evaluate(backend.data([sb, se, sc])), backend.host, "CaseFold utf-8")
    assert_same(list(plain), NormalizeUnicode("nfkc", charsmap=blob, lib=backend.lib).evaluate(backend.data([sb, se, sc])), backend.host, "NormalizeUnicode")
    got = NormalizeUnicode("nfkc", charsmap=blob, lib=backend.lib).evaluate(backend.data([sb, se, sc, skips]))
    assert_same(list(CharsMapRef(blob)(sb, se, sc, skips)), got[:3], backend.host, "NormalizeUnicode with skips")
    for make in (lambda: CaseFold("utf-8", lib=backend.lib), lambda: NormalizeUnicode("NFC", lib=backend.lib), lambda: CaseFold("utf-8", lower=False, charsmap=blob, lib=backend.lib),
                 lambda: CaseFold("latin-1", lib=backend.lib)):
        with pytest.raises(Exception):
            make()


# ---------------------------------------------------------------------------------------------- 9. pipeline
def test_pipeline_in_front_of_unigram(backend):
    from openvino_tokenizers_amd import pipeline as P
    from openvino_tokenizers_amd.ops import CharsMapNormalization, RegexSplit, UnigramTokenizer
    z = np.load(G / "golden_unigram_small.npz")
    cut = lambda ends, data: [bytes(data[x:y]) for x, y in zip(np.concatenate([[0], ends[:-1]]), ends)]   # noqa: E731
    vocab, scores, unk = cut(z["vocab_ends"], z["vocab_chars"]), z["scores"], int(z["unk_id"])
    g = golden()
    blob = g["blobs"]["nmt_nfkc_cf"]
    strings = [s for s in g["strings"][:400] if s][:60] + [b"  Hello   World  ", "ｈｅｌｌｏ ① ".encode()]
    b, e, c = O.pack_strings(strings)
    rb = np.arange(len(strings), dtype=np.int32)
    fl = dict(add_dummy_prefix=True, remove_extra_whitespaces=True, escape_whitespaces=False)
    steps = [P.CharsmapStep(charsmap=blob, lib=backend.lib, **fl), P.RegexSplitStep(r"\s+", "remove", lib=backend.lib),
             P.UnigramModelStep(vocab, scores, unk_token_id=unk, lib=backend.lib)]
    got = P.Pipeline(steps).run("strings", backend.data([rb, rb + 1, b, e, c]) + [None])
    nb, ne, nc = CharsMapNormalization(lib=backend.lib, **fl).evaluate(backend.data([b, e, c]) + [np.frombuffer(blob, np.uint8)])
    assert_same(list(CharsMapRef(blob, **fl)(b, e, c)), [nb, ne, nc], backend.host, "normalized")
    pieces = RegexSplit("remove", lib=backend.lib).evaluate(backend.data([rb, rb + 1]) + [nb, ne, nc, np.frombuffer(rb"\s+", np.uint8)])
    vb, ve, vc = O.pack_strings(vocab)
    want = UnigramTokenizer(unk_token_id=unk, lib=backend.lib).evaluate(list(pieces[:5]) + [vb, ve, vc, scores])
    assert_same([backend.host(x) for x in want], got, backend.host, "pipeline")
    assert [type(s) for s in P.fuse(steps)] == [type(s) for s in steps]


def test_fuse_leaves_normalizers_in_front_of_bert_chain(backend):
    from openvino_tokenizers_amd import pipeline as P
    from tools.make_tokenizers import load_tokenizer
    tok = load_tokenizer("bert_small")
    consts = list(O.pack_strings(tok["vocab"])) + [np.asarray(tok["unk_id"], np.int32)]
    blob = golden()["blobs"]["nmt_nfkc_cf"]
    strings = [b"Hello, World!  This is BERT.", "ｈｅｌｌｏ ①st café".encode(), b"", b"UPPER lower MiXeD, punct;uation"] + [s for s in golden()["strings"][40:70]]
    b, e, c = O.pack_strings(strings)
    rb = np.arange(len(strings), dtype=np.int32)
    steps = [P.NormalizeUnicode("NFKC", charsmap=blob, lib=backend.lib), P.CaseFoldStep("", lib=backend.lib),
             P.RegexSplitStep(P.BERT_WS, "remove", lib=backend.lib), P.RegexSplitStep(P.BERT_PUNCT, "isolate", lib=backend.lib),
             P.WordPieceTokenizationStep(consts, tok["suffix_indicator"], tok["max_bytes_per_word"], lib=backend.lib)]
    fused = P.fuse(steps)
    assert [type(s).__name__ for s in fused] == ["NormalizeUnicode", "CaseFoldStep", "FusedSplitWordpieceStep"]
    state = backend.data([rb, rb + 1, b, e, c]) + [None]
    want = P.Pipeline(steps).run("strings", state)
    got = P.Pipeline(fused).run("strings", state)
    assert_same([backend.host(x) for x in want], got, backend.host, "fused == unfused")
    assert len(backend.host(got[2])) > len(strings)


# ---------------------------------------------------------------------------------------------- 10. the config-2 batch
@pytest.mark.gpu
def test_config2_batch(gpu_backend):
    """65 536 rows x ~512 bytes as tools/ops_timing.py builds them, 5 % of the characters replaced by ones the map rewrites: the restatement
    on a 1 500-row prefix and on every 64th row; host and device buffers agree on the whole batch."""
    from tests.conftest import Backend
    from tools.workloads import TextModel
    blob = golden()["blobs"]["nmt_nfkc_cf"]
    b, e, c = TextModel(1234, "zipf").batch(65536, 512, seed=1000)
    c = c.copy()
    rng = np.random.default_rng(3)
    c[rng.random(len(c)) < 0.05] = ord("Q")   # (the case-folding map rewrites capitals)
    fl = dict(add_dummy_prefix=True, remove_extra_whitespaces=True, escape_whitespaces=True)
    blob_in = np.frombuffer(blob, np.uint8)
    dev = _op(gpu_backend, **fl).evaluate(gpu_backend.data([b, e, c]) + [blob_in])
    dev = [gpu_backend.host(x) for x in dev]
    host = _op(Backend("hip-host", gpu_backend.lib), **fl).evaluate([b, e, c, blob_in])
    assert_same(dev, host, np.asarray, "host == device")
    ref = CharsMapRef(blob, **fl)
    rows = sorted(set(range(1500)) | set(range(0, 65536, 64)))
    for i in rows:
        assert bytes(dev[2][dev[0][i]:dev[1][i]]) == ref.normalize(bytes(c[b[i]:e[i]])), i
    assert dev[0][0] == 0 and np.array_equal(dev[0][1:], dev[1][:-1]) and dev[1][-1] == len(dev[2])
