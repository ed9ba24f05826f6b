"""BytesToChars, CharsToBytes, ContribStringSplit, ContribStringJoin and RaggedTensorPack against tests/string_ops_ref.py, whole
arrays, no tolerance.  The restatement itself is pinned by tokenizers' ByteLevel, the GPT-2 fixture's vocabulary, bytes.split and
bytes.join; the same pins are asserted on the library."""
import json
from pathlib import Path

import numpy as np
import pytest

from openvino_tokenizers_amd import _lib as L
from openvino_tokenizers_amd import ops as K
from openvino_tokenizers_amd import pipeline as P
from tests import string_ops_ref as R
from tests.util import BpeTok, assert_same
from tools.harness import pack_strings
from tools.make_tokenizers import load_tokenizer
from tools.workloads import ragged_rows

G = Path(__file__).resolve().parent / "golden"
BLOCK = 2048   # bytes a block of the map kernels takes at a time


def _host(backend, outs):
    return [backend.host(x) for x in outs]


def _one_row(n):
    return np.asarray([0], np.int32), np.asarray([n], np.int32)


def b2c(backend, rb, re_, b, e, c, skips=None, **kw):
    ins = backend.data([rb, re_, b, e, c]) + (backend.data([np.asarray(skips, np.uint8)]) if skips is not None else [])
    return _host(backend, K.BytesToChars(lib=backend.lib).evaluate(ins, **kw))


def c2b(backend, rb, re_, b, e, c, **kw):
    return _host(backend, K.CharsToBytes(lib=backend.lib).evaluate(backend.data([rb, re_, b, e, c]), **kw))


def split(backend, b, e, c, delim, skip_empty, **kw):
    ins = backend.data([b, e, c]) + [np.frombuffer(delim, np.uint8), np.asarray([skip_empty], np.uint8)]
    return _host(backend, K.ContribStringSplit(lib=backend.lib).evaluate(ins, **kw))


def join(backend, b, e, c, sep, axis, **kw):
    ins = backend.data([b, e, c]) + [np.frombuffer(sep, np.uint8), np.asarray([axis], np.int64)]
    return _host(backend, K.ContribStringJoin(lib=backend.lib).evaluate(ins, **kw))


def _code(fn):
    with pytest.raises(L.OvtkError) as err:
        fn()
    return err.value.code


def _check_maps(backend, rb, re_, b, e, c, skips=None, what=""):
    """BytesToChars against the restatement, then CharsToBytes of its output (no skips: skipped text need not be in the map)."""
    got = b2c(backend, rb, re_, b, e, c, skips)
    ref = R.bytes_to_chars(rb, re_, b, e, c, skips)
    assert_same([np.asarray(rb), np.asarray(re_)] + list(ref), got[:5], lambda x: x, what + " BytesToChars")
    if skips is None:
        back = c2b(backend, rb, re_, *got[2:5])
        assert_same(list(R.chars_to_bytes(rb, re_, *ref)), back, lambda x: x, what + " CharsToBytes")
        rows = b"".join(R.element(b, e, c, i) for j in range(len(rb)) for i in range(rb[j], re_[j]))
        assert bytes(back[2]) == rows, what + " round trip"
    return got


# ------------------------------------------------------------------------------------------ the restatement's pins
def test_map_is_gpt2_bytes_to_unicode():
    table = R.bytes_to_unicode()
    assert len(set(table.values())) == 256
    assert [b for b in range(256) if ord(table[b]) == b] == list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
    assert [ord(table[b]) for b in range(256) if ord(table[b]) != b] == list(range(256, 256 + 68))
    assert all(len(R.B2C[b]) == (1 if 33 <= b <= 126 else 2) for b in range(256))


def test_restatement_matches_hf_byte_level():
    tokenizers = pytest.importorskip("tokenizers")
    pre = tokenizers.pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)
    assert set(tokenizers.pre_tokenizers.ByteLevel.alphabet()) == set(R.bytes_to_unicode().values())
    dec = tokenizers.decoders.ByteLevel()
    for s in ["Hello, world!", " leading space\tand\ttabs\n", "naïve café — ☃ 日本語 🙂", "".join(chr(k) for k in range(1, 128))]:
        mapped = pre.pre_tokenize_str(s)[0][0]
        assert R.map_bytes(s.encode()).decode() == mapped
        assert R.unmap_bytes(mapped.encode()).decode() == dec.decode([mapped]) == s


def test_library_matches_hf_byte_level(backend):
    tokenizers = pytest.importorskip("tokenizers")
    pre = tokenizers.pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)
    dec = tokenizers.decoders.ByteLevel()
    texts = ["Hello, world!", " leading space\tand\ttabs\n", "naïve café — ☃ 日本語 🙂", "".join(chr(k) for k in range(1, 128))]
    b, e, c = pack_strings(texts)
    rb, re_ = ragged_rows(len(texts))
    got = b2c(backend, rb, re_, b, e, c)
    mapped = [bytes(got[4][x:y]).decode() for x, y in zip(got[2], got[3])]
    assert mapped == [pre.pre_tokenize_str(s)[0][0] for s in texts]
    back = c2b(backend, rb, re_, *got[2:5])
    assert [bytes(back[2][x:y]).decode() for x, y in zip(back[0], back[1])] == [dec.decode([m]) for m in mapped] == texts


def _fixture_vocab():
    vocab = load_tokenizer("gpt2_small")["vocab"]
    hf = json.loads((G / "tok_gpt2_small.hf.json").read_text())["model"]["vocab"]
    keys = sorted(hf, key=hf.get)
    # the npz vocabulary is the bytes form: some entry is no valid text of the map's characters, and mapping gives the keys
    assert any(v != k.encode() for v, k in zip(vocab, keys))
    return vocab[:len(keys)], keys


def test_restatement_matches_fixture_vocabulary():
    vocab, keys = _fixture_vocab()
    assert [R.map_bytes(v).decode() for v in vocab] == keys


def test_library_matches_fixture_vocabulary(backend):
    vocab, keys = _fixture_vocab()
    b, e, c = pack_strings(vocab)
    got = b2c(backend, *_one_row(len(vocab)), b, e, c)
    assert [bytes(got[4][x:y]).decode() for x, y in zip(got[2], got[3])] == keys
    back = c2b(backend, *ragged_rows(len(vocab)), *got[2:5])
    assert [bytes(back[2][x:y]) for x, y in zip(back[0], back[1])] == vocab


def test_restatement_split_and_join_are_python_s():
    for text, d in [(b"aaa", b"aa"), (b"", b","), (b"a,b,,c,", b","), (b"abababab", b"abab"), (b"baab", b"aa"), (b"x", b"xyz"), (b", a, ", b", ")]:
        assert R.split_tokens(text, d) == text.split(d)
    assert b"aaa".split(b"aa") == [b"", b"a"] and b"".split(b",") == [b""]
    assert R.split_tokens(b"abc", b"") == [b"a", b"b", b"c"] and R.split_tokens(b"", b"") == []
    b, e, c = pack_strings([b"a", b"bc", b"", b"d", b"ef", b"g"])
    jb, je, jc = R.string_join(b.reshape(2, 3), e.reshape(2, 3), c, b"-", 1)
    assert [bytes(jc[x:y]) for x, y in zip(jb, je)] == [b"a-bc-", b"d-ef-g"]
    jb, je, jc = R.string_join(b.reshape(2, 3), e.reshape(2, 3), c, b"-", 0)
    assert [bytes(jc[x:y]) for x, y in zip(jb, je)] == [b"a-d", b"bc-ef", b"-g"]


# ------------------------------------------------------------------------------------------ BytesToChars / CharsToBytes
def test_all_byte_values(backend):
    every = bytes(range(256))
    b, e, c = pack_strings([every])
    got = _check_maps(backend, *_one_row(1), b, e, c, what="256 values, one element")
    assert bytes(got[4]) == R.map_bytes(every) and len(got[4]) == 256 + 162
    b, e, c = pack_strings([bytes([k]) for k in range(256)])
    _check_maps(backend, *_one_row(256), b, e, c, what="256 elements")
    _check_maps(backend, *ragged_rows(256), b, e, c, what="256 rows")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 300])
def test_element_counts(backend, n):
    rng = np.random.default_rng(n)
    texts = [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in rng.integers(0, 9, n)]
    b, e, c = pack_strings(texts)
    _check_maps(backend, *ragged_rows(n), b, e, c, what=f"{n} elements, a row each")
    cuts = np.sort(rng.integers(0, n + 1, 5)).astype(np.int32)   # rows of any size, empty ones among them
    rb, re_ = np.concatenate([[0], cuts]).astype(np.int32), np.concatenate([cuts, [n]]).astype(np.int32)
    _check_maps(backend, rb, re_, b, e, c, what=f"{n} elements, six rows")


def test_empty_elements_and_rows(backend):
    texts = [b"", b"", b"ab\x00", b"", b"\xff", b"", b""]
    b, e, c = pack_strings(texts)
    rb = np.asarray([0, 0, 2, 3, 3, 5, 7, 7], np.int32)
    re_ = np.asarray([0, 2, 3, 3, 5, 7, 7, 7], np.int32)
    _check_maps(backend, rb, re_, b, e, c, what="empty in front, between, behind")
    none = np.zeros(0, np.int32)
    got = c2b(backend, np.zeros(3, np.int32), np.zeros(3, np.int32), none, none, np.zeros(0, np.uint8))
    assert_same([np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(0, np.uint8)], got, lambda x: x, "rows without elements")


def test_long_element_and_many_short_ones(backend):
    rng = np.random.default_rng(1)
    b, e, c = pack_strings([bytes(rng.integers(0, 256, 5000, dtype=np.uint8))])
    _check_maps(backend, *_one_row(1), b, e, c, what="5 000 bytes")
    texts = [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in rng.integers(1, 4, 3000)]
    b, e, c = pack_strings(texts)
    cuts = np.arange(0, 3001, 50, dtype=np.int32)
    _check_maps(backend, cuts[:-1], cuts[1:], b, e, c, what="3 000 short elements")
    b, e, c = pack_strings([b"ab", bytes(rng.integers(0, 256, 5000, dtype=np.uint8)), b"\x01"] + texts[:700])
    _check_maps(backend, *_one_row(703), b, e, c, what="long among short")


@pytest.mark.parametrize("lead", [0, 1])
def test_two_byte_characters_across_a_block_edge(backend, lead):
    """An element of wide bytes: its two-byte characters straddle the mapped text's 2 048-byte edges at either parity, and every
    pair of the mapped text straddles an input block edge of CharsToBytes for one of the two."""
    text = b"a" * lead + bytes([0, 200, 127, 255, 173, 32]) * 700
    b, e, c = pack_strings([b"xy", text, b"z"])
    got = _check_maps(backend, *_one_row(3), b, e, c, what=f"lead {lead}")
    assert got[4][BLOCK - 1 - lead] >= 194 or got[4][BLOCK - lead] >= 194   # a lead byte right at an edge, a continuation behind it


def test_uncovered_elements_and_unordered_offsets(backend):
    chars = np.frombuffer(b"\x00zero|one\xff|two two|" + bytes(range(120, 140)), np.uint8).copy()
    b = np.asarray([10, 5, 0, 18, 2, 18, 7], np.int32)   # neither ordered nor gap-free; two elements share text
    e = np.asarray([17, 9, 5, 38, 2, 38, 12], np.int32)
    rb, re_ = np.asarray([1, 4, 4], np.int32), np.asarray([3, 4, 6], np.int32)   # elements 0, 3 and 6: no row
    got = _check_maps(backend, rb, re_, b, e, chars, what="uncovered, unordered")
    assert got[2][0] == got[3][0] == got[2][3] == got[3][3] == got[2][6] == got[3][6] == 0
    b[0], e[0] = -5, 99999   # what no row covers is never read
    _check_maps(backend, rb, re_, b, e, chars, what="uncovered and out of range")


@pytest.mark.parametrize("kind", ["none", "all", "mixed"])
def test_skips(backend, kind):
    rng = np.random.default_rng(5)
    texts = [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in rng.integers(0, 40, 200)] + [bytes(rng.integers(0, 256, 3000, dtype=np.uint8))] * 2
    b, e, c = pack_strings(texts)
    n = len(texts)
    skips = {"none": np.zeros(n, np.uint8), "all": np.ones(n, np.uint8), "mixed": (rng.integers(0, 2, n)).astype(np.uint8)}[kind]
    if kind == "mixed":
        skips[-2:] = [1, 0]
    got = _check_maps(backend, *ragged_rows(n), b, e, c, skips, what=f"skips {kind}")
    assert len(got) == 6 and np.array_equal(got[5], skips)
    for i in np.flatnonzero(skips):   # skipped elements come back as bytes
        assert bytes(got[4][got[2][i]:got[3][i]]) == texts[i]


def test_map_errors(backend):
    b, e, c = pack_strings([b"ab", b"cd", b"ef"])
    two = lambda lo, hi: (np.asarray(lo, np.int32), np.asarray(hi, np.int32))
    for fn in (b2c, c2b):
        assert _code(lambda: fn(backend, *two([0, 1], [2, 3]), b, e, c)) == L.E_UNSUPPORTED          # overlapping rows
        assert _code(lambda: fn(backend, *two([2, 0], [3, 2]), b, e, c)) == L.E_UNSUPPORTED          # rows going backwards
        assert _code(lambda: fn(backend, *two([0], [4]), b, e, c)) == L.E_RANGE                      # a row past the elements
        assert _code(lambda: fn(backend, *two([2], [1]), b, e, c)) == L.E_RANGE                      # row end < begin
        assert _code(lambda: fn(backend, *two([-1], [1]), b, e, c)) == L.E_RANGE
        bad_e = e.copy()
        bad_e[1] = 1
        assert _code(lambda: fn(backend, *two([0], [3]), b, bad_e, c)) == L.E_RANGE                  # element end < begin
        bad_e[1] = 7
        assert _code(lambda: fn(backend, *two([0], [3]), b, bad_e, c)) == L.E_RANGE                  # an offset past the tensor
        bad_b = b.copy()
        bad_b[0] = -1
        assert _code(lambda: fn(backend, *two([0], [3]), bad_b, e, c)) == L.E_RANGE


OUT_OF_DOMAIN = {
    "a lone continuation byte": [b"a\x80b"],
    "a continuation byte first": [b"\xa1"],
    "a lead byte at the end of an element": [b"ab\xc4"],
    "a lead byte followed by ASCII": [b"\xc4a"],
    "the pair 194,128": [bytes([194, 128])],
    "the pair 194,173": [bytes([194, 173])],
    "the pair 197,132": [bytes([197, 132])],
    "byte 192": [b"a\xc0\x80"],
    "byte 198": [b"\xc6\x80"],
    "byte 255": [b"ab\xff"],
    "a pair split across two elements of one row": [b"a\xc4", b"\x80b"],
    "two continuation bytes": [b"\xc4\x80\x80"],
}


@pytest.mark.parametrize("what", list(OUT_OF_DOMAIN))
def test_chars_to_bytes_out_of_domain(backend, what):
    texts = [b"fine \xc4\xa0", b""] + OUT_OF_DOMAIN[what] + [b"\xc3\xbf"]
    b, e, c = pack_strings(texts)
    with pytest.raises(R.OutOfDomain):
        R.chars_to_bytes(*_one_row(len(texts)), b, e, c)
    assert _code(lambda: c2b(backend, *_one_row(len(texts)), b, e, c)) == L.E_RANGE
    # ... and the same text a few blocks into a long row
    b, e, c = pack_strings([b"\xc4\xa0" * 3000] + texts)
    assert _code(lambda: c2b(backend, *_one_row(len(texts) + 1), b, e, c)) == L.E_RANGE


def test_chars_to_bytes_out_of_domain_in_every_block(backend):
    """Malformed bytes all over a text of some fifty blocks: blocks start while others are already reporting."""
    text = (b"\xc4\xa0" * 500 + b"\xff" + b"ok\x80") * 100
    b, e, c = pack_strings([text[:40000], text[40000:]])
    assert _code(lambda: c2b(backend, *_one_row(2), b, e, c)) == L.E_RANGE
    good = b"\xc4\xa0" * 50000   # ... and the workspace the refused call used serves the next one
    b, e, c = pack_strings([good])
    assert bytes(c2b(backend, *_one_row(1), b, e, c)[2]) == b" " * 50000


def test_map_capacity(backend):
    b, e, c = pack_strings([b"ab\x00", b"", b"\xff\x01"])
    ref = R.bytes_to_chars(*_one_row(3), b, e, c)
    need = len(ref[2])
    for fn, ins, want in ((K.BytesToChars, [b, e, c], need), (K.CharsToBytes, list(ref), 5)):
        op = fn(lib=backend.lib)
        data = backend.data(list(_one_row(3)) + ins)
        with pytest.raises(L.OvtkError) as err:
            op.evaluate(data, chars_capacity=want - 1)
        assert err.value.code == L.E_CAPACITY and op.needed_chars == want
        assert len(backend.host(op.evaluate(data, chars_capacity=want)[-1])) == want
    # nothing is written: the raw call, into a buffer of sentinels
    import ctypes as C
    rb, re_ = _one_row(3)
    oc = np.full(need, 0xEE, np.uint8)
    ob, oe = np.full(3, -7, np.int32), np.full(3, -7, np.int32)
    if backend.name == "hip-device":
        import torch
        t = [torch.as_tensor(a, device="cuda") for a in (rb, re_, b, e, c, ob, oe, oc)]
        p = [x.data_ptr() for x in t]
        mem = L.MEM_DEVICE
    else:
        t = [rb, re_, b, e, c, ob, oe, oc]
        p = [x.ctypes.data for x in t]
        mem = L.MEM_HOST
    rs = L.RaggedStrings(p[0], p[1], 1, L.Strings(p[2], p[3], p[4], 3, len(c)))
    out = L.StringsOut(p[5], p[6], p[7], need - 1, 0)
    assert backend.lib.ovtk_bytes_to_chars(C.byref(rs), None, C.byref(out), mem, 0, None) == L.E_CAPACITY
    assert out.n_chars == need
    after = [backend.host(x) for x in t[5:]]
    assert (after[0] == -7).all() and (after[1] == -7).all() and (after[2] == 0xEE).all()


# ------------------------------------------------------------------------------------------ ContribStringSplit
SPLIT_CASES = [
    (b",", [b"a,b", b"", b",", b",,", b",a", b"a,", b"a,,b", b"abc"]),
    (b", ", [b"a, b", b", ", b",", b" ,", b", , ", b"a, ", b""]),
    ("▁".encode(), ["▁a▁b".encode(), "▁".encode(), "▁▁".encode(), b"\xe2\x96", b"ab", "a▁".encode()]),
    (b"aa", [b"aaaaa", b"aaaa", b"baab", b"a", b"aa", b"aaa", b"", b"ab" + b"a" * 131]),
    (b"abab", [b"abababab", b"ababab", b"abab", b"aba", b"xababababy" * 20]),
    (b"longer than any", [b"short", b"", b"longer than an"]),
    (b"same", [b"same", b"samesame", b"sam"]),
    (b"", [b"abc", b"", b"x", b"\x00\xff"]),
]


@pytest.mark.parametrize("skip_empty", [0, 1])
@pytest.mark.parametrize("case", range(len(SPLIT_CASES)))
def test_split_delimiters(backend, case, skip_empty):
    delim, texts = SPLIT_CASES[case]
    b, e, c = pack_strings(texts)
    ref = R.string_split(b, e, c, delim, bool(skip_empty))
    if delim:   # bytes.split is the rule
        kept = [[t for t in x.split(delim) if t or not skip_empty] for x in texts]
        assert [bytes(ref[3][x:y]) for x, y in zip(ref[1], ref[2])] == [t for row in kept for t in row]
        assert ref[4][-1] == max(len(x.split(delim)) for x in texts)
    assert_same(list(ref), split(backend, b, e, c, delim, skip_empty), lambda x: x, f"{delim!r} skip_empty={skip_empty}")


@pytest.mark.parametrize("skip_empty", [0, 1])
def test_split_long_elements(backend, skip_empty):
    rng = np.random.default_rng(2)
    words = [b"w" * int(k) for k in rng.integers(0, 16, 600)]
    long_one = b" ".join(words)[:5000]
    assert 500 <= long_one.count(b" ") <= 700
    for delim, text in [(b" ", long_one), (b", ", b"x" * 63 + b", " + b"y" * 1982 + b", z"), (b"aa", b"a" * 4999), (b"abc", b"ab" + b"abc" * 1500 + b"c")]:
        # (the second: a delimiter across the 64th position and across byte 2 048)
        b, e, c = pack_strings([b"in front", text, b"", text[:100]])
        assert_same(list(R.string_split(b, e, c, delim, bool(skip_empty))), split(backend, b, e, c, delim, skip_empty), lambda x: x, f"long, {delim!r}")


@pytest.mark.parametrize("skip_empty", [0, 1])
@pytest.mark.parametrize("shape", [(), (12,), (3, 4), (2, 3, 2), (2, 0, 3), (0,)])
def test_split_ranks(backend, shape, skip_empty):
    n = int(np.prod(shape, dtype=np.int64))
    texts = [b"a,b", b"", b",,", b"c", b"d,e,f,g", b",x", b"y,", b"zz", b",", b"1,2", b"3", b"4,,5"][:n]
    b, e, c = pack_strings(texts)
    b, e = b.reshape(shape), e.reshape(shape)
    ref = R.string_split(b, e, c, b",", bool(skip_empty))
    got = split(backend, b, e, c, b",", skip_empty)
    assert_same(list(ref), got, lambda x: x, f"shape {shape}")
    assert got[0].shape == (len(got[1]), len(shape) + 1) and list(got[4][:-1]) == list(shape)


def test_split_rank_9_is_unsupported(backend):
    b, e, c = pack_strings([b"a,b"])
    assert _code(lambda: split(backend, b.reshape((1,) * 9), e.reshape((1,) * 9), c, b",", 0)) == L.E_UNSUPPORTED
    assert len(split(backend, b.reshape((1,) * 8), e.reshape((1,) * 8), c, b",", 0)[1]) == 2


def test_split_dense_shape_counts_before_skipping(backend):
    b, e, c = pack_strings([b"a,b", b",,,,", b"c"])   # the longest element: five tokens, all empty
    got = split(backend, b, e, c, b",", 1)
    assert list(got[4]) == [3, 5] and [list(r) for r in got[0]] == [[0, 0], [0, 1], [2, 0]]
    assert_same(list(R.string_split(b, e, c, b",", True)), got, lambda x: x, "dense_shape")
    got = split(backend, *pack_strings([b"", b",", b",,"]), b",", 1)   # N = 0
    assert got[0].shape == (0, 2) and len(got[1]) == len(got[3]) == 0 and list(got[4]) == [3, 3]


def test_split_errors_and_capacity(backend):
    b, e, c = pack_strings([b"a,b", b"cd,"])
    bad = e.copy()
    bad[0] = -1
    assert _code(lambda: split(backend, b, bad, c, b",", 0)) == L.E_RANGE      # end < begin
    bad[0] = 9
    assert _code(lambda: split(backend, b, bad, c, b",", 0)) == L.E_RANGE
    op = K.ContribStringSplit(lib=backend.lib)
    ins = backend.data([b, e, c]) + [np.frombuffer(b",", np.uint8), np.asarray([0], np.uint8)]
    for kw in ({"values_capacity": 3}, {"chars_capacity": 3}):   # one value short, one byte short
        with pytest.raises(L.OvtkError) as err:
            op.evaluate(ins, **kw)
        assert err.value.code == L.E_CAPACITY and (op.needed_values, op.needed_chars) == (4, 4)
    assert len(backend.host(op.evaluate(ins, values_capacity=4, chars_capacity=4)[1])) == 4


# ------------------------------------------------------------------------------------------ ContribStringJoin
JOIN_TEXTS = [bytes([65 + k % 26]) * (k % 5) for k in range(24)]


@pytest.mark.parametrize("sep", [b"", b"-", b"12345"])
@pytest.mark.parametrize("shape", [(0,), (1,), (5,), (4, 6), (6, 1), (1, 5), (2, 3, 4), (2, 0, 3), (0, 4), ()])
def test_join_every_axis(backend, shape, sep):
    n = int(np.prod(shape, dtype=np.int64))
    b, e, c = pack_strings(JOIN_TEXTS[:n])
    b, e = b.reshape(shape), e.reshape(shape)
    for axis in (range(-len(shape), len(shape)) if shape else [0]):
        ref = R.string_join(b, e, c, sep, axis)
        assert_same(list(ref), join(backend, b, e, c, sep, axis), lambda x: x, f"shape {shape} axis {axis} sep {sep!r}")
    if len(shape) == 1 and n:   # sep.join is the rule
        assert bytes(ref[2]) == sep.join(JOIN_TEXTS[:n])


@pytest.mark.parametrize("axis", [0, 1])
def test_join_many_short_and_one_long(backend, axis):
    rng = np.random.default_rng(axis)
    texts = [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(0, 7, 300 * 7)]
    texts[1000] = bytes(rng.integers(0, 256, 5000, dtype=np.uint8))
    b, e, c = pack_strings(texts)
    b, e = b.reshape(300, 7), e.reshape(300, 7)
    assert_same(list(R.string_join(b, e, c, b", ", axis)), join(backend, b, e, c, b", ", axis), lambda x: x, f"300 x 7, axis {axis}")


def test_join_errors(backend):
    b, e, c = pack_strings(JOIN_TEXTS[:6])
    for shape, axis in [((6,), 1), ((6,), -2), ((2, 3), 2), ((2, 3), -3), ((1,), 1)]:
        assert _code(lambda: join(backend, b[:int(np.prod(shape))].reshape(shape), e[:int(np.prod(shape))].reshape(shape), c, b"-", axis)) == L.E_ARG
    bad = e.copy()
    bad[2] = 0
    assert _code(lambda: join(backend, b, bad, c, b"-", 0)) == L.E_RANGE
    op = K.ContribStringJoin(lib=backend.lib)
    ins = backend.data([b, e, c]) + [np.frombuffer(b"-", np.uint8), np.asarray([0])]
    need = len(c) + 5
    with pytest.raises(L.OvtkError) as err:
        op.evaluate(ins, chars_capacity=need - 1)
    assert err.value.code == L.E_CAPACITY and op.needed_chars == need


@pytest.mark.parametrize("delim", [b" ", b", ", b"aa"])
def test_join_of_split_is_the_input(backend, delim):
    rows = [b"one two  three", b"", b" lead", b"trail ", b"a, b, , c", b"aaaaa", b"baab aab", b"x" * 300 + b" " + b"y" * 70]
    b, e, c = pack_strings(rows)
    idx, vb, ve, vc, dense = split(backend, b, e, c, delim, 0)
    # densify: [rows, most tokens]; Join puts a delimiter behind every padding slot, so only full rows are compared
    k = int(dense[1])
    db, de = np.zeros((len(rows), k), np.int32), np.zeros((len(rows), k), np.int32)
    db[idx[:, 0], idx[:, 1]], de[idx[:, 0], idx[:, 1]] = vb, ve
    jb, je, jc = join(backend, db, de, vc, delim, -1)
    counts = np.bincount(idx[:, 0], minlength=len(rows))
    for r, text in enumerate(rows):
        got = bytes(jc[jb[r]:je[r]])
        assert got == text + delim * (k - counts[r]), (r, got)


# ------------------------------------------------------------------------------------------ RaggedTensorPack, the pipeline
def test_ragged_tensor_pack_is_a_copy(backend):
    data = np.arange(17, dtype=np.int32)
    x = backend.data([np.asarray([0, 5], np.int32), np.asarray([5, 17], np.int32), data])
    out = K.RaggedTensorPack(lib=backend.lib).evaluate(x)
    assert len(out) == 1 and np.array_equal(backend.host(out[0]), data)
    ptr = (lambda t: t.data_ptr()) if backend.name == "hip-device" else (lambda a: a.ctypes.data)
    assert ptr(out[0]) != ptr(x[2])


def test_old_style_byte_level_chains(backend):
    """RegexSplit -> BytesToChars -> BPETokenizer and VocabDecoder -> CharsToBytes with the vocabulary in its "chars" form give what
    today's bytes-form chains give."""
    lib = backend.lib
    t = load_tokenizer("gpt2_small")
    hf = json.loads((G / "tok_gpt2_small.hf.json").read_text())["model"]
    keys = sorted(hf["vocab"], key=hf["vocab"].get)
    chars_vocab = [k.encode() for k in keys] + t["vocab"][len(keys):]   # (the added token behind them: not in the model's vocabulary)
    assert chars_vocab[:len(keys)] == [R.map_bytes(v) for v in t["vocab"][:len(keys)]]
    chars_merges = [(R.map_bytes(l), R.map_bytes(r)) for l, r in t["merges"]]
    bytes_tok = BpeTok.load("gpt2_small")
    chars_tok = BpeTok(chars_vocab, chars_merges, t["added"], t["pattern"], **t["attrs"])
    z = np.load(G / "golden_bpe_gpt2_small.npz")
    rb, re_ = ragged_rows(len(z["begins"]))
    state = lambda: backend.data([rb, re_, z["begins"], z["ends"], z["chars"]]) + [None]
    new = P.Pipeline([P.RegexSplitStep(t["pattern"], "isolate", lib=lib), P.BPETokenizationStep(bytes_tok.consts, lib=lib, **bytes_tok.attrs)])
    old = P.Pipeline([P.RegexSplitStep(t["pattern"], "isolate", lib=lib), P.BytesToCharsStep(lib=lib), P.BPETokenizationStep(chars_tok.consts, lib=lib, **chars_tok.attrs)])
    assert [type(s).__name__ for s in old.fused().steps] == ["RegexSplitStep", "BytesToCharsStep", "BPETokenizationStep"]
    ref = _host(backend, new.run("strings", state()))
    assert_same([z["id_begins"], z["id_ends"], z["ids"]], ref, lambda x: x, "bytes-form chain vs the golden ids")
    assert_same(ref, old.run("strings", state()), backend.host, "chars-form chain")

    d = np.load(G / "golden_detok_gpt2_small.npz")
    skip = d["skip_tokens"].tolist()
    new = P.Pipeline([P.VocabDecoderStep(list(pack_strings(t["vocab"])), skip_tokens=skip, lib=lib), P.FuseStep(lib=lib)])
    old = P.Pipeline([P.VocabDecoderStep(list(pack_strings(chars_vocab)), skip_tokens=skip, lib=lib), P.CharsToBytesStep(lib=lib)])
    assert [type(s).__name__ for s in old.fused().steps] == ["VocabDecoderStep", "CharsToBytesStep"]
    fb, fe, fc = _host(backend, new.run("tokens", backend.data([d["ids"]])))
    ob, oe, oc = _host(backend, old.run("tokens", backend.data([d["ids"]])))
    assert [bytes(fc[x:y]) for x, y in zip(fb, fe)] == [bytes(oc[x:y]) for x, y in zip(ob, oe)]
