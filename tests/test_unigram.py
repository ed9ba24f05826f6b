"""UnigramTokenizer (src/unigram_tokenizer.cpp:17-77, :147-224): the kernel against tests/unigram_ref.py, the restatement against
Hugging Face.  Every comparison is of whole begins / ends / ids arrays, no tolerance anywhere."""
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O
from tests.unigram_ref import UnigramRef, char_starts
from tests.util import assert_same

G = Path(__file__).resolve().parent / "golden"


def _op(backend, **attrs):
    from openvino_tokenizers_amd.ops import UnigramTokenizer
    return UnigramTokenizer(lib=backend.lib, **attrs)


def _rows(n):
    rb = np.arange(n, dtype=np.int32)
    return rb, rb + 1


def _check(backend, vocab, scores, strings, rows=None, what="", calls=1, **attrs):
    """The op on `strings` (one per row unless `rows` = (ragged_begins, ragged_ends)) == the restatement; returns the ids per row."""
    scores = np.asarray(scores, np.float32)
    b, e, c = O.pack_strings(strings)
    rb, re_ = rows if rows is not None else _rows(len(strings))
    ref = UnigramRef(vocab, scores, **attrs)(rb, re_, b, e, c)
    vb, ve, vc = O.pack_strings(vocab)
    op = _op(backend, **attrs)
    for call in range(calls):
        got = op.evaluate(backend.data([rb, re_, b, e, c]) + [vb, ve, vc, scores])
        assert_same(list(ref), got, backend.host, f"{what} call {call}")
    return [ref[2][x:y].tolist() for x, y in zip(ref[0], ref[1])]


# ---------------------------------------------------------------------------------------------- 1. the restatement against Hugging Face
def _golden():
    z = np.load(G / "golden_unigram_small.npz")
    cut = lambda ends, data: [bytes(data[x:y]) for x, y in zip(np.concatenate([[0], ends[:-1]]), ends)]   # noqa: E731
    vocab, strings = cut(z["vocab_ends"], z["vocab_chars"]), cut(z["ends"], z["chars"])
    ids = [z["ids"][x:y].tolist() for x, y in zip(np.concatenate([[0], z["id_ends"][:-1]]), z["id_ends"])]
    return vocab, z["scores"], int(z["unk_id"]), strings, ids


def test_restatement_matches_hf():
    """tests/gen_golden_unigram.py: tokenizers.models.Unigram on a generated vocabulary, scores multiples of 1/64 in (-32, 0], strings of at
    most 512 bytes: every sum is exact in float32 and in HF's float64.  Passes without the op: it pins the yardstick."""
    vocab, scores, unk, strings, ids = _golden()
    assert len(strings) == 3000 and max(map(len, strings)) <= 512
    assert np.all(scores * 64 == np.round(scores * 64)) and scores.min() > -32 and scores.max() <= 0
    ref = UnigramRef(vocab, scores, unk)
    assert [ref.tokenize(s) for s in strings] == ids
    assert sum(unk in r for r in ids) * 4 >= len(ids)


def test_kernel_matches_hf_golden(backend):
    vocab, scores, unk, strings, ids = _golden()
    if backend.name == "emu":
        strings, ids = strings[:150], ids[:150]
    assert _check(backend, vocab, scores, strings, what="golden", unk_token_id=unk) == ids


# ---------------------------------------------------------------------------------------------- 2. where float32 matters
def _decimal_case(n_strings):
    rng = np.random.default_rng(11)
    vocab = [bytes([x]) for x in b"abcd"]
    seen = set(vocab)
    while len(vocab) < 120:
        w = bytes(rng.choice(list(b"abcd"), size=int(rng.integers(2, 6))).tolist())
        if w not in seen:
            seen.add(w)
            vocab.append(w)
    scores = (-0.1 * rng.integers(1, 60, len(vocab))).astype(np.float32)
    strings = [bytes(rng.choice(list(b"abcd"), size=int(rng.integers(8, 60))).tolist()) for _ in range(n_strings)]
    return vocab, scores, strings


def test_float32_sums_decide(backend):
    """Scores -0.1 * k: decimal ties that float32 and float64 round differently.  At least 20 of the strings must tokenize differently
    under float64 accumulation (so the case cannot go soft); the kernel equals the float32 result on all of them."""
    vocab, scores, strings = _decimal_case(2000)
    f32, f64 = UnigramRef(vocab, scores, 0), UnigramRef(vocab, scores, 0, acc=np.float64)
    differ = [s for s in strings if f32.tokenize(s) != f64.tokenize(s)]
    print(f"{len(differ)} of {len(strings)} strings differ between float32 and float64 accumulation")
    assert len(differ) >= 20
    if backend.name == "emu":
        strings = differ + strings[:100]
    _check(backend, vocab, scores, strings, what="float32 ties", unk_token_id=0)


# ---------------------------------------------------------------------------------------------- 3. the rules one by one
def test_equal_sums_earliest_start(backend):
    # "ab" + "c" and "a" + "bc" both sum to -3 (exact): node 3 is reached first from start 0?  No: start 0 reaches nodes 1 and 2, start 1
    # reaches node 3 with a + bc = -3, start 2 offers ab + c = -3, not strictly greater: a, bc stays.
    vocab, scores = [b"a", b"b", b"c", b"ab", b"bc"], [-1.0, -5.0, -1.0, -2.0, -2.0]
    assert _check(backend, vocab, scores, [b"abc"], what="ties", unk_token_id=9) == [[0, 4]]
    # ... and with the whole string a token of the same sum: start 0 gets there first, length 3 after lengths 1 and 2
    vocab, scores = vocab + [b"abc"], scores + [-3.0]
    assert _check(backend, vocab, scores, [b"abc"], what="ties", unk_token_id=9) == [[5]]


def test_token_ending_inside_a_character(backend):
    # E4 B8 AD is one character; the token E4 B8 ends inside it and is a candidate for node 2, but position 2 starts no token: the only way to
    # node 3 is the whole character (a token) -- the cheap half-character is never continued from.
    vocab, scores = [b"\xe4\xb8", b"\xad", b"\xe4\xb8\xad", b"a"], [-0.5, -0.5, -9.0, -1.0]
    assert _check(backend, vocab, scores, [b"\xe4\xb8\xada", b"a\xe4\xb8\xad"], what="inside", unk_token_id=7) == [[2, 3], [3, 2]]


def test_characters_by_lead_nibble_alone(backend):
    vocab, scores = [b"a", b"b", b"ab", b"\xe4ab", b"\x80", b"\xe4"], [-1.0, -1.0, -1.5, -4.0, -2.0, -0.25]
    unk = 77
    assert char_starts(b"\xe4ab") == [0] and char_starts(b"ab\xe4") == [0, 1, 2] and char_starts(b"\x80\x80a") == [0, 1, 2]
    got = _check(backend, vocab, scores, [b"\xe4ab",        # ONE three-byte character, and a token: no unknown edge
                                          b"\xe4ba",        # one character, no token of length 3 (E4 alone ends inside it): unknown
                                          b"ab\xe4",        # a lead byte cut off by the string's end: a one-byte character, a token
                                          b"a\xf0b",        # F0 b: cut to two bytes, unknown
                                          b"\x80\x80a",     # stray continuation bytes: characters of one byte
                                          b"\xbfa"],        # ... one that is no token
                 what="lead nibble", unk_token_id=unk)
    assert got == [[3], [unk], [2, 5], [0, unk], [4, 4, 0], [unk, 0]]


def test_a_character_that_is_a_token_gets_no_unknown_edge(backend):
    # (the unknown edge, min - 10, is below every token's score by construction: what can be seen is that the character's own token is taken
    # and the unknown id appears only for the character that is none)
    vocab, scores = [b"x", b"y", b"<unk>"], [-30.0, -30.0, 0.0]
    assert _check(backend, vocab, scores, [b"xy", b"xzy"], what="no unk edge", unk_token_id=2) == [[0, 1], [0, 2, 1]]


def test_runs_of_unknowns_collapse(backend):
    vocab, scores = [b"a", b"<unk>", b"b"], [-1.0, -1.0, -2.0]
    # ... also across a real token whose position is unk_token_id: with unk_token_id = 2, "b" itself counts as unknown on the way back
    assert _check(backend, vocab, scores, [b"zzz", b"azza", b"zaz", b"az"], what="runs", unk_token_id=1) == [[1], [0, 1, 0], [1, 0, 1], [0, 1]]
    assert _check(backend, vocab, scores, [b"zbz", b"bb", b"abba", b"zab"], what="runs", unk_token_id=2) == [[2], [2], [0, 2, 0], [2, 0, 2]]
    # unk_token_id = -1: back-tracking starts with "previous id = -1", so unknowns at a string's END are dropped too
    assert _check(backend, vocab, scores, [b"zzz", b"azza"], what="runs", unk_token_id=-1) == [[], [0, -1, 0]]


@pytest.mark.parametrize("fuse_unk", [False, True])
@pytest.mark.parametrize("byte_fallback", [False, True])
def test_fuse_unk_and_byte_fallback_change_nothing(backend, fuse_unk, byte_fallback):
    vocab, scores = [b"a", b"<unk>", b"b", b"<0x7A>"], [-1.0, -1.0, -2.0, -3.0]
    got = _check(backend, vocab, scores, [b"zzz", b"azzb"], what="flags", unk_token_id=1, fuse_unk=fuse_unk, byte_fallback=byte_fallback)
    assert got == [[1], [0, 1, 2]]


def test_unk_score_from_the_minimum_given(backend):
    """unk_score = float32(float64(min) - 10.0).  tests/gen_golden_unigram.py::unk_score_search looked for a float32 minimum where that
    and float32(min) - float32(10) differ: none exists (2 000 000 random bit patterns and the neighbourhoods of every half-ulp boundary:
    0 found; a float32 subtraction is already one rounding of the exact difference, and the float64 difference is exact whenever the
    float32 rounding could see its low bits).  So the rule is checked where it decides a path: min = -2.5 -> unknown = -12.5 exactly."""
    from tests.gen_golden_unigram import unk_score_search
    assert len(unk_score_search(200_000)) == 0
    # "ab": a + unknown(b) = p - 12.5 against the token "ab" at the minimum itself, -2.5: the unknown path wins from p = 10 on, strictly above
    for p, want in ((10.5, [0, 9]), (10.0, [1]), (9.0, [1])):
        assert _check(backend, [b"a", b"ab"], [p, -2.5], [b"ab"], what="unk score", unk_token_id=9) == [want]
    # the minimum is the smallest score GIVEN, also that of an entry that can never match (an empty string): unknown = -110, a + unknown = -90
    # loses to "ab" at -50 (from the matching entries alone it would be -60, and 20 - 60 would win)
    assert _check(backend, [b"a", b"", b"ab"], [20.0, -100.0, -50.0], [b"ab"], what="unk score", unk_token_id=9) == [[2]]


def test_duplicate_and_empty_vocabulary_strings(backend):
    vocab, scores = [b"a", b"b", b"a", b"", b"b"], [-5.0, -1.0, -1.0, 0.0, -0.5]
    # this library's choices: the lowest id answers (with ITS score); the empty string never matches
    assert _check(backend, vocab, scores, [b"ab", b""], what="duplicates", unk_token_id=8) == [[0, 1], []]


def test_row_shapes(backend):
    rng = np.random.default_rng(5)
    vocab, scores, strings = _decimal_case(40)
    strings[3] = b""
    # rows of 0-3 strings, an empty row at the end
    cuts = np.unique(np.concatenate([[0, len(strings)], rng.integers(0, len(strings), 25)])).astype(np.int32)
    rb = np.concatenate([cuts[:-1], [5], [0]]).astype(np.int32)
    re_ = np.concatenate([cuts[1:], [5], [0]]).astype(np.int32)
    _check(backend, vocab, scores, strings, rows=(rb, re_), what="row shapes", unk_token_id=0)
    _check(backend, vocab, scores, [b""], what="one empty string", unk_token_id=0)


def test_rows_that_share_strings(backend):
    """Rows may name the same strings again, and strings may overlap in the chars tensor: the nodes of all strings then outnumber the
    first workspace (chars + strings) and the call is run again with what the scan asked for; twice on the same handle."""
    vocab, scores, strings = _decimal_case(30)
    vocab += [s[:20] for s in strings]          # long tokens: few ids, so that rows naming every string fit the reference's output size
    scores = np.concatenate([scores, np.full(len(strings), -0.5, np.float32)])
    b, e, c = O.pack_strings(strings)
    n = len(strings)
    b = np.concatenate([b, np.zeros(2, np.int32), b[:10]]).astype(np.int32)      # two strings that are the WHOLE chars tensor, ten once more
    e = np.concatenate([e, np.full(2, len(c), np.int32), e[:10]]).astype(np.int32)
    rb = np.array([0, n, n + 2, 3, n + 1], np.int32)
    re_ = np.array([n, n + 2, n + 12, 4, n + 2], np.int32)
    ref = UnigramRef(vocab, scores, 0)(rb, re_, b, e, c)
    assert int((e - b).sum()) + len(b) > len(c) + len(b) + 1 and len(ref[2]) <= len(c)
    vb, ve, vc = O.pack_strings(vocab)
    op = _op(backend, unk_token_id=0)
    for call in range(2):
        got = op.evaluate(backend.data([rb, re_, b, e, c]) + [vb, ve, vc, scores])
        assert_same(list(ref), got, backend.host, f"shared strings, call {call}")


def test_long_string_and_full_edge_lists(backend):
    """A string of 5 000 bytes (the lane-per-string relaxation walks it start by start), and starts with more matching tokens than the
    fixed edge list of seven holds -- the chain a, aa, aaa, ... up to the longest token: the left-over path must give the same ids."""
    rng = np.random.default_rng(6)
    vocab = [b"a", b"b"] + [b"a" * k for k in range(2, 25)] + [b"ab", b"ba", b"bab"]
    scores = (-rng.integers(1, 200, len(vocab)) / 16).astype(np.float32)
    long_one = bytes(rng.choice(list(b"aaab"), size=5000).tolist())
    strings = [long_one, b"a" * 7, b"a" * 8, b"a" * 9, b"a" * 24, b"a" * 25, b"a" * 100, b"b" + b"a" * 30 + b"b", b"abab", b"a" * 6 + b"z" + b"a" * 10]
    _check(backend, vocab, scores, strings, what="left-over path", unk_token_id=1)
    # eight tokens at one start, seven at another: exactly one over, exactly full
    vocab = [b"a" * k for k in range(1, 9)] + [b"b" * k for k in range(1, 8)]
    scores = (-rng.integers(1, 200, len(vocab)) / 16).astype(np.float32)
    _check(backend, vocab, scores, [b"a" * 8, b"b" * 7, b"b" * 9, b"a" * 7 + b"b" * 7, b"a" * 20], what="list of seven", unk_token_id=0)


def test_errors(backend):
    from openvino_tokenizers_amd import _lib as L
    vb, ve, vc = O.pack_strings([b"a", b"ab"])
    b, e, c = O.pack_strings([b"abz"])
    one = np.array([0], np.int32)
    sc = np.array([-1.0, -2.0], np.float32)
    with pytest.raises(L.OvtkError, match="Vocab size must be equal to vocab_probs size"):
        _op(backend).evaluate([one, one + 1, b, e, c, vb, ve, vc, sc[:1]])
    with pytest.raises(L.OvtkError) as ei:   # a row that names a string outside the chars tensor
        _op(backend).evaluate([one, one + 1, b, np.array([9], np.int32), c, vb, ve, vc, sc])
    assert ei.value.code == L.E_RANGE
    # ... a string with such offsets that no row names is never read
    got = _op(backend, unk_token_id=5).evaluate([one, one + 1, np.array([0, 0], np.int32), np.array([3, 9], np.int32), c, vb, ve, vc, sc])
    assert backend.host(got[2]).tolist() == [1, 5]
    long_vocab = O.pack_strings([b"a" * 1024])
    with pytest.raises(L.OvtkError) as ei:
        _op(backend).evaluate([one, one + 1, b, e, c, *long_vocab, sc[:1]])
    assert ei.value.code == L.E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- 4. size
@pytest.mark.gpu
def test_size(hip_lib):
    """20 000 random strings per call, a second call on the same handle; host and device buffers."""
    from tests.conftest import Backend
    rng = np.random.default_rng(2)
    alphabet = list(b"abcdeft \n") + [0xE4, 0xB8, 0xAD, 0xE6, 0x96, 0x87]
    vocab = [bytes([x]) for x in b"abcdeft \n"] + [b"\xe4\xb8\xad", b"\xe6\x96\x87"]
    seen = set(vocab)
    while len(vocab) < 3000:
        w = bytes(rng.choice(alphabet, size=int(rng.integers(2, 9))).tolist())
        if w not in seen:
            seen.add(w)
            vocab.append(w)
    scores = (-rng.random(len(vocab)) * 12).astype(np.float32)
    strings = [bytes(rng.choice(alphabet + list(b"xyz\x00\xff"), size=int(rng.integers(0, 90))).tolist()) for _ in range(20000)]
    b, e, c = O.pack_strings(strings)
    cuts = np.unique(np.concatenate([[0, len(strings)], rng.integers(0, len(strings), len(strings) // 2)])).astype(np.int32)
    rb, re_ = cuts[:-1], cuts[1:]
    vb, ve, vc = O.pack_strings(vocab)
    k = int(np.searchsorted(re_, 1500))   # the rows of the first ~1 500 strings
    ref = UnigramRef(vocab, scores, 4)(rb[:k], re_[:k], b, e, c)
    results = []
    for name in ("hip-host", "hip-device"):
        be = Backend(name, hip_lib)
        op = _op(be, unk_token_id=4)
        for call in range(2):
            got = [be.host(x) for x in op.evaluate(be.data([rb, re_, b, e, c]) + [vb, ve, vc, scores])]
            assert np.array_equal(got[0][:k], ref[0]) and np.array_equal(got[1][:k], ref[1]), f"{name} call {call}: offsets"
            assert np.array_equal(got[2][:len(ref[2])], ref[2]), f"{name} call {call}: ids of the prefix"
            results.append(got)
    for got in results[1:]:
        assert_same(results[0], got, Backend.host, "calls and memory spaces agree")


# ---------------------------------------------------------------------------------------------- 5. the pipeline
def test_pipeline_step_by_step_equals_fused(backend):
    from openvino_tokenizers_amd import pipeline as P
    vocab, scores, strings = _decimal_case(24)
    texts = [b" ".join(strings[i:i + 3]) for i in range(0, 24, 3)] + [b"", b"  ", b"abz dab"]
    b, e, c = O.pack_strings(texts)
    rb, re_ = _rows(len(texts))
    lib = backend.lib
    steps = [P.RegexSplitStep(r"\s+", "remove", lib=lib), P.UnigramModelStep(vocab, scores, unk_token_id=0, lib=lib), P.TruncationStep(12, lib=lib),
             P.CombineSegmentsStep([1], [2], lib=lib), P.PaddingStep(pad_value=0, lib=lib)]
    pipe = P.Pipeline(steps)
    fused = pipe.fused()
    assert [type(s) for s in fused.steps] == [P.RegexSplitStep, P.UnigramModelStep, P.FusedEncodeTailStep] and fused.steps[1] is steps[1]
    state = backend.data([rb, re_, b, e, c]) + [None]
    plain, quick = pipe.run("strings", state), fused.run("strings", state)
    assert_same([backend.host(x) for x in plain], quick, backend.host, "pipeline")
    # the ids in front of the tail are the restatement's, row by row
    words = [t.split() for t in texts]
    ref = UnigramRef(vocab, scores, 0)
    dense = backend.host(plain[0])
    for row, ws in zip(dense, words):
        want = ([1] + [i for w in ws for i in ref.tokenize(w)][:12] + [2])
        assert row[:len(want)].tolist() == want and not row[len(want):].any()
    with pytest.raises(ValueError, match="skips"):
        steps[1].apply("strings", state[:5] + [np.zeros(len(texts), np.uint8)])
