"""Every op with its buffers at odd addresses between guard bands (tests/placement.py).

The parity tests hand the kernels torch / numpy allocations: 512-byte aligned, with slack behind them.  Here every data buffer of a
call -- inputs and outputs -- is a region of one arena, `shift` bytes past a 16-byte boundary, exactly as large as asked for, with
4096 bytes of a known `fill` on both sides.  For every case and placement:
  a. every output is bit-identical to the expected value (dtype, shape, bytes) -- the oracle's or the plain-Python reference's of
     the op's own test file, never an aligned run of the library;
  b. the guard bytes and the placed inputs are untouched (Arena.check);
  c. (a) holds under a NUL, an invalid byte, a space and a UTF-8 lead as the neighbours, so the result does not depend on them.
"""
import ctypes as C
import inspect
from functools import lru_cache

import numpy as np
import pytest

from openvino_tokenizers_amd import _lib as L
from openvino_tokenizers_amd import ops as K
from oracle import oracle as O
from tests.placement import GUARD, Arena
from tests.util import BpeTok, one_string_per_row, pack_strings

PLACEMENTS = [(1, 0x00), (2, 0xFF), (3, 0x20), (4, 0xE2), (7, 0xFF), (8, 0x20), (12, 0x00), (15, 0xE2)]
EMU_PLACEMENTS = [(3, 0x20), (12, 0x00), (15, 0xE2)]   # (the emulator runs every lane on one CPU thread)

CASES = {}    # name -> Case
EXEMPT = {}   # class name -> why no case can exist: its evaluate takes no data buffer in the call's memory space


class Case:
    def __init__(self, fn, name, ops, backends, min_align, size):
        self.fn, self.name, self.ops, self.backends, self.min_align, self.size = fn, name, tuple(ops), backends, min_align, size


def case(name, ops, backends=("emu", "hip-host", "hip-device"), min_align=None, size=2 << 20):
    """Registers `fn(run)`: it places its data inputs (run.place), runs the op(s) and hands every result to run.same()."""
    def register(fn):
        assert name not in CASES
        CASES[name] = Case(fn, name, ops, backends, min_align, size)
        return fn
    return register


class Run:
    def __init__(self, backend, arena, shift, monkeypatch):
        self.backend, self.lib, self.arena, self.shift, self.monkeypatch = backend, backend.lib, arena, shift, monkeypatch
        self.compared = 0

    def place(self, *arrays, min_align=None):
        out = [self.arena.place(a, self.shift, min_align) for a in arrays]
        return out if len(out) != 1 else out[0]

    def carve(self, n, kind, min_align=None):
        return self.arena.carve(n, kind, self.shift, min_align)

    def same(self, what, got, want):
        assert len(got) == len(want), f"{what}: {len(got)} outputs, expected {len(want)}"
        for i, (g, w) in enumerate(zip(got, want)):
            g, w = self.backend.host(g), np.asarray(w)
            assert g.dtype == w.dtype, f"{what} output {i}: dtype {g.dtype}, expected {w.dtype}"
            assert g.shape == w.shape, f"{what} output {i}: shape {g.shape}, expected {w.shape}"
            if g.tobytes() != w.tobytes():
                gf, wf = g.reshape(-1), w.reshape(-1)
                bad = int(np.flatnonzero(gf != wf)[0])
                raise AssertionError(f"{what} output {i}: first difference at {bad}: got {gf[bad:bad + 8]}, expected {wf[bad:bad + 8]}")
            self.compared += 1


def _params():
    out = []
    for name, c in CASES.items():
        for b in c.backends:
            for shift, fill in (EMU_PLACEMENTS if b == "emu" else PLACEMENTS):
                marks = [pytest.mark.gpu] if b != "emu" else []
                out.append(pytest.param(b, name, shift, fill, marks=marks, id=f"{name}-{b}-{shift}-{fill:02X}"))
    return out


def u8(s):
    return np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), np.uint8)


def i32(x):
    return np.ascontiguousarray(x, np.int32)


# ================================================================================================ decode writes
@lru_cache(maxsize=None)
def decode_ref(B, S):
    """The inputs and the oracle chain of tests/test_ops_parity.py::test_vocab_decoder_chain."""
    from tests.test_ops_parity import detok_vocab
    vocab, n_base = detok_vocab()
    V = len(vocab)
    ids = np.random.default_rng(B * 1000 + S).integers(0, V, (B, S)).astype(np.int32)
    ids[0, 0], ids[-1, -1], ids[B // 2, S // 2] = -5, V + 3, n_base
    skips = [3, 17, n_base + 2, V + 100, -1]
    dec = O.vocab_decoder(ids, vocab, skips)
    bf = O.byte_fallback(*dec[2:5])
    return dict(ids=ids, skips=skips, vconst=list(pack_strings(vocab)), dec=list(dec), bf=list(bf),
                fuzed=list(O.fuze(dec[0], dec[1], bf[0], bf[1])), plain=list(O.fuze(dec[0], dec[1], dec[2], dec[3])))


for _B, _S in ((7, 33), (3, 2050)):
    def _decode_cases(B=_B, S=_S):
        tag = f"{B}x{S}"

        @case(f"VocabDecoder-{tag}", ["VocabDecoder"])
        def _(run):
            r = decode_ref(B, S)
            got = K.VocabDecoder(skip_tokens=r["skips"], lib=run.lib).evaluate([run.place(r["ids"])] + r["vconst"])
            run.same("VocabDecoder", got, r["dec"])

        @case(f"ByteFallback-{tag}", ["ByteFallback"])
        def _(run):
            r = decode_ref(B, S)
            run.same("ByteFallback", K.ByteFallback(lib=run.lib).evaluate(run.place(*r["dec"][2:5])), r["bf"])

        @case(f"FuzeRagged-{tag}", ["FuzeRagged"])
        def _(run):
            r = decode_ref(B, S)
            got = K.FuzeRagged(lib=run.lib).evaluate(run.place(r["dec"][0], r["dec"][1], r["bf"][0], r["bf"][1]))
            run.same("FuzeRagged", got, r["fuzed"])

        @case(f"FusedDetokenizer-{tag}", ["FusedDetokenizer"])
        def _(run):
            r = decode_ref(B, S)
            dec = K.VocabDecoder(skip_tokens=r["skips"], lib=run.lib)
            inputs = [run.place(r["ids"])] + r["vconst"]
            run.same("with byte fallback", K.FusedDetokenizer(dec, byte_fallback=True).evaluate(inputs), r["fuzed"] + [r["bf"][2]])
            run.same("without", K.FusedDetokenizer(dec, byte_fallback=False).evaluate(inputs), r["plain"] + [r["dec"][4]])
    _decode_cases()


@lru_cache(maxsize=None)
def sp_detok_ref(kind, which):
    from tests import test_sp_detokenizer as T
    ids = np.ascontiguousarray(T.Z[f"bytes_{which}_ids"], np.int32)
    want = T.cut(T.Z[f"bytes_{which}_{T.OPS[kind]}_ends"], T.Z[f"bytes_{which}_{T.OPS[kind]}_chars"])
    lens = np.array([len(w) for w in want], np.int64)
    ends = np.cumsum(lens).astype(np.int32)
    return T.model("bytes"), ids, [(ends - lens).astype(np.int32), ends, np.frombuffer(b"".join(want), np.uint8)]


for _kind, _cls in (("decode", "SentencepieceDetokenizer"), ("stream", "SentencepieceStreamDetokenizer")):
    for _which in ("mix3", "mix5"):   # ids of shape (5, 65) and (2, 1030)
        @case(f"{_cls}-{_which}", [_cls])
        def _(run, kind=_kind, cls=_cls, which=_which):
            mdl, ids, want = sp_detok_ref(kind, which)
            run.same(cls, getattr(K, cls)(lib=run.lib).evaluate([mdl, run.place(ids)]), want)


# ================================================================================================ NumericToString
for _name in ("float64", "float32", "int64", "uint8", "bool"):
    @case(f"NumericToString-{_name}", ["NumericToString"])
    def _(run, name=_name):
        from tests.test_numeric_to_string import expected, golden
        arr, texts = golden(name)
        arr, texts = arr[:130], texts[:130]   # two full waves and a partial one
        x = run.place(arr, min_align=arr.dtype.itemsize)
        if name == "bool":
            x = x.view(run.arena.torch.bool if run.arena.device else np.bool_)
        run.same(name, K.NumericToString(lib=run.lib).evaluate([x]), list(expected(texts)))


# ================================================================================================ RaggedToDense
@lru_cache(maxsize=None)
def dense_inputs(dtype):
    """The inputs of tests/test_ops_parity.py::test_ragged_to_dense_shapes with inner == ()."""
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 40, 50)
    lens[3] = 0
    ends = np.cumsum(lens).astype(np.int32)
    return (ends - lens).astype(np.int32), ends, rng.integers(0, 120, int(lens.sum())).astype(dtype), int(lens.max())


for _dtype in ("int32", "uint8", "int64"):
    @case(f"RaggedToDense-{_dtype}", ["RaggedToDense"])
    def _(run, dtype=_dtype):
        """The C entry point with `dense` and `mask` carved (ops.py allocates the two itself).  int32: `dense` at 4, 8 and 12 modulo 16
        and `mask` at 1, 2 and 3 modulo 4 are the placements that take ragged_to_dense_kernel, not its flat4 form."""
        begins, ends, data, longest = dense_inputs(dtype)
        b, e, d = run.place(begins, ends, data)
        dflt = np.asarray([9], data.dtype)
        for pad_right in (True, False):
            for target in (longest, 7, 64):
                ref = O.ragged_to_dense(begins, ends, data, target, 9, pad_right=pad_right)
                dense, mask = run.carve(50 * target, data.dtype), run.carve(50 * target, "u8")
                rc = run.lib.ovtk_ragged_to_dense(Arena.pointer(b), Arena.pointer(e), C.c_int64(50), Arena.pointer(d), C.c_int64(len(data)),
                                                  data.dtype.itemsize, C.c_int64(1), C.c_int32(target), C.c_void_p(dflt.ctypes.data), int(pad_right), 0,
                                                  Arena.pointer(dense), Arena.pointer(mask), run.arena.mem_kind, 0, run.arena.stream)
                L.check(run.lib, rc)
                run.same(f"target {target} pad_right {pad_right}", [dense.reshape(50, target), mask.reshape(50, target)],
                         [ref[0], np.asarray(ref[1]).astype(np.uint8)])


# ================================================================================================ encodes
def _small_strings():
    """The strings of tests/test_bpe_parity.py::test_unaligned_chars_tensor and one 2100-byte row; strings touch both ends of chars."""
    long_row = ("it's a long row, isn't it?  1234 tabs\tand\nline breaks we'll see " * 40)[:2100]
    return ["it's", "a b", "x" * 700 + " y's", "", long_row, "tail isn't"]


@lru_cache(maxsize=None)
def text_inputs(size, specials=False):
    """ragged_begins, ragged_ends, begins, ends, chars: "small", or "large" = the 320 rows that take the span kernel."""
    if size == "small":
        strings = [s.encode() for s in _small_strings()]
        if specials:
            strings = [strings[0] + b"<|endoftext|>", b"<|endoftext|>" + strings[1]] + strings[2:5] + [b"tail<|endoftext|>isn't"]
    else:
        from tests.test_special_tokens import _texts_with_specials
        strings = _texts_with_specials(np.random.default_rng(320), 320)
        if not specials:
            strings = [s.replace(b"<|endoftext|>", b"") for s in strings]
    return tuple(one_string_per_row(strings))


LLAMA3_FAMILY = "qwen2"   # (tests/test_regex_general.py::test_llama3_family_fused: runs on the Llama-3 scanners)
COMPILED = "clip"          # (a pattern without a hand-written scanner: the compiled DFA)


@lru_cache(maxsize=None)
def encode_ref(which, size):
    from tests.test_regex_general import MODEL_PATTERNS
    inputs = text_inputs(size)
    if which == "gpt2":
        tok = BpeTok.load("gpt2_small")
        pattern = tok.pattern
    else:
        tok = BpeTok.load("llama3_small")
        pattern = MODEL_PATTERNS[LLAMA3_FAMILY]
    pieces = O.RegexSplit(pattern, "isolate")(*inputs)
    return tok, pattern, [np.asarray(x) for x in pieces[:5]], list(tok.oracle()(*pieces[:5]))


def _twice(run, what, call, want):
    for state in ("memo cold", "memo warm"):
        run.same(f"{what}, {state}", call(), want)


for _size in ("small", "large"):
    for _which in ("gpt2", "llama3-family"):
        @case(f"FusedSplitBPE-{_which}-{_size}", ["FusedSplitBPE"], size=4 << 20)
        def _(run, which=_which, size=_size):
            tok, pattern, _, want = encode_ref(which, size)
            data = run.place(*text_inputs(size))
            fused = K.FusedSplitBPE(K.RegexSplit("isolate", lib=run.lib), K.BPETokenizer(**tok.attrs, lib=run.lib))
            _twice(run, which, lambda: fused.evaluate(data + [u8(pattern)], tok.consts), want)

    @case(f"BPETokenizer-{_size}", ["BPETokenizer"], size=6 << 20)
    def _(run, size=_size):
        tok, _, pieces, want = encode_ref("gpt2", size)
        data = run.place(*pieces)
        op = K.BPETokenizer(**tok.attrs, lib=run.lib)
        _twice(run, "BPETokenizer", lambda: op.evaluate(data + tok.consts), want)

    for _pat in ("scanner", "compiled"):
        @case(f"RegexSplit-{_pat}-{_size}", ["RegexSplit"], size=6 << 20)
        def _(run, pat=_pat, size=_size):
            from tests.test_regex_general import MODEL_PATTERNS
            pattern = BpeTok.load("gpt2_small").pattern if pat == "scanner" else MODEL_PATTERNS[COMPILED]
            inputs = text_inputs(size)
            want = _regex_split_ref(pattern, size)
            data = run.place(*inputs)
            op = K.RegexSplit("isolate", lib=run.lib)
            for call in range(2):
                got = op.evaluate(data + [u8(pattern)])
                run.same(f"RegexSplit call {call}", got, want[:4] + [inputs[4]])

    @case(f"FusedSplitWordpiece-{_size}", ["FusedSplitWordpiece"], size=4 << 20)
    def _(run, size=_size):
        from tests.test_ops_parity import BERT_PUNCT, BERT_WS
        tok, _, want = wordpiece_ref(size)
        data = run.place(*text_inputs(size))
        fused = K.FusedSplitWordpiece(K.RegexSplit("remove", lib=run.lib), K.RegexSplit("isolate", lib=run.lib),
                                      K.WordpieceTokenizer(tok["suffix_indicator"], tok["max_bytes_per_word"], lib=run.lib))
        consts = list(pack_strings(tok["vocab"])) + [np.asarray(tok["unk_id"], np.int32)]
        _twice(run, "FusedSplitWordpiece", lambda: fused.evaluate(data, u8(BERT_WS), u8(BERT_PUNCT), consts), want)

    @case(f"WordpieceTokenizer-{_size}", ["WordpieceTokenizer"], size=6 << 20)
    def _(run, size=_size):
        tok, words, want = wordpiece_ref(size)
        data = run.place(*words)
        op = K.WordpieceTokenizer(tok["suffix_indicator"], tok["max_bytes_per_word"], lib=run.lib)
        consts = list(pack_strings(tok["vocab"])) + [np.asarray(tok["unk_id"], np.int32)]
        _twice(run, "WordpieceTokenizer", lambda: op.evaluate(data + consts), want)

    @case(f"FusedSpecialSplitBPE-{_size}", ["FusedSpecialSplitBPE"], size=4 << 20)
    def _(run, size=_size):
        tok, pat, want = special_ref(size)
        data = run.place(*text_inputs(size, True))
        fused = K.FusedSpecialSplitBPE(K.SpecialTokensSplit(lib=run.lib), K.RegexSplit("isolate", lib=run.lib), K.BPETokenizer(**tok.attrs, lib=run.lib))
        _twice(run, "FusedSpecialSplitBPE", lambda: fused.evaluate(data + [u8(pat)], tok.pattern_u8(), tok.consts), want)

    @case(f"FusedEncodeDense-{_size}", ["FusedEncodeDense"], backends=("emu", "hip-device"), size=4 << 20)   # (device tensors only)
    def _(run, size=_size):
        tok, pat, ids = special_ref(size)
        (tb, te), = O.truncate([(ids[0], ids[1])], 20, "right", "longest_first")
        one = lambda v: (np.zeros(1, np.int32), np.full(1, len(v), np.int32), np.asarray(v, np.int32))   # noqa: E731
        cb, ce, cdata = O.combine_segments([one((7,)), (tb, te, ids[2]), one((9, 11))], [0, 1, 2])[:3]
        width = int((ce - cb).max())
        ref_ids, ref_mask = O.ragged_to_dense(cb, ce, cdata, width, 50256, pad_right=True)
        data = run.place(*text_inputs(size, True))
        op = K.FusedEncodeDense(K.RegexSplit("isolate", lib=run.lib), K.BPETokenizer(**tok.attrs, lib=run.lib), K.SpecialTokensSplit(lib=run.lib),
                                max_length=20, trunc_side="right", pad_right=True, pad_value=50256, prefix=(7,), suffix=(9, 11))
        _twice(run, "FusedEncodeDense", lambda: op.evaluate(data, tok.pattern_u8(), tok.consts, special_pattern=u8(pat), row_capacity=width),
               [ref_ids, np.asarray(ref_mask).astype(bool)])


@lru_cache(maxsize=None)
def _regex_split_ref(pattern, size):
    return [np.asarray(x) for x in O.RegexSplit(pattern, "isolate")(*text_inputs(size))[:5]]


@lru_cache(maxsize=None)
def wordpiece_ref(size):
    from tests.test_ops_parity import bert_words
    from tools.make_tokenizers import load_tokenizer
    tok = load_tokenizer("bert_small")
    words = [np.asarray(x) for x in bert_words(list(text_inputs(size)))]
    return tok, words, list(O.WordpieceTokenizer(tok["vocab"], tok["suffix_indicator"], tok["max_bytes_per_word"])(*words, tok["unk_id"]))


@lru_cache(maxsize=None)
def special_ref(size):
    tok = BpeTok.load("gpt2_small")
    pat = O.special_tokens_pattern([("<|endoftext|>", False, False)])
    s = O.SpecialTokensSplit(pat)(*text_inputs(size, True))
    return tok, pat, list(tok.oracle()(*O.RegexSplit(tok.pattern, "isolate")(*s[:5], skips=s[5])[:5]))


# ================================================================================================ strings in, strings or numbers out
@lru_cache(maxsize=None)
def window_batch():
    """tests/test_utf8_validate.py::test_symbols_across_the_64_byte_windows, cut to k = 63, 64, 65."""
    seqs = [b"\xc3\xa9", b"\xe5\x85\x83", b"\xf0\x9f\x98\x81", b"\xc0\xaf", b"\xc1\xbf", b"\xe0\x80\xaf", b"\xe0\x9f\xbf", b"\xe0\xa0\x80",
            b"\xf0\x80\x80\xaf", b"\xf0\x8f\xbf\xbf", b"\xf0\x90\x80\x80", b"\xf7\xbf\xbf\xbf", b"\xc3", b"\xe5\x85", b"\xe5", b"\xf0\x9f\x98", b"\xf0\x9f",
            b"\xf0", b"\x80", b"\x80\x80\x80\x80", b"\xc3\xa9\x80", b"\xe5\x85\x83\xbf\xbf", b"\xf8\x80", b"\xff", b"\xc3\xc3\xa9", b"\xe5\xc3\xa9",
            b"\xf0\xe5\x85\x83", b"\xe5\x85\xc3", b"\xf0\x9f\x98\xf0\x9f\x98\x81", b"\xed\xa0\x80", b"\xf4\x90\x80\x80"]
    strings = []
    for k in (63, 64, 65):
        for q in seqs:
            strings += [b"a" * k + q, b"a" * k + q + b"z" * 5, b"\xc3\xa9" * (k // 2) + b"b" * (k % 2) + q + b"\xe5\x85\x83"]
    return tuple(O.pack_strings(strings))


for _replace in (False, True):
    @case(f"UTF8Validate-{'replace' if _replace else 'ignore'}", ["UTF8Validate"])
    def _(run, replace=_replace):
        b, e, c = window_batch()
        run.same("UTF8Validate", K.UTF8Validate(replace_mode=replace, lib=run.lib).evaluate(run.place(b, e, c)), list(O.utf8_validate(b, e, c, replace)))


@lru_cache(maxsize=None)
def charsmap_rows():
    """tests/test_charsmap.py::test_row_sizes_and_tile_boundaries without its 8 KB row."""
    from tests.test_charsmap import SMALL, make_blob
    key = b"mnopqrstuvwx"
    rows = [b"q", b"x" * 63, b"y" * 64, b"z" * 65, ("é" * 40).encode()[:63], ("é" * 40).encode()[:65], b"a" * 63 + "あ".encode() + b"b"]
    rows += [b"." * off + key + b"." * 30 for off in range(50, 71)]
    rows += [b" " * off + key + b"  " + key for off in range(250, 262)]
    rows += [b"." * off + b"\xe3\x81\x82" * 3 + b"\xe3\x81" for off in range(58, 66)]
    return make_blob(SMALL), tuple(O.pack_strings(rows))


@case("CharsMapNormalization", ["CharsMapNormalization"])
def _(run):
    from tests.charsmap_ref import CharsMapRef
    from tests.test_charsmap import flags_of
    blob, (b, e, c) = charsmap_rows()
    data = run.place(b, e, c)
    for f in (0, 7):
        got = K.CharsMapNormalization(lib=run.lib, **flags_of(f)).evaluate(data + [np.frombuffer(blob, np.uint8)])
        run.same(f"flags {f}", got, list(CharsMapRef(blob, **flags_of(f))(b, e, c)))


@lru_cache(maxsize=None)
def golden_charsmap_strings():
    from tests.charsmap_ref import CharsMapRef
    from tests.test_charsmap import golden
    g = golden()
    blob = g["blobs"]["nmt_nfkc_cf"]
    b, e, c = O.pack_strings(g["strings"][:120])
    return blob, (b, e, c), list(CharsMapRef(blob)(b, e, c))


@case("NormalizeUnicode", ["NormalizeUnicode"])
def _(run):
    blob, strings, want = golden_charsmap_strings()
    run.same("NormalizeUnicode", K.NormalizeUnicode("nfkc", charsmap=blob, lib=run.lib).evaluate(run.place(*strings)), want)


@case("CaseFold", ["CaseFold"])
def _(run):
    from tests.charsmap_ref import case_fold_ascii
    blob, strings, want = golden_charsmap_strings()
    run.same("utf-8", K.CaseFold("utf-8", charsmap=blob, lib=run.lib).evaluate(run.place(*strings)), want)
    every = bytes(range(256))
    b, e = i32([0, 256, 100]), i32([256, 256, 130])
    data = run.place(b, e, np.frombuffer(every, np.uint8))
    for lower in (True, False):
        text = b"".join(case_fold_ascii(every[x:y], lower) for x, y in zip(b, e))
        run.same(f"bytes, lower={lower}", K.CaseFold(encoding="", lower=lower, lib=run.lib).evaluate(data),
                 [i32([0, 256, 256]), i32([256, 256, 286]), np.frombuffer(text, np.uint8)])


@lru_cache(maxsize=None)
def regex_norm_ref():
    """A class-path pattern of tests/test_regex_normalization.py over its rows around bytes 64 and 2048."""
    from tests.pcre2_substitute import normalize
    from tests.test_regex_normalization import CONSTRUCTORS, pack
    strs = ["a" * 63, "a" * 64, "a" * 65, " " * 64, "元" * 63, "元" * 64, "元" * 65, "a" * 63 + "元", "a" * 62 + "元 ", "a" * 61 + "́元", "a" * 2047 + "元x",
            "a" * 2046 + "元 ", " " * 2045 + "気元", "x" * 62 + "​" + " ", "a" * 63 + "é" * 3, "", " ", "it 's\tnot\n\nso", "\x01ctl \r\n"]
    pattern, replace, g = CONSTRUCTORS["replace_whitespace"]
    bs, b, e, c = pack(strs)
    return pattern, replace, g, (b, e, c), [np.asarray(x) for x in normalize(bs, pattern, replace, g)]


for _path in ("class", "general"):
    @case(f"RegexNormalization-{_path}", ["RegexNormalization"])
    def _(run, path=_path):
        pattern, replace, g, strings, want = regex_norm_ref()
        if path == "general":
            run.monkeypatch.setenv("OVTK_REGEX_NORM_GENERAL", "1")   # (read at create)
        got = K.RegexNormalization(g, lib=run.lib).evaluate(run.place(*strings) + [u8(pattern), u8(replace)])
        run.same(path, got, want)


@lru_cache(maxsize=None)
def byte_level_ref():
    """tests/test_string_ops.py: every byte value, then its test_element_counts at 65 elements in six rows."""
    from tests import string_ops_ref as R
    rng = np.random.default_rng(65)
    texts = [bytes(range(256))] + [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in rng.integers(0, 9, 65)]
    b, e, c = pack_strings(texts)
    cuts = np.sort(rng.integers(0, 67, 5)).astype(np.int32)
    rb, re_ = np.concatenate([[0], cuts]).astype(np.int32), np.concatenate([cuts, [66]]).astype(np.int32)
    mapped = R.bytes_to_chars(rb, re_, b, e, c, None)
    return (rb, re_, b, e, c), [np.asarray(x) for x in mapped], [np.asarray(x) for x in R.chars_to_bytes(rb, re_, *mapped)]


@case("BytesToChars", ["BytesToChars"])
def _(run):
    inputs, mapped, _ = byte_level_ref()
    run.same("BytesToChars", K.BytesToChars(lib=run.lib).evaluate(run.place(*inputs)), list(inputs[:2]) + mapped)


@case("CharsToBytes", ["CharsToBytes"])
def _(run):
    inputs, mapped, back = byte_level_ref()
    run.same("CharsToBytes", K.CharsToBytes(lib=run.lib).evaluate(run.place(inputs[0], inputs[1], *mapped)), back)


@case("ContribStringSplit", ["ContribStringSplit"])
def _(run):
    from tests import string_ops_ref as R
    from tests.test_string_ops import SPLIT_CASES
    for delim, texts in (SPLIT_CASES[3], SPLIT_CASES[2]):
        b, e, c = pack_strings(texts)
        data = run.place(b, e, c)
        for skip_empty in (0, 1):
            got = K.ContribStringSplit(lib=run.lib).evaluate(data + [np.frombuffer(delim, np.uint8), np.asarray([skip_empty], np.uint8)])
            run.same(f"{delim!r} skip_empty={skip_empty}", got, list(R.string_split(b, e, c, delim, bool(skip_empty))))


@case("ContribStringJoin", ["ContribStringJoin"])
def _(run):
    from tests import string_ops_ref as R
    from tests.test_string_ops import JOIN_TEXTS
    b, e, c = pack_strings(JOIN_TEXTS)
    b, e = b.reshape(4, 6), e.reshape(4, 6)
    data = run.place(b, e, c)
    for axis in (0, 1):
        got = K.ContribStringJoin(lib=run.lib).evaluate(data + [np.frombuffer(b"12345", np.uint8), np.asarray([axis], np.int64)])
        run.same(f"axis {axis}", got, list(R.string_join(b, e, c, b"12345", axis)))


@case("StringTensorUnpack", ["StringTensorUnpack"], backends=("emu", "hip-device"))   # (the device-resident packed buffer)
def _(run):
    """The C entry point: ops.py allocates the three outputs itself (_device_alloc)."""
    from tests.test_string_tensor import STRINGS, wire
    packed = wire(STRINGS)
    want = O.pack_strings(STRINGS)
    src = run.place(packed)
    rows = (len(packed) - 8) // 4
    ob, oe, oc = run.carve(rows, "i32"), run.carve(rows, "i32"), run.carve(len(packed), "u8")
    out = L.StringsOut(Arena.pointer(ob), Arena.pointer(oe), Arena.pointer(oc), len(packed), 0)
    n = C.c_int64(0)
    L.check(run.lib, run.lib.ovtk_string_tensor_unpack(Arena.pointer(src), C.c_int64(len(packed)), L.MEM_DEVICE, C.byref(out), C.c_int64(rows), C.byref(n),
                                                       0, run.arena.stream))
    run.same("StringTensorUnpack", [ob[:n.value], oe[:n.value], oc[:out.n_chars]], list(want))


@case("StringTensorPack", ["StringTensorPack"], backends=("emu", "hip-device"))   # (begins, ends, chars in device memory)
def _(run):
    """The C entry point: ops.py allocates the packed buffer itself."""
    from tests.test_string_tensor import wire
    rng = np.random.default_rng(3)
    strings = [bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8)) for _ in range(130)]
    lens = np.array([len(s) for s in strings])
    starts = (np.cumsum((lens + 3)[::-1])[::-1] - (lens + 3)).astype(np.int32)   # reversed order in memory, with gaps
    chars = np.zeros(int((lens + 3).sum()) + 1, np.uint8)
    for i, s in enumerate(strings):
        chars[starts[i]:starts[i] + lens[i]] = np.frombuffer(s, np.uint8)
    b, e, c = run.place(starts, (starts + lens).astype(np.int32), chars)
    cap = int(run.lib.ovtk_string_tensor_packed_bytes(C.c_int64(len(strings)), C.c_int64(int(lens.sum()))))
    buf = run.carve(cap, "u8")
    s = L.Strings(Arena.pointer(b), Arena.pointer(e), Arena.pointer(c), len(strings), len(chars))
    n = C.c_int64(0)
    L.check(run.lib, run.lib.ovtk_string_tensor_pack(C.byref(s), Arena.pointer(buf), C.c_int64(cap), L.MEM_DEVICE, C.byref(n), 0, run.arena.stream))
    run.same("StringTensorPack", [buf[:n.value]], [wire(strings)])


@case("SpecialTokensSplit", ["SpecialTokensSplit"])
def _(run):
    from tests.test_special_tokens import TOKEN_SETS
    tokens = [("<|endoftext|>", False, False), ("<pad>", True, True)]   # test_skips_input_and_ragged_rows
    pat = O.special_tokens_pattern(tokens)
    b, e, c = O.pack_strings([b"hello <|endoftext|> world", b"<pad>", b"", b"  <pad>  x<|endoftext|>", b"keep <|endoftext|> whole"])
    ins = [i32([0, 2, 2]), i32([2, 2, 5]), b, e, c, np.array([0, 0, 0, 0, 1], np.uint8)]
    ref = O.SpecialTokensSplit(pat)(*ins[:5], skips=ins[5])
    got = K.SpecialTokensSplit(lib=run.lib).evaluate(run.place(*ins) + [u8(pat)])
    run.same("7-input form", list(got[:4]) + [got[5]], [np.asarray(x) for x in ref[:4]] + [np.asarray(ref[5]).astype(np.uint8)])
    tokens = TOKEN_SETS[1]                                              # test_random_texts
    rng = np.random.default_rng(len(tokens) * 7 + len(tokens[0][0]))
    alphabet = [t for t, _, _ in tokens] * 3 + [" ", " ", "\t", "\n", " ", "　", "a", "b", "c", "x", "y", "<", ">", "s", "|", "é", "元", "▁", "<s", "</", "[MASK"]
    strings = ["".join(rng.choice(alphabet, size=int(rng.integers(0, 24)))) for _ in range(70)] + ["", " ", " " * 300 + tokens[0][0] + " " * 300]
    inputs = one_string_per_row(strings)
    pat = O.special_tokens_pattern(tokens)
    ref = O.SpecialTokensSplit(pat)(*inputs)
    got = K.SpecialTokensSplit(lib=run.lib).evaluate(run.place(*inputs) + [u8(pat)])
    run.same("random texts", list(got[:4]) + [got[5]], [np.asarray(x) for x in ref[:4]] + [np.asarray(ref[5]).astype(np.uint8)])


@lru_cache(maxsize=None)
def trie_ref():
    """tests/test_trie_tokenizer.py::test_kernel_matches_oracle at the emulator's size."""
    from tests.test_trie_tokenizer import rwkv_like_vocab
    rng = np.random.default_rng(2)
    vocab, indices = rwkv_like_vocab(rng)
    strings = [bytes(rng.choice(list(b"abcdeft \n\xe4\xb8\xad\xe6\x96\x87xyz\x00\xff"), size=int(rng.integers(0, 90))).tolist()) for _ in range(120)]
    strings[3] = b""
    b, e, c = O.pack_strings(strings)
    cuts = np.unique(np.concatenate([[0, len(strings)], rng.integers(0, len(strings), len(strings) // 2)])).astype(np.int32)
    rb, re_ = np.concatenate([cuts[:-1], [5]]).astype(np.int32), np.concatenate([cuts[1:], [5]]).astype(np.int32)
    return (rb, re_, b, e, c), list(O.pack_strings(vocab)) + [indices], list(O.TrieTokenizer(vocab, indices)(rb, re_, b, e, c))


@case("TrieTokenizer", ["TrieTokenizer"])
def _(run):
    inputs, consts, want = trie_ref()
    run.same("TrieTokenizer", K.TrieTokenizer(lib=run.lib).evaluate(run.place(*inputs) + consts), want)


@lru_cache(maxsize=None)
def unigram_ref():
    from tests.test_unigram import _golden, _rows
    from tests.unigram_ref import UnigramRef
    vocab, scores, unk, strings, _ = _golden()
    b, e, c = O.pack_strings(strings[:60])
    rb, re_ = _rows(60)
    scores = np.asarray(scores, np.float32)
    return unk, (rb, re_, b, e, c), list(O.pack_strings(vocab)) + [scores], list(UnigramRef(vocab, scores, unk_token_id=unk)(rb, re_, b, e, c))


@case("UnigramTokenizer", ["UnigramTokenizer"])
def _(run):
    unk, inputs, consts, want = unigram_ref()
    run.same("UnigramTokenizer", K.UnigramTokenizer(unk_token_id=unk, lib=run.lib).evaluate(run.place(*inputs) + consts), want)


@lru_cache(maxsize=None)
def sentencepiece_ref():
    from tests.test_sentencepiece import Golden, pack, sparse_of
    g = Golden()
    return g.models["bytes"], pack(g.rows[:80]), list(sparse_of(g.ids["bytes", "plain"][:80]))


@case("SentencepieceTokenizer", ["SentencepieceTokenizer"], min_align={"i64": 16})   # include/ovtk_amd.h: `indices` 16-byte aligned
def _(run):
    model, strings, want = sentencepiece_ref()
    run.same("SentencepieceTokenizer", K.SentencepieceTokenizer(lib=run.lib).evaluate([model] + run.place(*strings)), want)


@lru_cache(maxsize=None)
def vocab_encoder_ref(dtype):
    """tests/test_ops_parity.py::test_vocab_encoder with 100 drawn queries, and queries and keys of every length 0..17 (load_words16)."""
    from tools.make_tokenizers import load_tokenizer
    tok = load_tokenizer("bert_small")
    by_len = [bytes([97 + (k + j) % 26 for j in range(k)]) for k in range(18)]
    keys = list(tok["vocab"]) + [tok["vocab"][5], b""] + by_len[1:]
    values = (np.arange(len(keys)) * 7 - 3).astype(dtype)
    rng = np.random.default_rng(3)
    queries = [keys[i] for i in rng.integers(0, len(keys), 100)] + [b"not-in-vocab", b"", b"zz", keys[5], b"\xff\xfe"] + by_len
    queries += [q[:-1] + b"#" for q in by_len[1:]]   # ... and the same with another last byte: not in the vocabulary
    qb, qe, qc = pack_strings(queries[::-1])
    qb, qe = qb[::-1].copy(), qe[::-1].copy()
    return (qb, qe, qc), list(pack_strings(keys)) + [values, np.asarray(-1, dtype)], [np.asarray(O.VocabEncoder(keys, values)(qb, qe, qc, -1), dtype)]


for _dtype in ("int32", "int64"):
    @case(f"VocabEncoder-{_dtype}", ["VocabEncoder"])
    def _(run, dtype=_dtype):
        strings, consts, want = vocab_encoder_ref(dtype)
        run.same("VocabEncoder", K.VocabEncoder(lib=run.lib).evaluate(run.place(*strings) + consts), want)


@lru_cache(maxsize=None)
def hash_ref():
    """tests/test_tf_string_ops.py::every_length_batch cut to the lengths 0..80."""
    from tests.test_tf_string_ops import every_length_batch
    b, e, chars, raw = every_length_batch()
    keep = np.flatnonzero(e - b <= 80)
    nb = (1 << 63) - 1
    return (b[keep].copy(), e[keep].copy(), chars), [np.array([raw[i] % nb for i in keep], np.int64)], nb


@case("StringToHashBucket", ["StringToHashBucket"])
def _(run):
    strings, want, nb = hash_ref()
    run.same("StringToHashBucket", K.StringToHashBucket(nb, lib=run.lib).evaluate(run.place(*strings)), want)


@case("EqualStr", ["EqualStr"])
def _(run):
    from tests.test_tf_string_ops import equal_ref, pack, pairs
    a, b = pairs(65)
    run.same("EqualStr", K.EqualStr(lib=run.lib).evaluate(run.place(*(list(pack(a)) + list(pack(b, 5))))), [equal_ref(a, b)])


# ================================================================================================ offsets only
@case("Truncate", ["Truncate"])
def _(run):
    from tests.test_truncate_combine import ragged
    rng = np.random.default_rng(7)
    (b0, e0, d0), (b1, e1, d1) = ragged(rng, 70, 24), ragged(rng, 70, 24)
    data = run.place(b0, e0, d0, b1, e1, d1)
    for side in ("right", "left"):
        ref = O.truncate([(b0, e0)], 7, side)
        got = K.Truncate(lib=run.lib).evaluate(data[:3] + [np.int32(7), u8(side), u8("longest_first")])
        run.same(f"single {side}", got, list(ref[0]) + [d0])
        ref = O.truncate([(b0, e0), (b1, e1)], 9, side, "longest_first")
        got = K.Truncate(lib=run.lib).evaluate(data + [np.int32(9), u8(side), u8("longest_first")])
        run.same(f"pair {side}", got, [ref[0][0], ref[0][1], d0, ref[1][0], ref[1][1], d1])


@case("CombineSegments", ["CombineSegments"])
def _(run):
    from tests.test_truncate_combine import ragged
    rng = np.random.default_rng(9)
    one = lambda v: (i32([0]), i32([1]), i32([v]))   # noqa: E731
    segs, ids = [one(101), ragged(rng, 70, 200), one(102), ragged(rng, 70, 90), one(102)], [0, 0, 0, 1, 1]   # bert_pair
    ref = O.combine_segments(segs, ids)
    got = K.CombineSegments(lib=run.lib).evaluate(run.place(*[x for s in segs for x in s]) + [i32(ids)])
    run.same("CombineSegments", got, [ref[0], ref[1], ref[2], ref[0], ref[1], ref[3]])


@case("FusedEncodeTail", ["FusedEncodeTail"])
def _(run):
    from tests.test_truncate_combine import ragged
    rng = np.random.default_rng(12)
    one = lambda v: (i32([0]), i32([1]), i32([v]))   # noqa: E731
    a, b2 = ragged(rng, 70, 70), ragged(rng, 70, 50)
    segs, ids, trunc = [one(101), a, one(102), b2, one(102)], [0, 0, 0, 1, 1], [1, 3]   # pair_longest
    cut = [list(s) for s in segs]
    for j, (tb, te) in zip(trunc, O.truncate([(segs[j][0], segs[j][1]) for j in trunc], 61, "right", "longest_first")):
        cut[j][0], cut[j][1] = tb, te
    cb, ce, cd, ci = O.combine_segments([tuple(s) for s in cut], ids)
    for pad_right, T in ((True, None), (False, 48)):
        width = int((ce - cb).max()) if T is None else T
        want_ids, want_mask = O.ragged_to_dense(cb, ce, cd, width, 9, pad_right)
        want_types, _ = O.ragged_to_dense(cb, ce, ci, width, 4, pad_right)
        placed = [tuple(run.place(*s)) for s in segs]
        got = K.FusedEncodeTail(61, "right", "longest_first", pad_right, lib=run.lib).evaluate(placed, ids, truncated=trunc, pad_value=9, type_pad_value=4,
                                                                                             target_dim=T)
        run.same(f"pad_right {pad_right} target {T}", got, [want_ids, np.asarray(want_mask).astype(bool), want_types])


RAGGED_HAND = [([2, 2, 3], 5), ([0, 0, 3, 3, 3, 6], 7), ([0, 1, 1], 6), ([2, 2, 2, 2], 3), ([0, 1, 2, 3], 4), ([1], 3)]   # test_ragged_hand_cases


@case("RaggedToRagged", ["RaggedToRagged"])
def _(run):
    from tests.test_tf_string_ops import ragged_ref
    for rowids, batch in RAGGED_HAND + [(sorted(np.random.default_rng(1).integers(0, 90, 300).tolist()), 90)]:
        wb, we, written = ragged_ref(rowids, batch)
        assert written.all()
        run.same(f"{rowids[:8]} {batch}", K.RaggedToRagged(lib=run.lib).evaluate([run.place(i32(rowids)), i32([batch])]), [wb, we])


@case("RaggedToSparse", ["RaggedToSparse"], min_align={"i32": 8})   # include/ovtk_amd.h: `out` 8-byte aligned
def _(run):
    for lens, lead in ((np.random.default_rng(3).integers(0, 200, 65).tolist(), 0), ([2, 129, 0, 4], 17), ([3, 0, 0, 70, 0, 1], 0)):
        ends = np.cumsum(lens, dtype=np.int64).astype(np.int32) + lead
        begins = (ends - i32(lens)).astype(np.int32)
        want = np.array([(i, j) for i in range(len(begins)) for j in range(ends[i] - begins[i])], np.int32).reshape(-1, 2)
        run.same(f"{len(lens)} rows", K.RaggedToSparse(lib=run.lib).evaluate(run.place(begins, ends)), [want])


@case("RaggedTensorPack", ["RaggedTensorPack"])
def _(run):
    data = np.arange(17, dtype=np.int32)
    run.same("RaggedTensorPack", K.RaggedTensorPack(lib=run.lib).evaluate(run.place(i32([0, 5]), i32([5, 17]), data)), [data])


# ================================================================================================ the tests
@pytest.mark.parametrize("backend,name,shift,fill", _params(), indirect=["backend"])
def test_placed(backend, name, shift, fill, monkeypatch):
    c = CASES[name]
    arena = Arena(backend, fill, c.size)
    run = Run(backend, arena, shift, monkeypatch)
    with arena.outputs(monkeypatch, shift, c.min_align):
        c.fn(run)
    assert run.compared, "a case must compare at least one output"
    arena.check()


def _raw_pointer(view, off):
    return C.c_void_p((view.data_ptr() if hasattr(view, "data_ptr") else view.ctypes.data) + off)


def test_alignment_rules_are_enforced(backend):
    """The three buffers include/ovtk_amd.h gives an alignment rule: breaking it is OVTK_E_ARG, decided on the host -- no kernel runs."""
    arena = Arena(backend, 0x00, 1 << 20)
    mem, lib = arena.mem_kind, backend.lib
    # ovtk_numeric_to_string: the input aligned to its element's size
    x = arena.place(np.arange(9, dtype=np.int64), 0)
    ob, oe, oc = arena.carve(8, "i32", 0), arena.carve(8, "i32", 0), arena.carve(256, "u8", 0)
    out = L.StringsOut(Arena.pointer(ob), Arena.pointer(oe), Arena.pointer(oc), 256, 0)
    assert lib.ovtk_numeric_to_string(_raw_pointer(x, 4), L.NUM_I64, C.c_int64(8), C.byref(out), mem, 0, arena.stream) == L.E_ARG
    assert lib.ovtk_numeric_to_string(_raw_pointer(x, 8), L.NUM_I64, C.c_int64(8), C.byref(out), mem, 0, arena.stream) == L.OVTK_OK
    if mem != L.MEM_DEVICE:
        arena.check()
        return   # (the two rules below are about device memory: a host buffer is staged)
    # ovtk_ragged_to_sparse: `out` 8-byte aligned
    b, e = arena.place(i32([0, 3]), 0), arena.place(i32([3, 5]), 0)
    sparse = arena.carve(12, "i32", 0, min_align=8)
    n = C.c_int64(0)
    assert lib.ovtk_ragged_to_sparse(Arena.pointer(b), Arena.pointer(e), C.c_int64(2), _raw_pointer(sparse, 4), C.c_int64(5), C.byref(n), mem, 0,
                                     arena.stream) == L.E_ARG
    # ovtk_sentencepiece_run: `indices` 16-byte aligned
    model, (sb, se, sc), _ = sentencepiece_ref()
    op = K.SentencepieceTokenizer(lib=lib)
    op._ensure(model)
    sb, se, sc = arena.place(sb[:2], 0), arena.place(se[:2], 0), arena.place(sc[:int(se[1])], 0)
    idx, val, shape = arena.carve(2 * 512 + 1, "i64", 0, min_align=16), arena.carve(512, "i32", 0), arena.carve(2, "i64", 0)
    s = L.Strings(Arena.pointer(sb), Arena.pointer(se), Arena.pointer(sc), 2, int(se[1]))
    sparse_out = L.SparseI32Out(_raw_pointer(idx, 8), Arena.pointer(val), Arena.pointer(shape), 512, 0)
    assert lib.ovtk_sentencepiece_run(op._h, C.byref(s), C.byref(sparse_out), mem, arena.stream) == L.E_ARG
    arena.check()


# ------------------------------------------------------------------------------------------------ the harness itself (CPU tier)
def test_arena_detects_a_stray_write(emu_lib):
    from tests.conftest import Backend
    backend = Backend("emu", emu_lib)
    arena = Arena(backend, 0xE2, 1 << 16)
    inp = arena.place(np.arange(10, dtype=np.int32), 3)
    out = arena.carve(7, "u8", 3)
    assert inp.ctypes.data % 16 == 0 and out.ctypes.data % 16 == 3
    arena.check()
    at = out.ctypes.data - arena.base + 7
    arena.mem[at] = 0x00                       # one byte just behind the output
    with pytest.raises(AssertionError, match=r"stray write: byte \+7 relative to buffer 1 \(uint8\[7\]\)"):
        arena.check()
    arena.mem[at] = 0xE2
    arena.mem[out.ctypes.data - arena.base - 1] = 0x01   # ... and one just in front of it
    with pytest.raises(AssertionError, match=r"stray write: byte -1 relative to buffer 1"):
        arena.check()
    arena.mem[out.ctypes.data - arena.base - 1] = 0xE2
    arena.check()
    inp[4] = 99                                # a placed input
    with pytest.raises(AssertionError, match=r"input overwritten: byte \+16 of input 0 \(int32\[10\]\)"):
        arena.check()
    assert GUARD == 4096 and out.ctypes.data - (inp.ctypes.data + 40) >= GUARD


def test_every_op_class_has_a_case():
    classes = [n for n, c in inspect.getmembers(K, inspect.isclass)
               if c.__module__ == K.__name__ and ((issubclass(c, K._Op) and c is not K._Op) or n.startswith("Fused"))]
    assert len(classes) >= 38
    covered = {op for c in CASES.values() for op in c.ops}
    assert covered <= set(classes), covered - set(classes)
    for n in classes:
        assert (n in covered) != (n in EXEMPT), f"{n}: a case in this module, or an entry in EXEMPT with the reason -- one of the two"
    for n, why in EXEMPT.items():
        assert "no data buffer" in why, f"{n}: the only reason is that evaluate takes no data buffer in the call's memory space"
