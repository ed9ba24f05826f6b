"""The reference's tokenizer graph as a list of steps over the mirror ops of ops.py, and `fuse()`: the rewrite that puts the fused
entry points behind the operator interface.

The reference builds a converted tokenizer as a chain of custom-op nodes, each one an `evaluate()` of its own
(python/openvino_tokenizers/tokenizer_pipeline.py: SpecialTokensSplit -> RegexSplitStep :392-489 -> BPETokenizationStep :773-822 /
WordPieceTokenizationStep :641-659 -> TruncationStep -> CombineSegmentsStep -> PaddingStep :1211-1236, assembled :1613-1636; the
detokenizer VocabDecoderStep -> ByteFallbackStep / FuseStep :1321-1371).  `Pipeline(steps).run(...)` executes such a chain op by op
through the C ABI, one library call per node -- what `core.add_extension()` + the op classes of adapter/ give an OpenVINO user.
`fuse(steps)` recognises the sub-chains the library has one call for and replaces them:

  [SpecialTokensSplit] RegexSplit(isolate, a pattern the span kernel scans) BPETokenizer Truncate CombineSegments(constant ids in front
      / behind) Padding                                         -> FusedEncodeDenseStep      ovtk_encode_dense_enqueue / _finish
  [SpecialTokensSplit] RegexSplit BPETokenizer                  -> FusedSplitBPEStep          ovtk_encode_run / ovtk_encode_special_run
  RegexSplit(\\s+, remove) RegexSplit(BERT delimiters, isolate) WordpieceTokenizer
                                                                -> FusedSplitWordpieceStep    ovtk_wordpiece_encode_run
  Truncate CombineSegments Padding                              -> FusedEncodeTailStep        ovtk_encode_tail_run
  [SpecialTokensSplit] RegexSplit BPETokenizer PairTruncation PairCombineSegments PairPadding (a list made by add_second_input)
                                                                -> FusedPairEncodeDenseStep   ovtk_encode_pair_dense_enqueue / _finish
  the BERT splits WordpieceTokenizer PairTruncation PairCombineSegments PairPadding
                                                                -> FusedPairWordpieceDenseStep ovtk_wordpiece_encode_pair_dense_enqueue
  VocabDecoder [ByteFallback] FuzeRagged                        -> FusedDetokenizeStep        ovtk_detokenize_run

and leaves every other step as it is -- a RegexSplit / BPETokenizer pair with a BytesToCharsStep between them and a VocabDecoder with a
CharsToBytesStep behind it (the old-style byte-level graphs, vocabulary in "chars" form) are no such sub-chain and run op by op; the normalizers (CharsmapStep, NormalizeUnicode, CaseFoldStep, RegexNormalizationStep) and the detokenizer's RegexDecodingSteps among them: a chain behind them
is fused as if they were not there.  The rewritten list gives the same outputs as the original one (tests/test_pipeline_fuse.py:
bit for bit, on BASELINE.json's configurations); adapter/fuse_pass.cpp is the same recogniser over ov::Node chains.
"""
from __future__ import annotations

import numpy as np

from . import ops as K

# ---------------------------------------------------------------------------------------------------------------- state
# What flows between steps: ("strings", [ragged_begins, ragged_ends, begins, ends, chars, skips | None]) -- a ragged tensor of strings --,
# ("ids", [begins, ends, ids]) -- ragged token ids --, ("dense", [input_ids, attention_mask]), ("tokens", [ids[B, S]]) and
# ("token_strings", [ragged_begins, ragged_ends, begins, ends, chars]) / ("text", [begins, ends, chars]) on the way back.


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _u8(s):
    return np.frombuffer(s if isinstance(s, bytes) else s.encode(), np.uint8)


def _like(ref, values, dtype=np.int32):
    """A small constant next to `ref` (a device tensor stays on its device)."""
    a = np.asarray(values, dtype)
    if _is_torch(ref):
        import torch
        return torch.as_tensor(a, device=ref.device)
    return a


class Step:
    lib = None

    def apply(self, kind, vals):
        raise NotImplementedError


class _NormalizationStep(Step):
    """A normalizer in front of the splits: strings -> strings, the ragged rows and the skips passed through."""

    def apply(self, kind, vals):
        assert kind == "strings"
        rb, re_, b, e, c = vals[:5]
        skips = vals[5] if len(vals) > 5 else None
        out = self.op.evaluate([b, e, c] + ([skips] if skips is not None else []))
        return "strings", [rb, re_] + list(out[:3]) + [skips]


class CharsmapStep(_NormalizationStep):
    """src/charsmap_normalization.cpp:34-69 (tokenizer_pipeline.py:293-352): sentencepiece's normalizer over a precompiled charsmap --
    `charsmap` bytes, the table of `normalization_form` where that is given (this library ships none)."""

    def __init__(self, charsmap=None, normalization_form=None, add_dummy_prefix=False, remove_extra_whitespaces=True, escape_whitespaces=False,
                 case_fold=False, nmt=False, lib=None):
        if charsmap is None:
            raise ValueError("CharsmapStep: a precompiled charsmap is needed (charsmap=<bytes>); this library ships no tables")
        self.charsmap = bytes(charsmap)
        self.op = K.CharsMapNormalization(add_dummy_prefix, remove_extra_whitespaces, escape_whitespaces, normalization_form=normalization_form or "",
                                          case_fold=case_fold, nmt=nmt, charsmap=self.charsmap, lib=lib)


class NormalizeUnicode(_NormalizationStep):
    """src/normalize_unicode.cpp:32-62 (tokenizer_pipeline.py:168-190): the charsmap of NFD / NFC / NFKD / NFKC, every flag off."""

    def __init__(self, normalization_form="NFD", charsmap=None, lib=None):
        if normalization_form not in ("NFD", "NFC", "NFKD", "NFKC"):
            raise ValueError(f'[ NormalizeUnicode ] `normalization_form` attribute must be one of ["NFD", "NFC", "NFKD", "NFKC"], got {normalization_form}.')
        if charsmap is None:
            raise ValueError("NormalizeUnicode: the form's precompiled charsmap is needed (charsmap=<bytes>); this library ships no tables")
        self.normalization_form = normalization_form
        self.op = K.NormalizeUnicode(normalization_form.lower(), charsmap=charsmap, lib=lib)


class CaseFoldStep(_NormalizationStep):
    """src/case_fold.cpp:34-73 (tokenizer_pipeline.py:194-220): encoding "" shifts the ASCII range, "utf-8" runs the case-folding charsmap."""

    def __init__(self, encoding="utf-8", charsmap=None, lib=None):
        if encoding not in ("", "utf-8"):
            raise ValueError(f"[ CaseFoldStep ] `encoding` attribute must be one of ['', 'utf-8'], got {encoding!r}.")
        self.encoding = encoding
        self.op = K.CaseFold(encoding=encoding, lower=True, charsmap=charsmap, lib=lib)


class RegexNormalizationStep(_NormalizationStep):
    """src/regex_normalization.cpp:127-153 (tokenizer_pipeline.py:224-289): pcre2_substitute per string, with the reference's
    constructors by name."""

    def __init__(self, regex_search_pattern, replace_term, global_replace=True, lib=None):
        self.regex_search_pattern, self.replace_term, self.global_replace = regex_search_pattern, replace_term, bool(global_replace)
        self.op = K.RegexNormalization(global_replace=self.global_replace, lib=lib)

    def apply(self, kind, vals):
        assert kind == "strings"
        rb, re_, b, e, c = vals[:5]
        skips = vals[5] if len(vals) > 5 else None
        out = self.op.evaluate([b, e, c] + ([skips] if skips is not None else []) + [_u8(self.regex_search_pattern), _u8(self.replace_term)])
        return "strings", [rb, re_] + list(out[:3]) + [skips]

    @classmethod
    def strip_accents_regex(cls, lib=None):
        return cls(r"\p{Mn}", "", lib=lib)

    @classmethod
    def add_prefix_whitespace_regex(cls, lib=None):
        return cls(r"^(\S)", r" $1", lib=lib)

    @classmethod
    def replace_whitespace_regex(cls, lib=None):
        return cls(r"\s", " ", global_replace=True, lib=lib)

    @classmethod
    def handle_chinese_chars_regex(cls, lib=None):
        return cls(r"([\p{Han}])", r" $1 ", global_replace=True, lib=lib)

    @classmethod
    def add_prefix_whitespace_to_not_whitespace_regex(cls, lib=None):
        return cls(r"^([^ ])", r" $1", lib=lib)

    @classmethod
    def replace_spaces_metaspace(cls, replace_term="▁", lib=None):
        return cls(r" ", replace_term, lib=lib)

    @classmethod
    def prepend_regex(cls, string, lib=None):
        return cls(r"(?:^)([\s\S])", rf"{string}$1", lib=lib)

    @classmethod
    def prepend_with_check_regex(cls, string, check_string, lib=None):
        return cls(rf"(^)([^{check_string}])", rf"{string}$2", lib=lib)

    @classmethod
    def del_control_chars_regex(cls, lib=None):
        return cls(r"([\x00-\x08\x0B\x0C\x0E-\x1F\x7F-\x9F\p{Cf}])", "", global_replace=True, lib=lib)   # (\n \t \r stay)

    @classmethod
    def strip_regex(cls, left=True, right=True, lib=None):
        return cls(r"^\s*" * left + "|" * (left and right) + r"\s*$" * right, "", lib=lib)

    clean_up_and_remove_extra_whitespaces_regex = strip_regex   # (the strip pattern under the name older converters used)


class RegexDecodingStep(Step):
    """The detokenizer's clean-up steps (tokenizer_pipeline.py:1375-1457): RegexNormalization over the decoded text (always global)."""

    def __init__(self, regex_search_pattern, replace_term, lib=None):
        self.regex_search_pattern, self.replace_term = regex_search_pattern, replace_term
        self.op = K.RegexNormalization(global_replace=True, lib=lib)

    def apply(self, kind, vals):
        assert kind in ("text", "token_strings")
        ragged = list(vals[:2]) if kind == "token_strings" else []
        out = self.op.evaluate(list(vals[len(ragged):len(ragged) + 3]) + [_u8(self.regex_search_pattern), _u8(self.replace_term)])
        return kind, ragged + list(out[:3])

    @classmethod
    def clean_up_tokenization_spaces(cls, lib=None):
        return cls(r"(?| ([\\.\\?\\!,])| ('[ms])| (') | ('[rv]e)| (n't))", r"$1", lib=lib)

    @classmethod
    def parse_replace_dict(cls, replace_dict, lib=None):
        pattern, content = replace_dict.get("pattern", {}).get("String"), replace_dict.get("content")
        if pattern is None or content is None:
            raise ValueError(f"Replace Decoding Op with this parameters: `{replace_dict}` does not support yet.")
        return cls(pattern, content, lib=lib)

    @classmethod
    def parse_strip_dict(cls, replace_dict, lib=None):
        content = replace_dict.get("content")
        if content is None:
            raise ValueError(f"Replace Decoding Op with this parameters: `{replace_dict}` does not support yet.")
        return cls(f"^{content}", "", lib=lib)

    @classmethod
    def rstrip_space(cls, lib=None):
        return cls(r" $", "", lib=lib)

    @classmethod
    def strip_forward_space(cls, lib=None):
        return cls(r"^ ", "", lib=lib)

    @classmethod
    def strip_forward_space_before_not_space(cls, lib=None):
        return cls(r"(^ )([^ ])", r"$2", lib=lib)

    @classmethod
    def replace_end_of_word_suffix(cls, suffix="</w>", lib=None):
        return cls(suffix, " ", lib=lib)

    @classmethod
    def replace_continuing_subword_prefix(cls, prefix="##", lib=None):
        return cls(prefix, "", lib=lib)

    @classmethod
    def replace_sp_spaces(cls, lib=None):
        return cls("▁", " ", lib=lib)


class SpecialTokensSplitStep(Step):
    """src/special_tokens_split.cpp:61-162; in front of every RegexSplit of a converted HF tokenizer (tokenizer_pipeline.py:1613-1636)."""

    def __init__(self, pattern, lib=None):
        self.pattern, self.op = _u8(pattern), K.SpecialTokensSplit(lib=lib)

    def apply(self, kind, vals):
        assert kind == "strings"
        ins = list(vals[:5]) + ([vals[5]] if vals[5] is not None else []) + [self.pattern]
        out = self.op.evaluate(ins)
        return "strings", list(out[:6])


class RegexSplitStep(Step):
    """src/regex_split.cpp:124-324 (tokenizer_pipeline.py:475-489)."""

    def __init__(self, pattern, behaviour="isolate", invert=False, max_splits=-1, lib=None):
        self.pattern, self.behaviour, self.invert, self.max_splits = pattern, behaviour, invert, max_splits
        self.op = K.RegexSplit(behaviour, invert=invert, max_splits=max_splits, lib=lib)

    def apply(self, kind, vals):
        assert kind == "strings"
        ins = list(vals[:5]) + ([vals[5]] if vals[5] is not None else []) + [_u8(self.pattern)]
        out = self.op.evaluate(ins)
        return "strings", list(out[:5]) + [out[5] if len(out) > 5 else None]


class BPETokenizationStep(Step):
    """src/bpe_tokenizer.cpp:47-164 (tokenizer_pipeline.py:773-822).  consts: inputs 5.. of the op."""

    def __init__(self, consts, lib=None, **attrs):
        self.consts, self.op = list(consts), K.BPETokenizer(**attrs, lib=lib)

    def apply(self, kind, vals):
        assert kind == "strings"
        return "ids", self.op.evaluate(list(vals[:5]) + self.consts)   # (BPETokenizer has no skips input: skipped strings arrive as whole pieces)


class WordPieceTokenizationStep(Step):
    """src/wordpiece_tokenizer.cpp:49-133 (tokenizer_pipeline.py:641-659).  consts: vocab (3) + unk_token_id."""

    def __init__(self, consts, suffix_indicator="##", max_bytes_per_word=100, lib=None):
        self.consts, self.op = list(consts), K.WordpieceTokenizer(suffix_indicator, max_bytes_per_word, lib=lib)

    def apply(self, kind, vals):
        assert kind == "strings"
        return "ids", self.op.evaluate(list(vals[:5]) + self.consts)


class UnigramModelStep(Step):
    """src/unigram_tokenizer.cpp:17-77 (tokenizer_pipeline.py:826-883).  vocab: the token strings (bytes or str, id = position);
    vocab_logprobs: one float32 score each.  The reference op has no skips input: a state that carries skips is refused."""

    def __init__(self, vocab, vocab_logprobs, byte_fallback=False, unk_token_id=0, fuse_unk=True, lib=None):
        words = [w if isinstance(w, bytes) else w.encode() for w in vocab]
        ends = np.cumsum([len(w) for w in words], dtype=np.int64).astype(np.int32)
        begins = np.concatenate([[0], ends[:-1]]).astype(np.int32) if len(words) else np.zeros(0, np.int32)
        probs = np.asarray(vocab_logprobs, np.float32).reshape(-1)
        if len(probs) != len(words):
            raise ValueError("UnigramModelStep: vocab and vocab_logprobs differ in length")
        self.consts = [begins, ends, np.frombuffer(b"".join(words), np.uint8), probs]
        self.op = K.UnigramTokenizer(byte_fallback=byte_fallback, unk_token_id=unk_token_id, fuse_unk=fuse_unk, lib=lib)

    def apply(self, kind, vals):
        assert kind == "strings"
        if len(vals) > 5 and vals[5] is not None:
            raise ValueError("UnigramModelStep: the state carries skips (a SpecialTokensSplit in front), and UnigramTokenizer has no skips "
                             "input: skipped strings would be tokenized like any other")
        return "ids", self.op.evaluate(list(vals[:5]) + self.consts)


class SentencepieceModelStep(Step):
    """src/sentence_piece.cpp:188-350 and what python/openvino_tokenizers/hf_parser.py:879-911 puts behind it: the op's sparse ids,
    then two ScatterNDUpdates -- the ids into a [batch, longest row] tensor of `pad_id`, ones into an attention mask of zeros.
    `model`: the serialized sentencepiece model.  The op takes whole sentences: a row of the state is one string (as behind
    StringTensorUnpack), and a state that carries skips is refused as UnigramModelStep refuses it.  The scatter is plain tensor
    indexing next to the op's outputs; it is no hot path.
    `special_tokens`: a list of (token, id) -- the op's 8-input form, which the converter builds for every BPE and CHAR model
    (handle_special_tokens_with_re, hf_parser.py:744-746, :858-877).  The order given is the order of the pattern's alternatives: of
    two tokens that match at one place the earlier one wins (the converter sorts them in reverse, hf_parser.py:859)."""

    def __init__(self, model, add_bos=False, add_eos=False, reverse=False, pad_id=0, nbest_size=1, alpha=1.0, lib=None, special_tokens=None):
        self.model = np.frombuffer(bytes(model), np.uint8)
        self.pad_id = int(pad_id)
        self.special = None
        if special_tokens is not None:
            toks = [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t, _ in special_tokens]
            ends = np.cumsum([len(t) for t in toks], dtype=np.int64).astype(np.int32) if toks else np.zeros(0, np.int32)
            begins = np.concatenate([[0], ends[:-1]]).astype(np.int32) if toks else np.zeros(0, np.int32)
            self.special = [begins, ends, np.frombuffer(b"".join(toks), np.uint8), np.array([i for _, i in special_tokens], np.int32)]
        self.op = K.SentencepieceTokenizer(nbest_size=nbest_size, alpha=alpha, add_bos=add_bos, add_eos=add_eos, reverse=reverse, lib=lib,
                                           special_tokens=special_tokens is not None)

    def apply(self, kind, vals):
        assert kind == "strings"
        if len(vals) > 5 and vals[5] is not None:
            raise ValueError("SentencepieceModelStep: the state carries skips (a SpecialTokensSplit in front), and the 4-input "
                             "SentencepieceTokenizer has no skips input")
        b, e, c = vals[2:5]
        indices, values, dense_shape = self.op.evaluate([self.model, b, e, c] + (self.special or []))
        if _is_torch(values):
            import torch
            shape = [int(x) for x in dense_shape.cpu()]
            ids = torch.full(shape, self.pad_id, dtype=torch.int32, device=values.device)
            mask = torch.zeros(shape, dtype=torch.int32, device=values.device)
        else:
            shape = [int(x) for x in dense_shape]
            ids = np.full(shape, self.pad_id, np.int32)
            mask = np.zeros(shape, np.int32)
        ids[indices[:, 0], indices[:, 1]] = values
        mask[indices[:, 0], indices[:, 1]] = 1
        return "dense", [ids, mask]


class SentencepieceDetokenizeStep(Step):
    """src/sentence_piece.cpp:395-433 (stream=False: SentencePieceProcessor::Decode) or :478-523 (stream=True: the pieces as they
    are): ids [B, S] -> one string per row.  `model`: the serialized sentencepiece model.  fuse() leaves the step as it is."""

    def __init__(self, model, stream=False, lib=None):
        self.model = np.frombuffer(bytes(model), np.uint8)
        self.op = (K.SentencepieceStreamDetokenizer if stream else K.SentencepieceDetokenizer)(lib=lib)

    def apply(self, kind, vals):
        assert kind == "tokens"
        return "text", self.op.evaluate([self.model, vals[0]])


class TruncationStep(Step):
    """src/truncate.cpp:37-150, one input."""

    def __init__(self, max_length, side="right", lib=None):
        self.max_length, self.side, self.op = int(max_length), side, K.Truncate(lib=lib)

    def apply(self, kind, vals):
        assert kind == "ids"
        b, e, ids = vals
        return "ids", self.op.evaluate([b, e, ids, np.int32(self.max_length), self.side.encode(), b"longest_first"])


class CombineSegmentsStep(Step):
    """src/combine_segments.cpp:36-134 with constant segments in front of / behind the sequence (the post-processor's BOS / EOS)."""

    def __init__(self, prefix=(), suffix=(), lib=None):
        self.prefix, self.suffix, self.op = [int(x) for x in prefix], [int(x) for x in suffix], K.CombineSegments(lib=lib)

    def apply(self, kind, vals):
        assert kind == "ids"
        b, e, ids = vals
        segs = []
        if self.prefix:
            segs += [_like(ids, [0]), _like(ids, [len(self.prefix)]), _like(ids, self.prefix)]
        segs += [b, e, ids]
        if self.suffix:
            segs += [_like(ids, [0]), _like(ids, [len(self.suffix)]), _like(ids, self.suffix)]
        k = len(segs) // 3
        return "ids", self.op.evaluate(segs + [np.arange(k, dtype=np.int32)])[:3]


class PaddingStep(Step):
    """src/ragged_to_dense.cpp:70-174 twice: input_ids (pad id) and attention_mask (tokenizer_pipeline.py:1211-1236: the target is the
    longest row, or `target_dim`)."""

    def __init__(self, pad_value=0, pad_right=True, target_dim=None, lib=None):
        self.pad_value, self.pad_right, self.target_dim, self.op = int(pad_value), bool(pad_right), target_dim, K.RaggedToDense(pad_right=pad_right, lib=lib)

    def apply(self, kind, vals):
        assert kind == "ids"
        b, e, ids = vals
        lens = (e - b)
        width = int(self.target_dim) if self.target_dim is not None else (int(lens.max()) if len(lens) else 0)
        dense, mask = self.op.evaluate([b, e, ids, np.int32(width), np.int32(self.pad_value)])
        return "dense", [dense, mask]


class VocabDecoderStep(Step):
    """src/vocab_decoder.cpp:23-87 (tokenizer_pipeline.py:1321-1338).  vocab: begins, ends, chars."""

    def __init__(self, vocab, skip_tokens=(), lib=None):
        self.vocab, self.op = list(vocab), K.VocabDecoder(skip_tokens=skip_tokens, lib=lib)

    def apply(self, kind, vals):
        assert kind == "tokens"
        return "token_strings", self.op.evaluate([vals[0]] + self.vocab)


class ByteFallbackStep(Step):
    """src/byte_fallback.cpp:16-50 (tokenizer_pipeline.py:1363-1371)."""

    def __init__(self, lib=None):
        self.op = K.ByteFallback(lib=lib)

    def apply(self, kind, vals):
        assert kind == "token_strings"
        rb, re_, b, e, c = vals
        return "token_strings", [rb, re_] + self.op.evaluate([b, e, c])


class FuseStep(Step):
    """src/fuze.cpp:20-40 (tokenizer_pipeline.py:1347-1351): a row's token strings become one string."""

    def __init__(self, lib=None):
        self.op = K.FuzeRagged(lib=lib)

    def apply(self, kind, vals):
        assert kind == "token_strings"
        rb, re_, b, e, c = vals
        return "text", self.op.evaluate([rb, re_, b, e]) + [c]


class BytesToCharsStep(Step):
    """src/bytes_to_chars.cpp:284-339 (tokenizer_pipeline.py:783-785, and every byte-level BPE graph converted before the converter
    folded the op away): between RegexSplit and a BPETokenizer whose vocabulary is in its "chars" form.  Skipped pieces stay bytes."""

    def __init__(self, lib=None):
        self.op = K.BytesToChars(lib=lib)

    def apply(self, kind, vals):
        assert kind == "strings"
        skips = vals[5] if len(vals) > 5 else None
        out = self.op.evaluate(list(vals[:5]) + ([skips] if skips is not None else []))
        return "strings", list(out[:5]) + [skips]


class CharsToBytesStep(Step):
    """src/chars_to_bytes.cpp:31-68: behind a VocabDecoder over a "chars"-form vocabulary -- a row's token strings become one string
    of bytes (the step fuses the row itself: no FuseStep behind it)."""

    def __init__(self, lib=None):
        self.op = K.CharsToBytes(lib=lib)

    def apply(self, kind, vals):
        assert kind == "token_strings"
        return "text", self.op.evaluate(list(vals[:5]))


# ---------------------------------------------------------------------------------------------------------------- fused steps
class FusedSplitBPEStep(Step):
    """[SpecialTokensSplit ->] RegexSplit -> BPETokenizer: ovtk_encode_run / ovtk_encode_special_run."""

    def __init__(self, special, split, bpe):
        self.special, self.split, self.bpe = special, split, bpe
        self.op = K.FusedSpecialSplitBPE(special.op, split.op, bpe.op) if special is not None else K.FusedSplitBPE(split.op, bpe.op)

    def apply(self, kind, vals):
        assert kind == "strings"
        ins = list(vals[:5]) + ([vals[5]] if vals[5] is not None else [])
        if self.special is not None:
            return "ids", self.op.evaluate(ins + [self.special.pattern], _u8(self.split.pattern), self.bpe.consts)
        return "ids", self.op.evaluate(ins + [_u8(self.split.pattern)], self.bpe.consts)


class FusedEncodeDenseStep(Step):
    """... -> Truncate -> CombineSegments -> Padding as the sink of the encode's last pass: ovtk_encode_dense_enqueue / _finish (device tensors).
    Host arrays (a CPU-plugin style caller) take the two-call form instead -- ovtk_encode_run / ovtk_encode_special_run, then
    ovtk_encode_tail_run --, both of which stage host memory themselves."""

    def __init__(self, special, split, bpe, trunc, comb, pad):
        self.special, self.split, self.bpe, self.pad = special, split, bpe, pad
        self.op = K.FusedEncodeDense(split.op, bpe.op, special.op if special is not None else None,
                                     max_length=trunc.max_length if trunc is not None else 2**31 - 1, trunc_side=trunc.side if trunc is not None else "right",
                                     pad_right=pad.pad_right, pad_value=pad.pad_value, prefix=comb.prefix if comb is not None else (),
                                     suffix=comb.suffix if comb is not None else ())
        self.host_form = [FusedSplitBPEStep(special, split, bpe), FusedEncodeTailStep(trunc, comb, pad, lib=pad.op._lib)]

    def apply(self, kind, vals):
        assert kind == "strings"
        if not _is_torch(vals[4]) and not hasattr(self.bpe.op._lib, "ovtk_emulator_build"):
            for s in self.host_form:
                kind, vals = s.apply(kind, vals)
            return kind, vals
        ins = list(vals[:5]) + ([vals[5]] if vals[5] is not None else [])
        return "dense", self.op.evaluate(ins, _u8(self.split.pattern), self.bpe.consts,
                                         special_pattern=self.special.pattern if self.special is not None else None, target_dim=self.pad.target_dim)


class FusedSplitWordpieceStep(Step):
    """RegexSplit(\\s+, remove) -> RegexSplit(BERT delimiters, isolate) -> WordpieceTokenizer: ovtk_wordpiece_encode_run."""

    def __init__(self, ws, pu, wp):
        self.ws, self.pu, self.wp = ws, pu, wp
        self.op = K.FusedSplitWordpiece(ws.op, pu.op, wp.op)

    def apply(self, kind, vals):
        assert kind == "strings" and vals[5] is None
        return "ids", self.op.evaluate(list(vals[:5]), _u8(self.ws.pattern), _u8(self.pu.pattern), self.wp.consts)


class FusedEncodeTailStep(Step):
    """Truncate -> CombineSegments -> Padding in one kernel: ovtk_encode_tail_run (the ragged ids exist already: WordPiece, or a BPE chain
    whose split is none the span kernel scans)."""

    def __init__(self, trunc, comb, pad, lib=None):
        self.trunc, self.comb, self.pad = trunc, comb, pad
        self.op = K.FusedEncodeTail(max_length=trunc.max_length if trunc is not None else 2**31 - 1, trunc_side=trunc.side if trunc is not None else "right",
                                    pad_right=pad.pad_right, lib=lib)

    def apply(self, kind, vals):
        assert kind == "ids"
        b, e, ids = vals
        segs, main = [], 0
        if self.comb is not None and self.comb.prefix:
            segs.append((_like(ids, [0]), _like(ids, [len(self.comb.prefix)]), _like(ids, self.comb.prefix)))
            main = 1
        segs.append((b, e, ids))
        if self.comb is not None and self.comb.suffix:
            segs.append((_like(ids, [0]), _like(ids, [len(self.comb.suffix)]), _like(ids, self.comb.suffix)))
        out = self.op.evaluate(segs, np.arange(len(segs), dtype=np.int32), truncated=(main,) if self.trunc is not None else (), pad_value=self.pad.pad_value,
                               target_dim=self.pad.target_dim)
        return "dense", out[:2]


class FusedDetokenizeStep(Step):
    """VocabDecoder -> [ByteFallback] -> FuzeRagged: ovtk_detokenize_run."""

    def __init__(self, dec, byte_fallback):
        self.dec = dec
        self.op = K.FusedDetokenizer(dec.op, byte_fallback=byte_fallback)

    def apply(self, kind, vals):
        assert kind == "tokens"
        return "text", self.op.evaluate([vals[0]] + self.dec.vocab)


# ---------------------------------------------------------------------------------------------------------------- paired input
# The mirror of the reference's add_second_input (python/openvino_tokenizers/tokenizer_transformations.py:22-304).  Pipeline.run_pair
# concatenates the two string inputs and runs the front steps on all nA + nB rows; the pair steps below get the state
# ("pair_ids", [first begins, first ends, second begins, second ends, ids, second_empty]): the halves of the ragged ids, broadcast 1
# against n, over one ids tensor.  second_empty: the second input had no row -- its begins / ends are zeros, the constants the pair
# signature adds have length 0, max_length stays reduced (:103-120, :196-200).
def _signature_slots(pair_ids):
    """front / between / behind constants of a pair signature, and the positions of its two sequence entries."""
    seq = [k for k, v in enumerate(pair_ids) if v <= -1]
    return list(pair_ids[:seq[0]]), list(pair_ids[seq[0] + 1:seq[1]]), list(pair_ids[seq[1] + 1:]), seq


class PairTruncationStep(Step):
    """src/truncate.cpp:69-144, two inputs.  max_length: what Truncate receives (add_second_input has subtracted the added tokens)."""
    pair = True

    def __init__(self, max_length, side="right", mode="longest_first", lib=None):
        self.max_length, self.side, self.mode, self.op = int(max_length), side, mode, K.Truncate(lib=lib)

    def apply(self, kind, vals):
        assert kind == "pair_ids"
        fb, fe, sb, se, ids, second_empty = vals
        out = self.op.evaluate([fb, fe, ids, sb, se, ids, np.int32(self.max_length), self.side.encode(), self.mode.encode()])
        return "pair_ids", [out[0], out[1], out[3], out[4], ids, second_empty]


class PairCombineSegmentsStep(Step):
    """src/combine_segments.cpp:36-134 over a pair signature: a non-negative entry is one constant id, an entry <= -1 a sequence (the
    first such entry the first input); type_ids: one per entry; n_single: the entries the single signature had (the rest were added:
    their constants have length 0 when the second input is empty)."""
    pair = True

    def __init__(self, pair_ids, type_ids, n_single, lib=None):
        self.pair_ids, self.type_ids, self.n_single = [int(x) for x in pair_ids], [int(x) for x in type_ids], int(n_single)
        self.op = K.CombineSegments(lib=lib)

    def segments(self, vals):
        """-> [(begins, ends, data)] per entry and the indices of the two sequences."""
        fb, fe, sb, se, ids, second_empty = vals
        segs, seq = [], []
        for k, v in enumerate(self.pair_ids):
            if v <= -1:
                seq.append(k)
                segs.append((fb, fe, ids) if len(seq) == 1 else (sb, se, ids))
            else:
                segs.append((_like(ids, [0]), _like(ids, [0 if second_empty and k >= self.n_single else 1]), _like(ids, [v])))
        return segs, seq

    def apply(self, kind, vals):
        assert kind == "pair_ids"
        segs, _ = self.segments(vals)
        out = self.op.evaluate([x for s in segs for x in s] + [np.asarray(self.type_ids, np.int32)])
        return "typed_ids", [out[0], out[1], out[2], out[5]]


class PairPaddingStep(Step):
    """src/ragged_to_dense.cpp:70-174 three times: input_ids, attention_mask and token_type_ids."""
    pair = True

    def __init__(self, pad_value=0, type_pad_value=0, pad_right=True, target_dim=None, lib=None):
        self.pad_value, self.type_pad_value, self.pad_right, self.target_dim = int(pad_value), int(type_pad_value), bool(pad_right), target_dim
        self.op = K.RaggedToDense(pad_right=pad_right, lib=lib)

    def apply(self, kind, vals):
        assert kind == "typed_ids"
        b, e, ids, types = vals
        lens = e - b
        width = int(self.target_dim) if self.target_dim is not None else (int(lens.max()) if len(lens) else 0)
        dense, mask = self.op.evaluate([b, e, ids, np.int32(width), np.int32(self.pad_value)])
        tdense, _ = self.op.evaluate([b, e, types, np.int32(width), np.int32(self.type_pad_value)])
        return "dense", [dense, mask, tdense]


def add_second_input(steps, single_ids, pair_ids, pair_type_ids, trunc_mode="longest_first", type_pad_value=0):
    """The step list for paired input (the mirror of tokenizer_transformations.py:22-304); returns a new list, `steps` is untouched.
    single_ids / pair_ids: the post-processor's signatures in the reference's form -- [101, -1, 102] widened to [101, -1, 102, -2, 102]
    with pair_type_ids [0, 0, 0, 1, 1].  The checks of assert_and_get_postprocessor and run_on_model, each a ValueError."""
    single_ids, pair_ids, pair_type_ids = [int(x) for x in single_ids], [int(x) for x in pair_ids], [int(x) for x in pair_type_ids]
    if pair_ids[:len(single_ids)] != single_ids:
        raise ValueError("add_second_input: the pair signature must widen the single one")
    if sum(v <= -1 for v in pair_ids) != 2:
        raise ValueError("add_second_input: the pair signature must have exactly two sequence entries")
    if sum(v <= -1 for v in single_ids) != 1:
        raise ValueError("add_second_input: the single signature must have exactly one sequence entry")
    if len(pair_type_ids) != len(pair_ids):
        raise ValueError("add_second_input: one type id per entry of the pair signature")
    at = next((k for k, s in enumerate(steps) if isinstance(s, CombineSegmentsStep)), None)
    if at is None or at == 0 or not isinstance(steps[at - 1], TruncationStep):
        raise ValueError("add_second_input: a TruncationStep in front of the CombineSegmentsStep is needed")
    comb, trunc = steps[at], steps[at - 1]
    if comb.prefix + [-1] + comb.suffix != single_ids:
        raise ValueError("add_second_input: the single signature does not match the CombineSegmentsStep")
    lib = comb.op._lib
    num_added_tokens = len(pair_ids) - len(single_ids) - 1   # (:138-151)
    out = list(steps[:at - 1])
    out.append(PairTruncationStep(trunc.max_length - num_added_tokens, trunc.side, trunc_mode, lib=lib))
    out.append(PairCombineSegmentsStep(pair_ids, pair_type_ids, len(single_ids), lib=lib))
    for s in steps[at + 1:]:
        if isinstance(s, PaddingStep):
            s = PairPaddingStep(s.pad_value, type_pad_value, s.pad_right, s.target_dim, lib=lib)
        out.append(s)
    return out


def _pair_halves(b, e, ids, n_first, n_second):
    """The ragged ids of the nA + nB rows -> the pair state: the halves, broadcast 1 against n; any other mismatch raises."""
    if n_second and n_first != n_second and 1 not in (n_first, n_second):
        raise ValueError(f"run_pair: {n_first} first rows against {n_second} second ones (equal counts, or 1 against n)")
    rows = max(n_first, n_second)
    rep = (lambda x, k: x.repeat(k)) if _is_torch(b) else (lambda x, k: np.repeat(x, k))
    fb, fe = b[:n_first], e[:n_first]
    if n_first == 1 and rows > 1:
        fb, fe = rep(fb, rows), rep(fe, rows)
    if n_second == 0:   # (:116-120: zeroed)
        sb = se = _like(ids, np.zeros(rows, np.int32))
    else:
        sb, se = b[n_first:n_first + n_second], e[n_first:n_first + n_second]
        if n_second == 1 and rows > 1:
            sb, se = rep(sb, rows), rep(se, rows)
    return [fb, fe, sb, se, ids, n_second == 0]


class _FusedPairStep(Step):
    """front of the graph + PairTruncation + PairCombineSegments + PairPadding.  Device tensors with nA == nB: the one call
    (self.op); broadcast, an empty second input and host arrays: the two-call form -- the fused encode on all rows (self.encode), then
    ovtk_encode_tail_run over the halves (as FusedEncodeDenseStep.host_form)."""
    pair = True
    two_call = False   # True: the two-call form whatever the inputs are (tools/ops_timing.py --only-pair times it beside the one call)

    def _init_tail(self, trunc, comb, pad, lib):
        self.trunc, self.comb, self.pad, self.lib = trunc, comb, pad, lib
        front, between, behind, _ = _signature_slots(comb.pair_ids)
        seq = [k for k, v in enumerate(comb.pair_ids) if v <= -1]
        t = comb.type_ids
        self.tail_args = dict(max_length=trunc.max_length, trunc_side=trunc.side, trunc_mode=trunc.mode, pad_right=pad.pad_right, pad_value=pad.pad_value,
                              type_pad_value=pad.type_pad_value, front=front, between=between, behind=behind,
                              type_ids=[t[0] if front else 0, t[seq[0]], t[seq[0] + 1] if between else 0, t[seq[1]], t[seq[1] + 1] if behind else 0])
        self.tail = K.FusedEncodeTail(trunc.max_length, trunc.side, trunc.mode, pad.pad_right, lib=lib)

    def one_call(self, vals, n_first):
        raise NotImplementedError

    def apply_pair(self, vals, n_first, n_second):
        device = _is_torch(vals[4]) or hasattr(self.lib, "ovtk_emulator_build")
        if device and n_first == n_second and not self.two_call:
            return "dense", self.one_call(vals, n_first)
        _, (b, e, ids) = self.encode.apply("strings", vals)
        if len(b) != n_first + n_second:   # (no text at all: the ragged tensor's one-row quirk, regex_split.cpp:129-143 -- every row is empty)
            b = e = _like(ids, np.zeros(n_first + n_second, np.int32))
        state = _pair_halves(b, e, ids, n_first, n_second)
        segs, seq = self.comb.segments(state)
        return "dense", self.tail.evaluate(segs, self.comb.type_ids, truncated=tuple(seq), pad_value=self.pad.pad_value,
                                           type_pad_value=self.pad.type_pad_value, target_dim=self.pad.target_dim)


class FusedPairEncodeDenseStep(_FusedPairStep):
    """[SpecialTokensSplit] RegexSplit BPETokenizer + the pair tail: ovtk_encode_pair_dense_enqueue / _finish."""

    def __init__(self, special, split, bpe, trunc, comb, pad):
        self.special, self.split, self.bpe = special, split, bpe
        self._init_tail(trunc, comb, pad, bpe.op._lib)
        self.encode = FusedSplitBPEStep(special, split, bpe)
        self.op = K.FusedPairEncodeDense(split.op, bpe.op, special.op if special is not None else None, **self.tail_args)

    def one_call(self, vals, n_first):
        ins = list(vals[:5]) + ([vals[5]] if vals[5] is not None else [])
        return self.op.evaluate(ins, n_first, _u8(self.split.pattern), self.bpe.consts,
                                special_pattern=self.special.pattern if self.special is not None else None, target_dim=self.pad.target_dim)


class FusedPairWordpieceDenseStep(_FusedPairStep):
    """The BERT split + WordpieceTokenizer + the pair tail: ovtk_wordpiece_encode_pair_dense_enqueue / ovtk_encode_pair_dense_finish."""

    def __init__(self, ws, pu, wp, trunc, comb, pad):
        self.ws, self.pu, self.wp = ws, pu, wp
        self._init_tail(trunc, comb, pad, wp.op._lib)
        self.encode = FusedSplitWordpieceStep(ws, pu, wp)
        self.op = K.FusedPairWordpieceDense(ws.op, pu.op, wp.op, **self.tail_args)

    def one_call(self, vals, n_first):
        return self.op.evaluate(list(vals[:5]), n_first, _u8(self.ws.pattern), _u8(self.pu.pattern), self.wp.consts, target_dim=self.pad.target_dim)


def _pair_tail(steps, i):
    """PairTruncation PairCombineSegments PairPadding at steps[i:] that the one call covers (at most four constants in a slot, one type id
    per slot) -> the three steps or None."""
    if i + 2 >= len(steps) or not (isinstance(steps[i], PairTruncationStep) and isinstance(steps[i + 1], PairCombineSegmentsStep) and
                                   isinstance(steps[i + 2], PairPaddingStep)):
        return None
    comb = steps[i + 1]
    front, between, behind, seq = _signature_slots(comb.pair_ids)
    if max(len(front), len(between), len(behind)) > 4 or seq[0] >= comb.n_single or seq[1] < comb.n_single:
        return None
    t = comb.type_ids
    for lo, hi in ((0, seq[0]), (seq[0] + 1, seq[1]), (seq[1] + 1, len(t))):
        if len(set(t[lo:hi])) > 1:
            return None
    return steps[i], comb, steps[i + 2]


# ---------------------------------------------------------------------------------------------------------------- the rewrite
def _span_pattern(step):
    """A split the fused encode has a scanner for (api_encode.cpp ovtk_regex_split_create: pattern equality picks it): isolate, no invert, no
    max_splits.  Any other RegexSplit is still fusable with BPETokenizer (the compiled DFA runs inside the call), but only ONE split."""
    return isinstance(step, RegexSplitStep) and step.behaviour in ("isolate", "contiguous") and not step.invert and step.max_splits == -1


# the converter's two patterns of the BERT pre-tokenizer (tokenizer_pipeline.py:392-431)
BERT_WS = r"\s+"
BERT_PUNCT = "|".join([r"[!-/]", r"[:-@]", r"[\[-`]", r"[{-~]", r"[\p{P}]", r"[\x{4E00}-\x{9FFF}]", r"[\x{3400}-\x{4DBF}]", r"[\x{20000}-\x{2A6DF}]",
                       r"[\x{2A700}-\x{2B73F}]", r"[\x{2B740}-\x{2B81F}]", r"[\x{2B820}-\x{2CEAF}]", r"[\x{F900}-\x{FAFF}]", r"[\x{2F800}-\x{2FA1F}]"])


def _is_bert_split(a, b):
    return (isinstance(a, RegexSplitStep) and isinstance(b, RegexSplitStep) and a.pattern == BERT_WS and a.behaviour == "remove" and not a.invert and
            b.pattern == BERT_PUNCT and b.behaviour == "isolate" and not b.invert and a.max_splits == -1 and b.max_splits == -1)


def _tail(steps, i):
    """[Truncation] [CombineSegments with at most four constant ids each side] Padding at steps[i:] -> (trunc, comb, pad, next index) or None."""
    trunc = comb = None
    j = i
    if j < len(steps) and isinstance(steps[j], TruncationStep):
        trunc, j = steps[j], j + 1
    if j < len(steps) and isinstance(steps[j], CombineSegmentsStep):
        if len(steps[j].prefix) > 4 or len(steps[j].suffix) > 4:
            return None
        comb, j = steps[j], j + 1
    if j < len(steps) and isinstance(steps[j], PaddingStep):
        return trunc, comb, steps[j], j + 1
    return None


def fuse(steps):
    """The list with every recognised sub-chain replaced by its fused step (module docstring); the input list is not modified."""
    out, i, n = [], 0, len(steps)
    while i < n:
        s = steps[i]
        # ---- [SpecialTokensSplit] RegexSplit BPETokenizer [tail]
        j = i
        special = None
        if isinstance(s, SpecialTokensSplitStep) and j + 1 < n:
            special, j = s, j + 1
        if j + 1 < n and isinstance(steps[j], RegexSplitStep) and isinstance(steps[j + 1], BPETokenizationStep) and _span_pattern(steps[j]):
            split, bpe = steps[j], steps[j + 1]
            pt = _pair_tail(steps, j + 2)
            if pt is not None:
                out.append(FusedPairEncodeDenseStep(special, split, bpe, *pt))
                i = j + 5
                continue
            t = _tail(steps, j + 2)
            if t is not None:
                out.append(FusedEncodeDenseStep(special, split, bpe, *t[:3]))
                i = t[3]
            else:
                out.append(FusedSplitBPEStep(special, split, bpe))
                i = j + 2
            continue
        # ---- the BERT pre-tokenizer + WordPiece
        if i + 2 < n and _is_bert_split(steps[i], steps[i + 1]) and isinstance(steps[i + 2], WordPieceTokenizationStep):
            pt = _pair_tail(steps, i + 3)
            if pt is not None:
                out.append(FusedPairWordpieceDenseStep(steps[i], steps[i + 1], steps[i + 2], *pt))
                i += 6
                continue
            out.append(FusedSplitWordpieceStep(steps[i], steps[i + 1], steps[i + 2]))
            i += 3
            continue
        # ---- a tail on ragged ids that exist
        if isinstance(s, (TruncationStep, CombineSegmentsStep, PaddingStep)):
            t = _tail(steps, i)
            if t is not None and (t[0] is not None or t[1] is not None):
                out.append(FusedEncodeTailStep(t[0], t[1], t[2], lib=t[2].op._lib))
                i = t[3]
                continue
        # ---- the detokenizer
        if isinstance(s, VocabDecoderStep):
            j = i + 1
            bf = j < n and isinstance(steps[j], ByteFallbackStep)
            if bf:
                j += 1
            if j < n and isinstance(steps[j], FuseStep):
                out.append(FusedDetokenizeStep(s, bf))
                i = j + 1
                continue
        out.append(s)
        i += 1
    return out


class Pipeline:
    """A chain of steps.  run(kind, values): the state a chain starts from -- ("strings", [ragged_begins, ragged_ends, begins, ends, chars, skips
    or None]) for a tokenizer, ("tokens", [ids[B, S]]) for a detokenizer -- through every step; returns the last state's values."""

    def __init__(self, steps):
        self.steps = list(steps)

    def fused(self):
        return Pipeline(fuse(self.steps))

    def run(self, kind, values):
        vals = list(values)
        for s in self.steps:
            kind, vals = s.apply(kind, vals)
        return vals

    def run_pair(self, first, second):
        """Paired input (a list made by add_second_input): first / second are [begins, ends, chars] each, numpy or torch.  The two inputs
        are concatenated, the front steps run on the nA + nB rows, the pair steps on the halves (1 against n is broadcast; an empty
        second input gives what the reference gives).  Returns [input_ids, attention_mask, token_type_ids]."""
        fb, fe, fc = first
        sb, se, sc = second
        n_first, n_second = len(fb), len(sb)
        if n_second and n_first != n_second and 1 not in (n_first, n_second):
            raise ValueError(f"run_pair: {n_first} first rows against {n_second} second ones (equal counts, or 1 against n)")
        if _is_torch(fc):
            import torch
            sb, se, sc = (torch.as_tensor(x, device=fc.device) for x in (sb, se, sc))
            cat = torch.cat
            rows = torch.arange(n_first + n_second + 1, dtype=torch.int32, device=fc.device)
        else:
            sb, se, sc = (np.asarray(x.cpu() if _is_torch(x) else x) for x in (sb, se, sc))
            cat = np.concatenate
            rows = np.arange(n_first + n_second + 1, dtype=np.int32)
        off = len(fc)
        kind, vals = "strings", [rows[:-1], rows[1:], cat([fb, sb + off]), cat([fe, se + off]), cat([fc, sc]), None]
        for s in self.steps:
            if getattr(s, "pair", False) and kind == "strings":
                kind, vals = s.apply_pair(vals, n_first, n_second)
            elif getattr(s, "pair", False) and kind == "ids":
                b, e, ids = vals
                if len(b) != n_first + n_second:   # (no text at all: the ragged tensor's one-row quirk -- every row is empty)
                    b = e = _like(ids, np.zeros(n_first + n_second, np.int32))
                kind, vals = s.apply("pair_ids", _pair_halves(b, e, ids, n_first, n_second))
            else:
                kind, vals = s.apply(kind, vals)
        return vals
