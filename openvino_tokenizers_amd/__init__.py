"""MI355X-native tokenizer hot path of openvino_tokenizers (RegexSplit, BPETokenizer, WordpieceTokenizer,
VocabEncoder, RaggedToDense, VocabDecoder, ByteFallback, FuzeRagged, plus SpecialTokensSplit, UTF8Validate, CharsMapNormalization,
Truncate and CombineSegments either side of it, and the TensorFlow front end's StringToHashBucket, EqualStr and RaggedToRagged, the old byte-level graphs' BytesToChars / CharsToBytes and the ONNX front end's ContribStringSplit / ContribStringJoin) behind the reference's op interface.

Compute happens only in csrc/build/libovtk_amd.so (hand-written HIP for gfx950) through the C ABI of
include/ovtk_amd.h; see DESIGN.md and INTEGRATION.md.
"""
from ._lib import OvtkError, load  # noqa: F401
from .ops import (BPETokenizer, ByteFallback, BytesToChars, CaseFold, CharsMapNormalization, CharsToBytes, CombineSegments, ContribStringJoin, ContribStringSplit, EqualStr, FusedDetokenizer, FusedEncodeDense, FusedEncodeTail, FusedPairEncodeDense, FusedPairWordpieceDense, FusedSpecialSplitBPE, FusedSplitBPE, FusedSplitWordpiece, FuzeRagged, NormalizeUnicode, RaggedTensorPack, RaggedToDense, RaggedToRagged, RaggedToSparse,  # noqa: F401
                  RegexNormalization, RegexSplit, SentencepieceDetokenizer, SentencepieceStreamDetokenizer, SentencepieceTokenizer, SpecialTokensSplit, StringTensorPack, StringTensorUnpack, StringToHashBucket, TrieTokenizer, Truncate, UnigramTokenizer, UTF8Validate, VocabDecoder, VocabEncoder, WordpieceTokenizer)
