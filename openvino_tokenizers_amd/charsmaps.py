"""Precompiled charsmaps for CharsMapNormalization / NormalizeUnicode / CaseFold.

This library ships no tables (the reference generates its precompiled_charsmap.hpp when it is built).  Where the `sentencepiece`
package is installed its own tables can be taken from it; nothing here is imported when the package is."""
from __future__ import annotations


def from_sentencepiece(rule_name: str) -> bytes:
    """The precompiled charsmap of one of sentencepiece's built-in rules (nfkc, nmt_nfkc, nfkc_cf, nmt_nfkc_cf, identity): the blob
    its normalizer_spec carries.  Raises ImportError without the package."""
    import sentencepiece as spm
    from sentencepiece import sentencepiece_model_pb2 as pb

    spec = pb.NormalizerSpec()
    spec.ParseFromString(spm.SentencePieceNormalizer(rule_name=rule_name).serialized_normalizer_spec())
    return bytes(spec.precompiled_charsmap)
