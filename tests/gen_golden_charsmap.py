"""Writes tests/golden/golden_charsmap.npz: what sentencepiece's own normalizer (SentencePieceNormalizer, the C++ class the reference's
CharsMapNormalization / NormalizeUnicode / CaseFold call) makes of 3 000 strings under three charsmaps and all eight flag combinations.

    python -m tests.gen_golden_charsmap          (needs the `sentencepiece` package; the tests do not)

Contents
  blob_nfkc, blob_nmt_nfkc_cf   sentencepiece's precompiled charsmaps of those rule names
  blob_small                    a map built with norm_map=: replacements that are empty, all spaces, space-leading, space-trailing
  in_ends, in_chars             the strings, back to back (at most 512 bytes each)
  out_lens [n, 3, 8] u16        bytes of the output of string i under blob j (the order above) and flags f
  out_chars                     those outputs back to back, string-major, then blob, then flags
  flags f = add_dummy_prefix | remove_extra_whitespaces << 1 | escape_whitespaces << 2
The generator also checks tests/charsmap_ref.py against every output before it writes.
"""
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent / "golden" / "golden_charsmap.npz"
BLOBS = ("nfkc", "nmt_nfkc_cf", "small")
SMALL_MAP = {"ab": "", "q": "  ", "xy": " X", "zz": "Z ", "ét": "e t", "Q": "", "w": " ", "あい": " う ", "kk": "  k"}
N_STRINGS = 3000


def flags_of(f):
    return dict(add_dummy_prefix=bool(f & 1), remove_extra_whitespaces=bool(f & 2), escape_whitespaces=bool(f & 4))


def make_strings(rng, n):
    ascii_words = [b"the", b"quick", b"brown", b"fox", b"ab", b"q", b"xy", b"zz", b"kk", b"w", b"Q", b"HELLO", b"World", b"zzab", b"abab", b"a", b"I"]
    wide = ["ｈｅｌｌｏ", "ﬁ", "①", "½", "㎥", "Å", "ＡＢ", "Ǆ", "ẞ", "İ"]
    multi = ["é", "ä", "ﾊﾟ", "ｶﾞ", "가", "한", "ố", "آ", "ét",
             "あい", "क़", "ড়"]
    cjk = ["中文", "한국어", "あいう", "カタカナ", "\U0001f600", "\U00020000"]
    odd_space = ["­", "​", "　", " ", "▁", "▁▁", " ", "﻿", "\t", "\n", "\x00", "‍", " "]
    bad = [b"\xc0\x80", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xe3\x81", b"\xf5\x80\x80\x80", b"\xf4\x90\x80\x80", b"\x80", b"\xbf\xbf",
           b"\xff", b"\xf0\x9f\x98", b"\xc2", b"\xe2\x96", b"\xf8\x88\x80\x80\x80", b"\xc1\xbf", b"\xf0\x80\x80\x80", b"\xef\xbf\xbd"]
    classes = [(ascii_words, 8), ([b" ", b"  ", b"   "], 6), (wide, 2), (multi, 2), (cjk, 2), (odd_space, 2), (bad, 1)]
    pool, weight = [], []
    for items, w in classes:
        for it in items:
            pool.append(it if isinstance(it, bytes) else it.encode("utf-8"))
            weight.append(w / len(items))
    weight = np.asarray(weight) / np.sum(weight)
    out = [b"", b" ", b"   ", "▁".encode("utf-8"), b"q", b"ab", b" ab ", b"w w", "a ▁".encode("utf-8"), b"\xe3\x81"]
    while len(out) < n:
        k = int(rng.integers(1, 5)) if rng.random() < 0.2 else int(rng.integers(4, 16)) if rng.random() < 0.9 else int(rng.integers(40, 120))
        s = b"".join(pool[i] for i in rng.choice(len(pool), size=k, p=weight))
        if rng.random() < 0.05 and len(s) > 2:   # a cut anywhere: sequences that the end of the string cuts off
            s = s[:int(rng.integers(1, len(s)))]
        out.append(s[:512])
    return out


def main():
    import sentencepiece as spm
    from sentencepiece import sentencepiece_model_pb2 as pb

    from tests.charsmap_ref import CharsMapRef

    def normalizer(name, **kw):
        return spm.SentencePieceNormalizer(norm_map=list(SMALL_MAP.items()), **kw) if name == "small" else spm.SentencePieceNormalizer(rule_name=name, **kw)

    def blob_of(name):
        spec = pb.NormalizerSpec()
        spec.ParseFromString(normalizer(name).serialized_normalizer_spec())
        return bytes(spec.precompiled_charsmap)

    rng = np.random.default_rng(20260107)
    strings = make_strings(rng, N_STRINGS)
    blobs = {name: blob_of(name) for name in BLOBS}
    lens = np.zeros((len(strings), len(BLOBS), 8), np.uint16)
    outs = [[[None] * 8 for _ in BLOBS] for _ in strings]
    for j, name in enumerate(BLOBS):
        for f in range(8):
            sp, ref = normalizer(name, **flags_of(f)), CharsMapRef(blobs[name], **flags_of(f))
            for i, s in enumerate(strings):
                got = sp.normalize(s)
                got = got.encode("utf-8") if isinstance(got, str) else bytes(got)
                assert ref.normalize(s) == got, (name, f, s, got, ref.normalize(s))
                outs[i][j][f] = got
                lens[i, j, f] = len(got)
    chars = b"".join(o for per_s in outs for per_b in per_s for o in per_b)
    in_ends = np.cumsum([len(s) for s in strings]).astype(np.int32)
    np.savez_compressed(OUT, in_ends=in_ends, in_chars=np.frombuffer(b"".join(strings), np.uint8), out_lens=lens,
                        out_chars=np.frombuffer(chars, np.uint8), **{"blob_" + k: np.frombuffer(v, np.uint8) for k, v in blobs.items()})
    print(f"{OUT.name}: {OUT.stat().st_size} bytes, {len(strings)} strings, {in_ends[-1]} input bytes, {len(chars)} output bytes")


if __name__ == "__main__":
    main()
