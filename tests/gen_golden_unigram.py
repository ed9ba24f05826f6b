"""Generates tests/golden/golden_unigram_small.npz: a generated Unigram vocabulary, strings, and the ids Hugging Face's
`tokenizers.models.Unigram` gives for them -- the external pin of tests/unigram_ref.py (tests/test_unigram.py::test_restatement_matches_hf).

HF adds scores in float64, the reference (and the restatement, and the kernel) in float32.  So that both give the same path, every
score is a multiple of 1/64 in (-32, 0] and no string is longer than 512 bytes: a path's sum is then below 2^15 in magnitude with 6
fraction bits, exact in either format (the unknown score, min - 10, is such a multiple too).  Text and vocabulary are valid UTF-8 (HF
works on `str`); unknown characters are drawn from an alphabet the vocabulary does not cover.

Also searches float32 for a minimum score m where float32(m) - float32(10) and float32(float64(m) - 10.0) differ (the unknown score's
"one rounding", src/unigram_tokenizer.cpp:157) and prints what it finds: nothing -- a float32 subtraction is itself one rounding of the
exact difference, and the float64 difference of two float32 values that far apart in exponent is either exact or off by less than the
float32 rounding can see.

Run here (needs `tokenizers`, nothing is downloaded); the .npz is committed:    python -m tests.gen_golden_unigram
"""
from pathlib import Path

import numpy as np

G = Path(__file__).resolve().parent / "golden"

KNOWN = list("abcdefghij ") + ["é", "ü", "中", "文", "▁", "😀"]
UNKNOWN = list("xyz") + ["ß", "日", "🙂"]
UNK_ID = 3


def make_vocab(rng, n=400):
    vocab = list(KNOWN[:3]) + ["<unk>"] + list(KNOWN[3:])
    seen = set(vocab)
    while len(vocab) < n:
        w = "".join(rng.choice(KNOWN, size=int(rng.integers(2, 7))).tolist())
        if w not in seen:
            seen.add(w)
            vocab.append(w)
    scores = -(rng.integers(0, 32 * 64, len(vocab)).astype(np.float64)) / 64.0
    return vocab, scores.astype(np.float32)


def make_strings(rng, n=3000):
    out = []
    for i in range(n):
        with_unknown = rng.random() < 0.3
        alphabet = KNOWN + (UNKNOWN if with_unknown else [])
        s = ""
        target = int(rng.integers(0, 120)) if i % 10 else int(rng.integers(300, 500))
        while len(s.encode()) < target:
            s += str(rng.choice(alphabet))
        while len(s.encode()) > 512:
            s = s[:-1]
        out.append(s)
    out[7] = ""
    return out


def unk_score_search(n=2_000_000, seed=3):
    """float32 minima m with float32(m) - float32(10) != float32(float64(m) - 10.0): random bit patterns and the neighbourhoods where a
    double rounding could show (|m| around 2^-21 .. 2^-25, around 10, around the exponent changes of the difference)."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    m = bits.view(np.float32)
    near = np.concatenate([np.float32(c) * (1 + np.arange(-4096, 4096, dtype=np.float32) * np.float32(2.0**-23))
                           for c in (2.0**-20, 2.0**-21, 2.0**-22, 2.0**-23, 2.0**-24, 2.0**-25, 2.0, 6.0, 10.0, 14.0, 18.0, 26.0)])
    m = np.concatenate([m, near, -near])
    m = m[np.isfinite(m)]
    one = m - np.float32(10.0)
    two = (m.astype(np.float64) - 10.0).astype(np.float32)
    return m[one != two]


def main():
    from tokenizers import Tokenizer, models

    rng = np.random.default_rng(20240611)
    vocab, scores = make_vocab(rng)
    strings = make_strings(rng)
    tok = Tokenizer(models.Unigram([(w, float(s)) for w, s in zip(vocab, scores)], UNK_ID, False))
    rows = [tok.encode(s, add_special_tokens=False).ids for s in strings]
    words = [w.encode() for w in vocab]
    data = [s.encode() for s in strings]
    assert max(map(len, data)) <= 512
    np.savez_compressed(G / "golden_unigram_small.npz",
                        vocab_ends=np.cumsum([len(w) for w in words]).astype(np.int32), vocab_chars=np.frombuffer(b"".join(words), np.uint8),
                        scores=scores, unk_id=np.int32(UNK_ID),
                        ends=np.cumsum([len(s) for s in data]).astype(np.int32), chars=np.frombuffer(b"".join(data), np.uint8),
                        id_ends=np.cumsum([len(r) for r in rows]).astype(np.int32), ids=np.asarray([i for r in rows for i in r], np.int32))
    with_unk = sum(UNK_ID in r for r in rows)
    print(f"{len(strings)} strings, {len(vocab)} tokens, {with_unk} rows with the unknown id, {sum(map(len, rows))} ids")
    diff = unk_score_search()
    print(f"unk_score search: {len(diff)} float32 minima where one and two roundings differ" + (f", e.g. {diff[:4]!r}" if len(diff) else ""))


if __name__ == "__main__":
    main()
