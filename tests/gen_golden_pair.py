"""Generates tests/golden/golden_pair_bert_small.npz: sentence pairs through HF `tokenizers`, the one reference that is independent of
this project's oracle.  Run by hand where `tokenizers` is installed: python tests/gen_golden_pair.py

The BERT-small tokenizer of tests/golden/tok_bert_small.hf.json with the template `[CLS] A [SEP] B [SEP]` (type ids 0 0 0 1 1),
`longest_first` truncation to MAX_LENGTH ids in both directions, and padding to the longest row.  The texts are word runs cut out of
the texts of golden_wordpiece_bert_small.npz.

One documented difference (tests/test_truncate_combine.py:30-45): on a tie over an odd budget -- first == second ids, together more than
the MAX_LENGTH - 3 that Truncate receives -- the reference gives the odd id to the first sequence, HF to the second.  Those rows are
left out of the comparison with HF by tests/test_pair_pipeline.py and checked against the reference's rule there; this generator makes
sure that at most 5 % of the rows are such rows and that at least 20 are.
"""
import json
from pathlib import Path

import numpy as np

G = Path(__file__).parent / "golden"
MAX_LENGTH = 20     # HF's: the whole row.  Truncate receives MAX_LENGTH - 3 = 17 (odd)
N_ROWS = 1200
TIE_EVERY = 48      # every 48th row is the same text twice


def pair_texts():
    z = np.load(G / "golden_wordpiece_bert_small.npz")
    raw = z["chars"].tobytes()
    words = []
    for b, e in zip(z["begins"], z["ends"]):
        words.append(raw[b:e].decode("utf-8").split())
    words = [w for w in words if len(w) >= 2 and max(len(x) for x in w) < 40]
    rng = np.random.default_rng(2025)

    def run(short):
        w = words[int(rng.integers(len(words)))]
        k = int(rng.integers(1, 4)) if short else int(rng.integers(1, 40))
        at = int(rng.integers(0, max(1, len(w) - k + 1)))
        return " ".join(w[at:at + k])
    first, second = [], []
    for i in range(N_ROWS):
        a, b = run(rng.integers(4) == 0), run(rng.integers(4) == 0)
        if i % TIE_EVERY == 0:
            a = b = " ".join((run(False) + " " + run(False)).split()[:30])
        first.append(a)
        second.append(b)
    first[1], second[2] = "", ""
    first[3] = second[3] = ""
    return first, second


def pack(strings):
    raw = [s.encode("utf-8") for s in strings]
    lens = np.array([len(r) for r in raw], np.int64)
    ends = np.cumsum(lens).astype(np.int32)
    return (ends - lens).astype(np.int32), ends, np.frombuffer(b"".join(raw), np.uint8)


def main():
    from tokenizers import Tokenizer
    from tokenizers.processors import TemplateProcessing
    tok = Tokenizer.from_file(str(G / "tok_bert_small.hf.json"))
    cls, sep, pad = tok.token_to_id("[CLS]"), tok.token_to_id("[SEP]"), tok.token_to_id("[PAD]")
    tok.post_processor = TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1", special_tokens=[("[CLS]", cls), ("[SEP]", sep)])
    first, second = pair_texts()
    la = np.array([len(tok.encode(s, add_special_tokens=False).ids) for s in first])
    lb = np.array([len(tok.encode(s, add_special_tokens=False).ids) for s in second])
    budget = MAX_LENGTH - 3
    assert budget % 2 == 1
    ties = (la == lb) & (la + lb > budget)
    assert ties.sum() >= 20, f"{ties.sum()} tie rows: at least 20 are needed"
    assert ties.sum() <= 0.05 * N_ROWS, f"{ties.sum()} tie rows of {N_ROWS}: at most 5 % may be left out of the comparison"
    out = dict(zip(("first_begins", "first_ends", "first_chars"), pack(first)))
    out.update(zip(("second_begins", "second_ends", "second_chars"), pack(second)))
    tok.enable_padding(pad_id=pad, pad_token="[PAD]", pad_type_id=0)
    for side in ("right", "left"):
        tok.enable_truncation(max_length=MAX_LENGTH, strategy="longest_first", direction=side)
        enc = tok.encode_batch(list(zip(first, second)))
        out[f"ids_{side}"] = np.array([e.ids for e in enc], np.int32)
        out[f"type_ids_{side}"] = np.array([e.type_ids for e in enc], np.int32)
        out[f"mask_{side}"] = np.array([e.attention_mask for e in enc], np.uint8)
    out["meta"] = np.frombuffer(json.dumps(dict(source="tokenizers " + __import__("tokenizers").__version__, tokenizer="tok_bert_small.hf.json",
                                                max_length=MAX_LENGTH, cls=cls, sep=sep, pad=pad, ties=int(ties.sum()))).encode(), np.uint8)
    path = G / "golden_pair_bert_small.npz"
    np.savez_compressed(path, **out)
    assert path.stat().st_size < 1_000_000
    print(path.name, N_ROWS, "pairs,", int(ties.sum()), "tie rows,", path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
