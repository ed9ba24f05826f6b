"""Writes tests/golden/spm_bpe_{bytes,unk,edit}.model, spm_bpe_refuse_{unused,tie}.model and golden_sentencepiece_bpe.npz: small BPE
models trained in-process by the `sentencepiece` package (num_threads=1: deterministic) on the syllable corpus of
gen_golden_sentencepiece.py, and the package's ids for a fixed list of sentences -- plain, add_bos, add_eos, both, reverse alone.
Nothing is downloaded.  Run from the repository root:

    python tests/gen_golden_sentencepiece_bpe.py

restate() below is bpe::Model::Encode and the post-processing of SentencePieceProcessor::Encode in plain Python, the rules the GPU
path (csrc/sp_bpe_kernels.hpp) implements.  THE PACKAGE IS THE AUTHORITY: the script asserts that restate() equals
SentencePieceProcessor.encode on every row of every model and option, and that the goldens reach what they are there for (the
counter-example to merging all local maxima, the chain, "▁▁", the inner-"▁" piece that switches the cut rule off, segments longer
than two waves, unknown runs, byte fallback); it fails otherwise.
"""
import io
import random
import sys
from pathlib import Path

import numpy as np
import sentencepiece as spm
from sentencepiece import sentencepiece_model_pb2 as pb

sys.path.insert(0, str(Path(__file__).resolve().parent))
from gen_golden_sentencepiece import OPTIONS, corpus, sentences, words   # noqa: E402

G = Path(__file__).resolve().parent / "golden"
MODELS = ("bytes", "unk", "edit")
T = pb.ModelProto.SentencePiece
SP = "▁"
WAVE = 64   # what one wave form of the merge kernel holds, in normalized bytes


def train(lines, **kw):
    buf = io.BytesIO()
    spm.SentencePieceTrainer.train(sentence_iterator=iter(lines), model_writer=buf, model_type="bpe", num_threads=1,
                                   hard_vocab_limit=False, minloglevel=2, **kw)
    return buf.getvalue()


def edited(model_bytes):
    """`bytes` with, at scores no other piece has: the ab / abc / cd counter-example on ξ ψ ω χ, a chain a, aa, aaaa, aaaaaaaa,
    the piece ▁▁, and a piece with an inner ▁ behind a letter (no position of a sentence is provably a cut any more)."""
    m = pb.ModelProto()
    m.ParseFromString(model_bytes)
    by_name = {p.piece: i for i, p in enumerate(m.pieces)}

    def put(piece, score):
        if piece in by_name:
            p = m.pieces[by_name[piece]]
            p.score, p.type = score, T.NORMAL
        else:
            by_name[piece] = len(m.pieces)
            m.pieces.add(piece=piece, score=score, type=T.NORMAL)

    for k, ch in enumerate("ξψωχ"):
        put(ch, -2000.25 - k)
    put("ξψ", -1.25)
    put("ξψω", -2.25)
    put("ωχ", -3.25)
    put("a", -1000.25)
    put("aa", -4.25)
    put("aaaa", -5.25)
    put("aaaaaaaa", -6.25)
    put(SP + SP, -7.25)
    put("ξ" + SP, -0.25)   # ξ + ▁, ahead of every trained merge
    scores = [np.float32(p.score) for p in m.pieces if p.type == T.NORMAL and len(p.piece) >= 2]
    assert len(scores) == len(set(scores)), "the edited model has tied scores"
    return m.SerializeToString()


def refused(model_bytes):
    m = pb.ModelProto()
    m.ParseFromString(model_bytes)
    multi = [p for p in m.pieces if p.type == T.NORMAL and len(p.piece) >= 2]
    multi[5].type = T.UNUSED
    unused = m.SerializeToString()
    m.ParseFromString(model_bytes)
    multi = [p for p in m.pieces if p.type == T.NORMAL and len(p.piece) >= 2]
    multi[7].score = multi[3].score
    return unused, m.SerializeToString()


# ------------------------------------------------------------------------------------------------ the rules, restated
def char_len(lead):
    return 1 if lead < 0xC0 else 2 if lead < 0xE0 else 3 if lead < 0xF0 else 4


class Restated:
    def __init__(self, model_bytes):
        m = pb.ModelProto()
        m.ParseFromString(model_bytes)
        self.sp = spm.SentencePieceProcessor(model_proto=model_bytes)
        self.id_of = {p.piece.encode(): i for i, p in enumerate(m.pieces)}
        self.normal = {p.piece.encode(): (np.float32(p.score), i) for i, p in enumerate(m.pieces) if p.type == T.NORMAL}
        self.unk = self.sp.unk_id()
        self.byte_fallback = m.trainer_spec.byte_fallback
        self.byte_id = [self.id_of.get(b"<0x%02X>" % v, self.unk) for v in range(256)]
        self.bos, self.eos = self.sp.bos_id(), self.sp.eos_id()

    def pieces(self, text):
        """bpe::Model::Encode over normalized bytes -> the remaining symbols."""
        syms, k = [], 0
        while k < len(text):
            n = min(char_len(text[k]), len(text) - k)
            syms.append(text[k:k + n])
            k += n
        while True:
            best = None
            for i in range(len(syms) - 1):
                hit = self.normal.get(syms[i] + syms[i + 1])
                if hit is not None and (best is None or hit[0] > best[0]):   # strict: among equal scores the leftmost stays
                    best = (hit[0], i)
            if best is None:
                return syms
            i = best[1]
            syms[i:i + 2] = [syms[i] + syms[i + 1]]

    def encode(self, row, add_bos=False, add_eos=False, reverse=False):
        text = self.sp.normalize(row)
        text = text.encode() if isinstance(text, str) else text
        ids, prev_unk = [], False
        for s in self.pieces(text):
            i = self.id_of.get(s, self.unk)
            unk = i == self.unk
            if unk and self.byte_fallback:
                ids += [self.byte_id[b] for b in s]
            elif not (unk and prev_unk):
                ids.append(i)
            prev_unk = unk
        if reverse:
            ids.reverse()
        return ([self.bos] if add_bos else []) + ids + ([self.eos] if add_eos else [])


def bpe_rows(rng, vocab):
    rows, hand = sentences(rng, vocab)
    rows[hand["row_5000"]] = rows[hand["row_5000"]][:700]   # (a whole sentence is one segment for `edit`: kept to a few waves)
    hand["row_700"] = hand.pop("row_5000")
    free = [k for k in range(len(rows)) if k not in set(hand.values())][-40:]
    extra = {
        "counter": "ξψωχ", "counter_in_text": "kato ξψωχ mireξψωχξψωχ ωχξψ", "counter_twice": "ξψωχξψωχ",
        "chain_8": "aaaaaaaa", "chain_9": "aaaaaaaaa", "chain_23": "kato " + "a" * 23 + " mire", "same_pair_thrice": "kakaka aaaaaa",
        "two_spaces_inside": "kato   mire", "space_symbols": "▁▁▁ ▁▁ kato▁▁mire", "inner_space_piece": "kato ξ mire ξξ ψ",
        "long_segment": "katomiresulo" * 12, "long_segment_in_text": "kato " + "mireka" * 25 + " sulo 😀",
        "long_unknowns": "漢字😀" * 16, "seg_63": "k" * 62, "seg_64": "k" * 63, "seg_65": "k" * 64, "seg_129": "ka" * 64,
        "four_byte_end": "kato😀 mire𓀀", "four_byte_at_wave_end": "k" * 59 + "😀 kato",
    }
    for (name, s), k in zip(extra.items(), free):
        rows[k] = s.encode()
        hand[name] = k
    return rows, hand


def main():
    rng = random.Random(20251018)
    vocab = words(rng)
    lines = corpus(rng, vocab)
    models = {"bytes": train(lines, vocab_size=420, character_coverage=1.0, byte_fallback=True, normalization_rule_name="identity"),
              "unk": train(lines, vocab_size=300, character_coverage=1.0)}
    assert models["unk"] == train(lines, vocab_size=300, character_coverage=1.0), "training is not deterministic"
    models["edit"] = edited(models["bytes"])
    rows, hand = bpe_rows(rng, vocab)
    assert len(rows) == 2000 and max(map(len, rows)) <= 700

    ends = np.cumsum([len(r) for r in rows]).astype(np.int32)
    out = {"chars": np.frombuffer(b"".join(rows), np.uint8), "ends": ends, "hand_names": np.array(sorted(hand)),
           "hand_index": np.array([hand[k] for k in sorted(hand)], np.int32)}
    for name in MODELS:
        data = models[name]
        assert len(data) < 300 << 10, (name, len(data))
        (G / f"spm_bpe_{name}.model").write_bytes(data)
        r = Restated(data)
        sp = r.sp
        for opt, kw in OPTIONS.items():
            ids = [sp.encode(row, **kw) for row in rows]
            for row, want in zip(rows, ids):
                got = r.encode(row, **kw)
                assert got == want, (name, opt, row, got, want)
            flat = np.array([x for row in ids for x in row], np.int64)
            assert flat.min() >= 0 and flat.max() < 65536
            out[f"{name}_{opt}_ids"] = flat.astype(np.uint16)
            out[f"{name}_{opt}_ends"] = np.cumsum([len(x) for x in ids]).astype(np.int32)
        pieces = lambda s: sp.encode(s, out_type=str)   # noqa: E731
        plain = [sp.encode(row) for row in rows]
        n_unk = sum((any(sp.is_byte(i) for i in ids) if name != "unk" else sp.unk_id() in ids) for ids in plain)
        print(f"{name}: {len(data)} bytes, {sp.get_piece_size()} pieces; rows {len(rows)}, with unknown {n_unk}")
        assert n_unk * 10 >= len(rows), name
        if name == "unk":   # a run of unknown characters is one id
            assert plain[hand["unknown_run_4byte"]].count(sp.unk_id()) == 1 and plain[hand["unknowns_apart"]].count(sp.unk_id()) == 4
        if name == "edit":
            assert pieces("ξψωχ") == [SP, "ξψω", "χ"], pieces("ξψωχ")   # merging every local maximum at once would give ξψ ωχ
            assert pieces("ξψωχξψωχ") == [SP, "ξψω", "χ", "ξψω", "χ"]
            assert "aaaaaaaa" in pieces("aaaaaaaa") and "aaaa" in pieces("a" * 23)
            assert SP + SP in pieces("▁▁▁ ▁▁ kato▁▁mire")
            assert "ξ" + SP in pieces("kato ξ mire ξξ ψ")
            base = spm.SentencePieceProcessor(model_proto=models["bytes"])
            assert any(base.encode(row) != ids for row, ids in zip(rows, plain))
    # what the merge kernel's left-over path is for: a stretch of normalized text without a cut that is longer than two wave forms
    norm = Restated(models["bytes"]).sp.normalize(rows[hand["long_segment"]])
    norm = norm.encode() if isinstance(norm, str) else norm
    assert max(map(len, norm.split(SP.encode()))) > 2 * WAVE
    # SentencepieceDetokenizer's side of the round trip: the package's texts for the first rows' ids (`bytes`, plain)
    sp = spm.SentencePieceProcessor(model_proto=models["bytes"])
    texts = [sp.decode(sp.encode(row)).encode() for row in rows[:300]]
    out["bytes_decoded_chars"] = np.frombuffer(b"".join(texts), np.uint8)
    out["bytes_decoded_ends"] = np.cumsum([len(t) for t in texts]).astype(np.int32)
    unused, tie = refused(models["bytes"])
    (G / "spm_bpe_refuse_unused.model").write_bytes(unused)
    (G / "spm_bpe_refuse_tie.model").write_bytes(tie)
    np.savez_compressed(G / "golden_sentencepiece_bpe.npz", **out)
    size = (G / "golden_sentencepiece_bpe.npz").stat().st_size
    print("golden_sentencepiece_bpe.npz:", size, "bytes")
    assert size < 1 << 20
    return 0


if __name__ == "__main__":
    sys.exit(main())
