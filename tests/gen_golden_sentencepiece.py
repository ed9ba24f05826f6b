"""Writes tests/golden/spm_unigram_{nfkc,bytes,edit}.model, spm_refuse_bpe.model and golden_sentencepiece.npz: small unigram models
trained in-process by the `sentencepiece` package (num_threads=1: deterministic) on a generated corpus, and the package's ids for a
fixed list of sentences -- plain, add_bos, add_eos, both, reverse alone.  Nothing is downloaded.  Run from the repository root:

    python tests/gen_golden_sentencepiece.py

The script asserts that the goldens exercise what they are there for (unknowns, runs of unknowns, normalization that changes the
length, empty rows, the tie, the chain, the UNUSED pieces) and fails otherwise.
"""
import io
import random
import sys
from pathlib import Path

import numpy as np
import sentencepiece as spm
from sentencepiece import sentencepiece_model_pb2 as pb

G = Path(__file__).resolve().parent / "golden"
OPTIONS = {"plain": {}, "bos": {"add_bos": True}, "eos": {"add_eos": True}, "bos_eos": {"add_bos": True, "add_eos": True}, "reverse": {"reverse": True}}
MODELS = ("nfkc", "bytes", "edit")

SYLL = ["ka", "to", "mi", "re", "su", "lo", "an", "be", "di", "fu", "ga", "he", "in", "jo", "ku", "le", "mo", "ne", "or", "pa", "ri", "sa", "te",
        "ul", "va", "we", "xi", "yo", "zu", "ch", "th", "st", "é", "ü", "ñ", "ø", "α", "β", "γ", "д", "ж", "я"]
UNKNOWN = ["😀", "🚀", "𝔘", "漢", "字", "ऋ", "ꙮ", "‰", "⚑", "𓀀"]           # never in the corpus
WIDENING = ["ﬁ", "①", "Ａ", "ｂ", "Ｃ", "㌔", "½", "ǆ", "™", "ﷺ"]             # NFKC makes them longer or shorter
SPACES = ["  ", "   ", "\t", " \t ", "　", " "]


def words(rng, n=260):
    out = set()
    while len(out) < n:
        out.add("".join(rng.choice(SYLL) for _ in range(rng.randint(1, 4))))
    return sorted(out)


def corpus(rng, vocab, lines=6000):
    weights = [1.0 / (k + 1) for k in range(len(vocab))]
    return [" ".join(rng.choices(vocab, weights, k=rng.randint(3, 14))) for _ in range(lines)]


def train(lines, **kw):
    buf = io.BytesIO()
    spm.SentencePieceTrainer.train(sentence_iterator=iter(lines), model_writer=buf, model_type="unigram", num_threads=1,
                                   hard_vocab_limit=False, minloglevel=2, **kw)
    return buf.getvalue()


def edited(model_bytes):
    """(c): (b) with UNUSED pieces, a chain a, aa, ... of 10 pieces, and two paths of equal float32 sums."""
    m = pb.ModelProto()
    m.ParseFromString(model_bytes)
    by_name = {p.piece: i for i, p in enumerate(m.pieces)}
    normal = [p for p in m.pieces if p.type == pb.ModelProto.SentencePiece.NORMAL]
    # a single character that must become unknown, and the best multi-character piece (it would have won)
    single = max((p for p in normal if len(p.piece) == 1 and p.piece.isalpha() and p.piece != "a"), key=lambda p: p.score)
    multi = max((p for p in normal if len(p.piece) >= 3 and not p.piece.startswith("a")), key=lambda p: p.score)
    for p in (single, multi):
        p.type = pb.ModelProto.SentencePiece.UNUSED
    unused = [single.piece, multi.piece]

    def put(piece, score):
        if piece in by_name:
            p = m.pieces[by_name[piece]]
            p.score, p.type = score, pb.ModelProto.SentencePiece.NORMAL
        else:
            by_name[piece] = len(m.pieces)
            m.pieces.add(piece=piece, score=score, type=pb.ModelProto.SentencePiece.NORMAL)

    for k in range(1, 11):
        put("a" * k, -(3.0 + 0.75 * k))
    # "▁" -3, then ξψ (-6) against ξ (-2) + ψ (-4): every sum is exact, the two paths are equal, the earliest start wins
    put("▁", -3.0)
    put("ξ", -2.0)
    put("ψ", -4.0)
    put("ξψ", -6.0)
    assert np.float32(np.float32(-3.0) + np.float32(-6.0)) == np.float32(np.float32(np.float32(-3.0) + np.float32(-2.0)) + np.float32(-4.0))
    return m.SerializeToString(), unused


def sentences(rng, vocab):
    """-> (list of bytes, {name: index} of the hand-made rows)."""
    rows, hand = [], {}

    def add(name, s):
        hand[name] = len(rows)
        rows.append(s if isinstance(s, bytes) else s.encode())

    add("empty", "")
    add("two_spaces", "  ")
    add("one_byte", "k")
    add("longer_normalized", "ﬁ① ＡＢｃ ﬁ")
    add("unknown_first", "😀kato mire")
    add("unknown_last", "kato mire😀")
    add("unknowns_apart", "漢 字 漢 字")
    add("unknown_run_4byte", "kato 😀🚀𝔘𓀀 mire")
    add("control_as_text", "<s> kato </s> <unk>")
    add("byte_piece_as_text", "<0x41> kato<0x0A>")
    add("literal_space_symbol", "ka▁to ▁ mi▁")
    add("lone_continuation", b"kato \x80 mire\xbf")
    add("truncated_lead", b"kato \xe2\x96 mire \xf0\x9f")
    add("chain_10", "aaaaaaaaaa")
    add("chain_in_text", "kato aaaaaaaaaaaaaaaaaaaaaaa mire aaaaaaaaa")
    add("tie", "ξψ")
    add("tie_in_text", "kato ξψξψ ψξ mire")
    add("row_5000", (" ".join(rng.choices(vocab, k=1200)) + " 😀😀 ﬁ")[:4990] + " kato")
    add("tab_only", "\t")
    add("wide_space_only", "　  ")
    for k in range(40):   # empty after normalization, or nothing but whitespace (the identity normalizer keeps a tab)
        add(f"blank_{k}", rng.choice(["", " ", "  ", "   ", "     ", "\t ", " \u3000", "\n"]))
    while len(rows) < 2000:
        kind = rng.random()
        ws = rng.choices(vocab, k=rng.randint(1, 9))
        if kind < 0.18:     # unknown characters, alone and in runs
            for _ in range(rng.randint(1, 3)):
                ws.insert(rng.randrange(len(ws) + 1), "".join(rng.choices(UNKNOWN, k=rng.choice([1, 1, 2, 3, 5]))))
        elif kind < 0.30:   # an unknown glued to a word
            k = rng.randrange(len(ws))
            ws[k] = ws[k] + "".join(rng.choices(UNKNOWN, k=rng.choice([1, 2, 2, 4]))) + rng.choice(["", "ka"])
        elif kind < 0.42:   # characters the normalizer rewrites
            for _ in range(rng.randint(1, 3)):
                ws.insert(rng.randrange(len(ws) + 1), "".join(rng.choices(WIDENING, k=rng.randint(1, 3))))
        elif kind < 0.50:   # the edited model's additions
            ws.insert(rng.randrange(len(ws) + 1), rng.choice(["a" * rng.randint(1, 14), "ξψ", "ψξψ", "ξξψψ"]))
        s = ""
        for k, w_ in enumerate(ws):
            s += (rng.choice(SPACES) if rng.random() < 0.08 else " ") if k else (" " if rng.random() < 0.05 else "")
            s += w_
        if rng.random() < 0.05:
            s += rng.choice(SPACES)
        data = s.encode()
        if rng.random() < 0.04:   # invalid UTF-8: a byte dropped or a stray one put in
            k = rng.randrange(len(data) + 1)
            data = data[:k] + bytes([rng.choice([0x80, 0xBF, 0xC3, 0xE2, 0xF0, 0xFF])]) + data[k:]
        while len(data) > 300:
            data = data[:len(data) // 2]
        rows.append(data)
    return rows, hand


def main():
    rng = random.Random(20251018)
    vocab = words(rng)
    lines = corpus(rng, vocab)
    models = {"nfkc": train(lines, vocab_size=400, character_coverage=1.0),
              "bytes": train(lines, vocab_size=520, character_coverage=1.0, byte_fallback=True, normalization_rule_name="identity")}
    assert models["nfkc"] == train(lines, vocab_size=400, character_coverage=1.0), "training is not deterministic"
    models["edit"], unused = edited(models["bytes"])
    rows, hand = sentences(rng, vocab)
    assert max(len(r) for k, r in enumerate(rows) if k != hand["row_5000"]) <= 300

    ends = np.cumsum([len(r) for r in rows]).astype(np.int32)
    out = {"chars": np.frombuffer(b"".join(rows), np.uint8), "ends": ends, "hand_names": np.array(sorted(hand)),
           "hand_index": np.array([hand[k] for k in sorted(hand)], np.int32), "edit_unused": np.array(unused)}
    for name in MODELS:
        data = models[name]
        assert len(data) < 300 << 10, (name, len(data))
        (G / f"spm_unigram_{name}.model").write_bytes(data)
        sp = spm.SentencePieceProcessor(model_proto=data)
        unk = sp.unk_id()
        is_byte = np.array([sp.is_byte(i) for i in range(sp.get_piece_size())])
        plain = [sp.encode(r) for r in rows]
        n_unk = n_run = n_len = n_blank = 0
        for r, ids in zip(rows, plain):
            a = np.asarray(ids, np.int64)
            if name == "nfkc":
                has = unk in ids
                run = any(i == unk and len(p) >= 2 for i, p in zip(ids, sp.encode(r, out_type=str)))
            else:
                byte = is_byte[a] if len(a) else np.zeros(0, bool)
                has, run, k = bool(byte.any()), False, 0
                while k < len(a):   # a run of byte pieces that spells two or more characters
                    j = k
                    while j < len(a) and byte[j]:
                        j += 1
                    if j > k:
                        text = bytes(int(sp.id_to_piece(int(x))[3:5], 16) for x in a[k:j]).decode("utf-8", "replace")
                        run |= len(text) >= 2
                    k = max(j, k + 1)
            n_unk += has
            n_run += run
            normalized = sp.normalize(r)
            n_len += len(normalized.encode() if isinstance(normalized, str) else normalized) != len(r)
            n_blank += len(ids) == 0
        n = len(rows)
        print(f"{name}: {len(data)} bytes, {sp.get_piece_size()} pieces; rows {n}, with unknown {n_unk}, with a run {n_run}, "
              f"length changed {n_len}, empty {n_blank}")
        assert n_unk * 10 >= n and n_run * 20 >= n and n_len * 20 >= n and n_blank >= 20, name
        for opt, kw in OPTIONS.items():
            ids = [sp.encode(r, **kw) for r in rows]
            flat = np.array([x for row in ids for x in row], np.int64)
            assert flat.size == 0 or (flat.min() >= 0 and flat.max() < 65536)
            out[f"{name}_{opt}_ids"] = flat.astype(np.uint16)
            out[f"{name}_{opt}_ends"] = np.cumsum([len(x) for x in ids]).astype(np.int32)
        if name == "edit":
            pieces = lambda s: sp.encode(s, out_type=str)   # noqa: E731
            assert pieces("ξψ") == ["▁", "ξψ"], pieces("ξψ")                     # the earliest start wins the tie
            assert all(p not in unused for r in rows[:400] for p in pieces(r))          # an UNUSED piece is never chosen
            base = spm.SentencePieceProcessor(model_proto=models["bytes"])
            assert any(set(unused) & set(base.encode(r, out_type=str)) for r in rows)   # ... and would have been
            assert len(sp.encode("aaaaaaaaaa")) >= 1
    # a model this library refuses by its type
    m = pb.ModelProto()
    m.ParseFromString(models["bytes"])
    m.trainer_spec.model_type = pb.TrainerSpec.BPE
    (G / "spm_refuse_bpe.model").write_bytes(m.SerializeToString())
    np.savez_compressed(G / "golden_sentencepiece.npz", **out)
    size = (G / "golden_sentencepiece.npz").stat().st_size
    print("golden_sentencepiece.npz:", size, "bytes")
    assert size < 1 << 20
    return 0


if __name__ == "__main__":
    sys.exit(main())
