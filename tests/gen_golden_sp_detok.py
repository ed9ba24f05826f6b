"""Writes tests/golden/spm_detok_*.model and golden_sp_detok.npz: id matrices and what the `sentencepiece` package decodes them to
(SentencepieceDetokenizer, src/sentence_piece.cpp:395-433), plus a restatement of :496-517 over the package's id_to_piece
(SentencepieceStreamDetokenizer).  The derived models are the encoder's fixtures with the proto edited.  Nothing is downloaded.  Run
from the repository root:

    python tests/gen_golden_sp_detok.py

The script asserts that the goldens exercise what they are there for and fails otherwise.
"""
import random
import sys
from pathlib import Path

import numpy as np
import sentencepiece as spm
from sentencepiece import sentencepiece_model_pb2 as pb

G = Path(__file__).resolve().parent / "golden"
T = pb.ModelProto.SentencePiece
SP = "▁"
SHAPES = [(64, 1), (65, 3), (7, 64), (5, 65), (3, 513), (2, 1030)]
FLAGS = {"tt": (True, True), "tf": (True, False), "ft": (False, True), "ff": (False, False)}
UNCHANGED = {"nfkc": "spm_unigram_nfkc", "bytes": "spm_unigram_bytes", "edit": "spm_unigram_edit", "bpe": "spm_refuse_bpe"}
DERIVED = ["tt", "tf", "ft", "ff", "unk", "nfkc41"]
MODELS = list(UNCHANGED) + DERIVED


def model_file(name):
    return G / (UNCHANGED[name] + ".model" if name in UNCHANGED else f"spm_detok_{name}.model")


def with_pieces(data, unused, extra=()):
    m = pb.ModelProto()
    m.ParseFromString(data)
    have = {p.piece for p in m.pieces}
    for piece, kind in [(SP, T.NORMAL), (SP + SP, T.NORMAL), (SP + SP + "ka", T.NORMAL), ("ka" + SP + SP + "to", T.NORMAL),
                        (SP + "♞" + SP + "♞", T.USER_DEFINED)] + list(extra):
        if piece not in have:
            m.pieces.add(piece=piece, score=-6.0, type=kind)
    for p in m.pieces:
        if p.piece in unused:
            p.type = T.UNUSED
    return m


def derive():
    """-> {name: bytes} of the derived models."""
    base = model_file("bytes").read_bytes()
    nfkc = model_file("nfkc").read_bytes()
    e = pb.ModelProto()
    e.ParseFromString(model_file("edit").read_bytes())
    unused = {p.piece for p in e.pieces if p.type == T.UNUSED}
    assert len(unused) == 2
    out = {}
    for name, (dummy, extra_ws) in FLAGS.items():
        m = with_pieces(base, unused)
        m.normalizer_spec.add_dummy_prefix = dummy
        m.normalizer_spec.remove_extra_whitespaces = extra_ws
        out[name] = m.SerializeToString()
    m = pb.ModelProto()
    m.ParseFromString(base)
    m.trainer_spec.unk_surface = "<?>"
    out["unk"] = m.SerializeToString()
    m = with_pieces(nfkc, set(), [("<0x41>", T.NORMAL)])   # a NORMAL piece with a byte piece's name, in a model without byte pieces
    assert not m.trainer_spec.byte_fallback
    out["nfkc41"] = m.SerializeToString()
    return out


class Vocab:
    def __init__(self, data):
        self.sp = sp = spm.SentencePieceProcessor(model_proto=data)
        m = pb.ModelProto()
        m.ParseFromString(data)
        self.V = sp.get_piece_size()
        self.id = {p.piece: i for i, p in enumerate(m.pieces)}
        self.type = [p.type for p in m.pieces]
        self.byte = {int(p.piece[3:5], 16): i for i, p in enumerate(m.pieces) if p.type == T.BYTE}
        self.unk = sp.unk_id()
        self.control = [i for i, t in enumerate(self.type) if t == T.CONTROL]
        normal = [i for i, t in enumerate(self.type) if t == T.NORMAL]
        self.lead = [i for i in normal if m.pieces[i].piece.startswith(SP) and len(m.pieces[i].piece) >= 3 and SP not in m.pieces[i].piece[1:]]
        self.plain = [i for i in normal if SP not in m.pieces[i].piece and not m.pieces[i].piece.startswith("<")]
        self.word = self.id.get(SP + "anøga", self.lead[0])
        self.x = self.plain[0]
        self.unused = [i for i, t in enumerate(self.type) if t == T.UNUSED]
        self.user = [i for i, t in enumerate(self.type) if t == T.USER_DEFINED]

    def decode(self, row):
        return self.sp.decode([int(x) for x in row if x < self.V]).encode()

    def stream(self, row):
        """src/sentence_piece.cpp:496-517."""
        out = b""
        for t in (self.sp.id_to_piece(int(x)).encode() for x in row if x < self.V):
            out += bytes([int(t[3:5], 16)]) if len(t) == 6 and t[:3] == b"<0x" and t[5:] == b">" else t
        return out


def hand_rows(v):
    """-> {name: ids}; a case a model has no pieces for is left out for that model."""
    rows = {}
    S, W, X, U, D = v.id.get(SP), v.word, v.x, v.unk, v.V + 7
    bos, eos = v.id.get("<s>"), v.id.get("</s>")
    B = (lambda *bs: [v.byte[b] for b in bs]) if len(v.byte) == 256 else None

    def add(name, ids, needs=()):
        if all(x is not None for x in needs):
            rows[name] = ids

    add("control_around_word", [bos, W, eos], (bos, eos))
    add("unknown_then_word", [U, W])
    add("unknowns_do_not_merge", [U, U, W, U])
    add("word_alone", [W])
    add("plain_then_word", [X, W])
    if v.unused:
        add("unused_decodes_like_normal", [v.unused[0], W, v.unused[1]])
    if v.user:
        add("user_defined", [v.user[0], v.user[0], W])
    if "<0x41>" in v.id and B is None:
        add("normal_piece_named_like_a_byte", [v.id["<0x41>"], W, v.id["<0x41>"]])
    add("sp_sp_word", [S, S, W], (S,))
    add("sp_alone", [S], (S,))
    add("sp_a_sp_sp_a_sp", [S, X, S, S, X, S], (S,))
    add("control_sp_word", [bos, S, W], (bos, S))
    for piece, name in ((SP + SP, "dsp"), (SP + SP + "ka", "dsp_ka"), ("ka" + SP + SP + "to", "ka_dsp_to")):
        k = v.id.get(piece)
        add(f"{name}_first", [k, W], (k,))
        add(f"{name}_alone", [k], (k,))
        add(f"{name}_after_sp", [S, k, k], (k, S))
        add(f"{name}_after_control", [bos, k], (k, bos))
        add(f"{name}_in_the_middle", [X, k, W], (k,))
    add("empty_row", [])
    add("dropped_only", [D, D + 1000, D])
    add("dropped_1030", [D] * 1030)
    add("sp_1030", [S] * 1030, (S,))
    add("first_state_end_at_700", [S] * 350 + [bos] * 350 + [W, S, W], (S, bos))
    add("padding_then_word_at_700", [D] * 700 + [W, W], ())
    if B:
        add("byte_A_then_word", B(0x41) + [W])
        add("byte_space_then_word", B(0x20) + [W])
        add("truncated_E2_96", B(0xE2, 0x96))
        add("overlong_C0_80", B(0xC0, 0x80))
        add("surrogate_ED_A0_80", B(0xED, 0xA0, 0x80))
        add("beyond_F4_90_80_80", B(0xF4, 0x90, 0x80, 0x80))
        add("mixed_80_41_F09F9880_FF", B(0x80, 0x41, 0xF0, 0x9F, 0x98, 0x80, 0xFF))
        add("nul_byte", B(0x00))
        add("bytes_spell_the_space_symbol", B(0xE2, 0x96, 0x81) + [W] + B(0xE2, 0x96, 0x81))
        add("replacement_character_itself", B(0xEF, 0xBF, 0xBD))
        add("run_split_by_control", [bos] + B(0xE2) + [eos] + B(0x96, 0x81), (bos, eos))
        add("run_split_by_unknown", B(0xE2) + [U] + B(0x96))
        add("run_split_by_plain_piece", B(0xE2, 0x96) + [X] + B(0x81))
        add("run_over_one_dropped_id", B(0xE2) + [D] + B(0x96, 0x81))
        add("run_over_600_dropped_ids", [X] * 500 + B(0xE2) + [D] * 600 + B(0x96, 0x81) + [X])
        add("run_over_dropped_then_control", B(0xE2) + [D] * 600 + [bos] + B(0x96, 0x81), (bos,))
        add("four_bytes_straddle_512_and_1024", [X] * 510 + B(0xF0, 0x9F, 0x98, 0x80) + [X] * 508 + B(0xF0, 0x9F, 0x98, 0x80) + [X])
        add("three_bytes_1_2_over_512", [X] * 511 + B(0xE2, 0x96, 0x81))
        add("three_bytes_2_1_over_512", [X] * 510 + B(0xE2, 0x96, 0x81))
        add("lead_at_511_dropped_behind", [X] * 511 + B(0xE2) + [D] * 512 + B(0x96, 0x81))
        add("lead_at_511_nothing_behind", [X] * 511 + B(0xE2) + [D] * 100)
        add("continuation_at_512_dropped_in_front", B(0xC3) + [D] * 511 + B(0xA9) + [W])
        add("continuation_at_512_nothing_in_front", [D] * 512 + B(0xA9) + [W])
        add("E2_1030", B(0xE2) * 1030)
        add("valid_two_byte_characters_1030", B(0xC3, 0xA9) * 515)
    return rows


def mixture(rng, v, shape):
    """Rows made of characters spelled in byte pieces (dropped ids inside them), stray bytes, unknowns, controls and words."""
    out = np.empty(shape, np.int32)
    chars = "éüøдя漢字‰😀🚀"
    for r in range(shape[0]):
        row = []
        while len(row) < shape[1]:
            k = rng.random()
            if k < 0.35 and v.byte:
                ids = [v.byte[b] for b in rng.choice(chars[:5] if rng.random() < 0.6 else chars).encode()]
                if rng.random() < 0.5:
                    ids.insert(rng.randrange(1, len(ids)), v.V + rng.randrange(40))
                row += ids
            elif k < 0.45 and v.byte:
                row += [v.byte[rng.choice([0x80, 0xBF, 0xC0, 0xE2, 0xF0, 0xF4, 0xFF, 0x41, 0x20])] for _ in range(rng.randint(1, 3))]
            elif k < 0.55:
                row.append(v.unk)
            elif k < 0.65:
                row.append(rng.choice(v.control))
            elif k < 0.75:
                row.append(v.V + rng.randrange(40))
            else:
                row.append(rng.choice(v.lead if rng.random() < 0.6 else v.plain))
        out[r] = row[:shape[1]]
    return out


def phenomena(v, row):
    ids = [int(x) for x in row if x < v.V]
    text = v.decode(row)
    is_byte = [v.type[i] == T.BYTE for i in ids]
    runs, k = [], 0
    while k < len(ids):
        j = k
        while j < len(ids) and is_byte[j]:
            j += 1
        if j > k:
            runs.append(bytes(int(v.sp.id_to_piece(i)[3:5], 16) for i in ids[k:j]).decode("utf-8", "replace"))
        k = max(j, k + 1)
    kept = [int(x) for x in row]
    inside = any(kept[k] >= v.V and any(x < v.V for x in kept[:k]) and any(x < v.V for x in kept[k + 1:]) and
                 v.type[[x for x in kept[:k] if x < v.V][-1]] == T.BYTE and v.type[[x for x in kept[k + 1:] if x < v.V][0]] == T.BYTE
                 for k in range(len(kept)))
    after_plain = v.sp.decode([v.x] + ids).encode()[len(v.sp.decode([v.x]).encode()):] if ids else b""
    # (in front of a plain piece nothing is stripped from it, and behind it nothing is: the difference is the start of the sentence)
    return {"stripped": bool(ids) and after_plain != text and len(after_plain) > len(text), "unknown": v.unk in ids,
            "replaced": any("�" in r for r in runs), "multibyte": any(ord(c) >= 0x80 and c != "�" for r in runs for c in r),
            "dropped_in_run": inside}


def pack(strings):
    return np.frombuffer(b"".join(strings), np.uint8), np.cumsum([len(s) for s in strings]).astype(np.int32)


def main():
    rng = random.Random(20251019)
    nprng = np.random.default_rng(20251019)
    derived = derive()
    for name, data in derived.items():
        assert len(data) < 300 << 10, (name, len(data))
        model_file(name).write_bytes(data)
    z = np.load(G / "golden_sentencepiece.npz")
    ends = z["ends"]
    sentences = [bytes(z["chars"][a:b]) for a, b in zip(np.concatenate([[0], ends[:-1]]), ends)][:400]
    out = {"models": np.array(MODELS)}
    seen_hand = set()
    for name in MODELS:
        v = Vocab(model_file(name).read_bytes())
        sets = {}
        # ---- round trip: the package's own ids, padded with ids outside the vocabulary
        enc = [v.sp.encode(s) for s in sentences]
        long_rows = [k for k, e in enumerate(enc) if len(e) > 256]
        assert len(long_rows) == 1   # the row of 5 000 bytes: a matrix of its own
        right = [k for k in range(300) if k not in long_rows]
        left = [k for k in range(300, 400)]

        def padded(rows, side):
            w = max(len(enc[k]) for k in rows) + 3
            m = np.empty((len(rows), w), np.int32)
            for r, k in enumerate(rows):
                pad = [v.V if (r + j) % 2 else v.V + 1000 for j in range(w - len(enc[k]))]
                m[r] = enc[k] + pad if side == "right" else pad + enc[k]
            return m
        sets["rt_right"], sets["rt_left"], sets["rt_long"] = padded(right, "right"), padded(left, "left"), padded(long_rows, "right")
        for k in right[:50]:
            assert v.decode(enc[k]) == v.sp.decode(enc[k]).encode()
        # ---- random ids
        stats, n_random = {}, 0
        for k, shape in enumerate(SHAPES):
            uni = nprng.integers(0, v.V + 40, shape).astype(np.int32)
            mix = mixture(rng, v, shape)
            if len(v.byte) == 256:
                b = v.byte
                if shape[1] == 513:
                    uni[0, 510:513] = [b[0xE2], b[0x96], b[0x81]]
                    mix[0, 509:513] = [b[0xF0], b[0x9F], b[0x98], b[0x80]]
                if shape[1] == 1030:
                    uni[0, 1022:1026] = [b[0xF0], b[0x9F], b[0x98], b[0x80]]
                    uni[1, 509:514] = [b[0xE2], v.V + 3, b[0x96], v.V + 9, b[0x81]]
                    mix[1, 1023:1025] = [b[0xC3], b[0xA9]]
            sets[f"rnd{k}"], sets[f"mix{k}"] = uni, mix
            for m in (uni, mix):
                for row in m:
                    n_random += 1
                    for key, hit in phenomena(v, row).items():
                        stats[key] = stats.get(key, 0) + hit
        if len(v.byte) == 256:
            types = lambda row, a, b_: all(x < v.V and v.type[x] == T.BYTE for x in row[a:b_])   # noqa: E731
            assert types(sets["rnd4"][0], 510, 513) and types(sets["rnd5"][0], 1022, 1026)   # runs that straddle 511/512 and 1023/1024
        can = {"stripped": v.sp.decode([v.word]) != v.sp.decode([v.x, v.word])[len(v.sp.decode([v.x])):], "unknown": True,
               "replaced": bool(v.byte), "multibyte": bool(v.byte), "dropped_in_run": bool(v.byte)}
        print(f"{name}: {v.V} pieces, random rows {n_random}: " + ", ".join(f"{k} {n}" for k, n in sorted(stats.items())))
        for key, possible in can.items():
            assert not possible or stats[key] * 20 >= n_random, (name, key, stats[key], n_random)
        for key, m in sets.items():
            out[f"{name}_{key}_ids"] = m
            out[f"{name}_{key}_dec_chars"], out[f"{name}_{key}_dec_ends"] = pack([v.decode(r) for r in m])
            out[f"{name}_{key}_str_chars"], out[f"{name}_{key}_str_ends"] = pack([v.stream(r) for r in m])
        # ---- the hand-made rows
        hand = hand_rows(v)
        seen_hand |= set(hand)
        names = sorted(hand)
        out[f"{name}_hand_names"] = np.array(names)
        out[f"{name}_hand_ids"] = np.array([x for n in names for x in hand[n]], np.int32)
        out[f"{name}_hand_id_ends"] = np.cumsum([len(hand[n]) for n in names]).astype(np.int32)
        out[f"{name}_hand_dec_chars"], out[f"{name}_hand_dec_ends"] = pack([v.decode(hand[n]) for n in names])
        out[f"{name}_hand_str_chars"], out[f"{name}_hand_str_ends"] = pack([v.stream(hand[n]) for n in names])
        # ---- what the issue's examples say, from the package
        dec = lambda n: v.decode(hand[n]).decode()   # noqa: E731
        w = v.sp.id_to_piece(v.word)[1:]
        if name in FLAGS:
            dummy, extra_ws = FLAGS[name]
            assert dec("control_around_word") == (w if dummy or extra_ws else " " + w)
            assert dec("unknown_then_word") == " ⁇  " + w
            assert dec("sp_sp_word") == {"tt": w, "tf": "  " + w, "ft": w, "ff": "   " + w}[name]
            assert dec("sp_alone") == (" " if name == "ff" else "")
            if name != "ff":
                assert dec("sp_a_sp_sp_a_sp") == "{0}  {0} ".format(v.sp.id_to_piece(v.x))
            assert dec("byte_A_then_word") == "A " + w and dec("byte_space_then_word") == "  " + w
            assert dec("truncated_E2_96") == "�" * 2 and dec("overlong_C0_80") == "�" * 2 and dec("surrogate_ED_A0_80") == "�" * 3
            assert dec("beyond_F4_90_80_80") == "�" * 4 and dec("mixed_80_41_F09F9880_FF") == "�A😀�" and dec("nul_byte") == "\0"
            assert dec("bytes_spell_the_space_symbol").startswith(SP) and dec("run_split_by_control") == "�" * 3
            assert dec("run_split_by_unknown") == "� ⁇ �" and dec("run_over_one_dropped_id") == SP
            assert SP in dec("run_over_600_dropped_ids") and "😀" in dec("four_bytes_straddle_512_and_1024")
            assert dec("E2_1030") == "�" * 1030 and dec("dropped_1030") == "" and dec("empty_row") == ""
        if name == "unk":
            assert dec("unknown_then_word") == "<?> " + w
        if name == "nfkc41":
            assert dec("normal_piece_named_like_a_byte").startswith("<0x41>")
    print("hand-made cases:", len(seen_hand))
    assert len(seen_hand) >= 50 and all(set(out[f"{n}_hand_names"].tolist()) >= seen_hand - {"normal_piece_named_like_a_byte"} for n in FLAGS)
    out["hand_cases"] = np.array(sorted(seen_hand))
    np.savez_compressed(G / "golden_sp_detok.npz", **out)
    size = (G / "golden_sp_detok.npz").stat().st_size
    print("golden_sp_detok.npz:", size, "bytes")
    assert size < 1 << 20
    return 0


if __name__ == "__main__":
    sys.exit(main())
