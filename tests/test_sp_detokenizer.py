"""SentencepieceDetokenizer (src/sentence_piece.cpp:395-433) and SentencepieceStreamDetokenizer (:478-523) against the `sentencepiece`
package: tests/gen_golden_sp_detok.py recorded what it decodes the id matrices to, for unigram, BPE-typed and edited models.  Every
comparison is of whole arrays, no tolerance anywhere."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

G = Path(__file__).resolve().parent / "golden"
Z = np.load(G / "golden_sp_detok.npz")
MODELS = [str(m) for m in Z["models"]]
HAND = [str(n) for n in Z["hand_cases"]]
UNCHANGED = {"nfkc": "spm_unigram_nfkc", "bytes": "spm_unigram_bytes", "edit": "spm_unigram_edit", "bpe": "spm_refuse_bpe"}
SETS = ["rt_right", "rt_left", "rt_long"] + [f"{k}{i}" for k in ("rnd", "mix") for i in range(6)]
OPS = {"decode": "dec", "stream": "str"}


def model(name):
    return np.frombuffer((G / (UNCHANGED[name] + ".model" if name in UNCHANGED else f"spm_detok_{name}.model")).read_bytes(), np.uint8)


def cut(ends, data):
    return [bytes(data[a:b]) for a, b in zip(np.concatenate([[0], ends[:-1]]).astype(np.int64), ends)]


def make_op(backend, kind):
    from openvino_tokenizers_amd.ops import SentencepieceDetokenizer, SentencepieceStreamDetokenizer
    return (SentencepieceDetokenizer if kind == "decode" else SentencepieceStreamDetokenizer)(lib=backend.lib)


def check(backend, op, mdl, ids, want, what):
    """want: one bytes per row."""
    ids = np.ascontiguousarray(ids, np.int32)
    got = [backend.host(x) for x in op.evaluate([mdl, backend.data([ids])[0]])]
    ends = np.cumsum([len(w) for w in want], dtype=np.int64).astype(np.int32).reshape(-1)
    ref = (ends - np.array([len(w) for w in want], np.int32), ends, np.frombuffer(b"".join(want), np.uint8))
    for name, g, r in zip(("begins", "ends", "chars"), got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, g.shape, r.shape)
        if not np.array_equal(g, r):
            k = int(np.argwhere(g != r)[0][0])
            row = int(np.searchsorted(ends, k, "right")) if name == "chars" else k
            raise AssertionError(f"{what}: {name} differs first at {k} (row {row}): got {bytes(got[2][got[0][row]:got[1][row]])[:80]!r}, "
                                 f"want {want[row][:80]!r}")
    return op


# ---------------------------------------------------------------------------------------------- the package's goldens
@pytest.mark.parametrize("kind", list(OPS))
@pytest.mark.parametrize("name", MODELS)
def test_matches_package_golden(backend, name, kind):
    op, mdl = make_op(backend, kind), model(name)
    for s in SETS:
        ids = Z[f"{name}_{s}_ids"]
        want = cut(Z[f"{name}_{s}_{OPS[kind]}_ends"], Z[f"{name}_{s}_{OPS[kind]}_chars"])
        check(backend, op, mdl, ids, want, f"{name} {s} {kind}")
        assert op.bound(*ids.shape) >= sum(map(len, want))


def hand_of(name, case):
    names = [str(n) for n in Z[f"{name}_hand_names"]]
    if case not in names:
        return None
    k = names.index(case)
    ids = cut(Z[f"{name}_hand_id_ends"], Z[f"{name}_hand_ids"].view(np.uint8).reshape(-1, 4))   # (rows of 4 bytes: cut by ids)
    return (np.frombuffer(ids[k], np.int32), cut(Z[f"{name}_hand_dec_ends"], Z[f"{name}_hand_dec_chars"])[k],
            cut(Z[f"{name}_hand_str_ends"], Z[f"{name}_hand_str_chars"])[k])


@pytest.mark.parametrize("case", HAND)
def test_hand_made_row(backend, case):
    """One named row through every model that has the pieces for it, both ops; alone in its batch and between two other rows."""
    ran = 0
    for name in MODELS:
        row = hand_of(name, case)
        if row is None:
            continue
        ids, dec, raw = row
        mdl = model(name)
        for kind, want in (("decode", dec), ("stream", raw)):
            op = check(backend, make_op(backend, kind), mdl, ids.reshape(1, -1), [want], f"{case} {name} {kind}")
            w = len(ids) + 2
            v = int(Z[f"{name}_rnd0_ids"].max()) + 2000   # an id no model has
            three = np.full((3, w), v, np.int32)
            three[0, :len(ids)], three[1, 1:1 + len(ids)], three[2, 2:] = ids, ids, ids
            check(backend, op, mdl, three, [want] * 3, f"{case} {name} {kind} x3")
        ran += 1
    assert ran >= 1


def test_examples_of_the_semantics():
    """What the goldens say for the cases the op's description names (pinned from the package by the generator)."""
    dec = lambda m, c: hand_of(m, c)[1].decode()   # noqa: E731
    assert dec("tt", "sp_sp_word") == dec("ft", "sp_sp_word") == dec("tf", "sp_sp_word").lstrip(" ") == dec("ff", "sp_sp_word").lstrip(" ")
    assert dec("tf", "sp_sp_word").startswith("  ") and dec("ff", "sp_sp_word").startswith("   ")
    assert [dec(m, "sp_alone") for m in ("tt", "tf", "ft", "ff")] == ["", "", "", " "]
    assert dec("tt", "truncated_E2_96") == "��" and dec("tt", "mixed_80_41_F09F9880_FF") == "�A😀�"
    assert dec("tt", "run_split_by_control") == "�" * 3 and dec("tt", "run_over_one_dropped_id") == "▁"
    assert dec("unk", "unknown_then_word").startswith("<?> ") and dec("tt", "unknown_then_word").startswith(" ⁇  ")
    assert dec("nfkc41", "normal_piece_named_like_a_byte").startswith("<0x41>")


# ---------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_batch_sizes(backend, n):
    for name in ("tt", "nfkc"):
        for kind in OPS:
            ids = Z[f"{name}_rt_right_ids"][40:40 + n]
            want = cut(Z[f"{name}_rt_right_{OPS[kind]}_ends"], Z[f"{name}_rt_right_{OPS[kind]}_chars"])[40:40 + n]
            check(backend, make_op(backend, kind), model(name), ids, want, f"{n} rows {name} {kind}")


@pytest.mark.parametrize("kind", list(OPS))
def test_seq_len_zero(backend, kind):
    check(backend, make_op(backend, kind), model("tt"), np.zeros((5, 0), np.int32), [b""] * 5, "seq_len 0")
    check(backend, make_op(backend, kind), model("tt"), np.zeros((0, 0), np.int32), [], "nothing at all")


# ---------------------------------------------------------------------------------------------- the C ABI's edges
def _run_raw(lib, h, ids, stream_mode, capacity, fill=0x5A):
    from openvino_tokenizers_amd import _lib as L
    ids = np.ascontiguousarray(ids, np.int32)
    b, e, c = np.full(max(len(ids), 1), -7, np.int32), np.full(max(len(ids), 1), -7, np.int32), np.full(max(capacity, 1), fill, np.uint8)
    out = L.StringsOut(b.ctypes.data, e.ctypes.data, c.ctypes.data, capacity, 0)
    rc = lib.ovtk_sp_detokenizer_run(h, ids.ctypes.data, C.c_int64(ids.shape[0]), C.c_int64(ids.shape[1]), stream_mode, C.byref(out), L.MEM_HOST, None)
    return rc, int(out.n_chars), b, e, c


@pytest.mark.parametrize("kind", list(OPS))
def test_capacity(backend, kind):
    from openvino_tokenizers_amd import _lib as L
    ids = Z["tt_mix3_ids"]
    want = cut(Z[f"tt_mix3_{OPS[kind]}_ends"], Z[f"tt_mix3_{OPS[kind]}_chars"])
    op = check(backend, make_op(backend, kind), model("tt"), ids, want, "capacity")
    need = sum(map(len, want))
    rc, n, b, e, c = _run_raw(backend.lib, op._h, ids, int(kind == "stream"), need - 1)
    assert rc == L.E_CAPACITY and n == need
    assert (c == 0x5A).all()
    rc, n, b, e, c = _run_raw(backend.lib, op._h, ids, int(kind == "stream"), need)
    assert rc == 0 and n == need and bytes(c) == b"".join(want) and e[-1] == need and b[0] == 0
    assert backend.lib.ovtk_sp_detokenizer_bound(op._h, -1, 3) == -1 and op.bound(0, 7) == 0


@pytest.mark.parametrize("kind", list(OPS))
@pytest.mark.parametrize("where", [(0, 0), (2, 63), (1, 600)])
def test_negative_id(backend, kind, where):
    from openvino_tokenizers_amd import _lib as L
    ids = Z["tt_rnd5_ids"][:, :700].copy() if where[1] >= 64 else Z["tt_rnd2_ids"].copy()
    op = make_op(backend, kind)
    op.evaluate([model("tt"), backend.data([ids])[0]])
    ids[where] = -1
    with pytest.raises(L.OvtkError) as err:
        op.evaluate([model("tt"), backend.data([ids])[0]])
    assert err.value.code == L.E_RANGE
    rc, n, b, e, c = _run_raw(backend.lib, op._h, ids, int(kind == "stream"), 1 << 16)
    assert rc == L.E_RANGE and n == 0 and (c == 0x5A).all()


def _append_field(mdl, outer, payload):
    """The model with one more sub-message field: protobuf merges it into the one already there."""
    assert len(payload) < 128
    return np.concatenate([mdl, np.frombuffer(bytes([outer << 3 | 2, len(payload)]) + payload, np.uint8)])


def _piece(text, kind=1):
    return bytes([0x0A, len(text)]) + text + bytes([0x15, 0, 0, 0, 0, 0x18, kind])


def _varint(n):
    out = b""
    while n >= 0x80:
        out += bytes([n & 0x7F | 0x80])
        n >>= 7
    return out + bytes([n])


def _n_pieces(mdl):
    """Top-level fields 1 of a ModelProto (every top-level field of the fixtures is length-delimited)."""
    buf, at, n = bytes(mdl), 0, 0
    while at < len(buf):
        tag, ln, at, shift = buf[at], 0, at + 1, 0
        assert tag & 7 == 2 and tag < 0x80
        while True:
            ln |= (buf[at] & 0x7F) << shift
            shift += 7
            at += 1
            if not buf[at - 1] & 0x80:
                break
        n += tag >> 3 == 1
        at += ln
    return n


def test_refusals(backend):
    from openvino_tokenizers_amd import _lib as L
    mdl, ids = model("tt"), backend.data([np.array([[5, 6, 7]], np.int32)])[0]

    def code(m, kind="decode", inputs=None):
        with pytest.raises(L.OvtkError) as err:
            make_op(backend, kind).evaluate([m, ids] if inputs is None else inputs)
        return err.value.code

    assert code(_append_field(mdl, 2, bytes([0xC0, 0x01, 1]))) == L.E_UNSUPPORTED   # trainer_spec.treat_whitespace_as_suffix (24) = true
    assert code(_append_field(mdl, 5, bytes([0x12, 3]) + b"abc")) == L.E_UNSUPPORTED   # denormalizer_spec.precompiled_charsmap
    assert code(_append_field(mdl, 5, bytes([0x12, 3]) + b"abc"), "stream") == L.E_UNSUPPORTED
    big = b"k" * 1024
    long_piece = bytes([0x0A, 0x80, 0x08]) + big + bytes([0x15, 0, 0, 0, 0])
    grown = np.concatenate([mdl, np.frombuffer(bytes([0x0A]) + bytes([len(long_piece) & 0x7F | 0x80, len(long_piece) >> 7]) + long_piece, np.uint8)])
    assert code(grown) == L.E_UNSUPPORTED
    # a piece of the shape <0x..> that is no upper-case hex: the stream op alone refuses it, and only when it is run
    odd = _append_field(mdl, 1, _piece(b"<0xzz>"))
    assert code(odd, "stream") == L.E_UNSUPPORTED
    assert code(_append_field(mdl, 1, _piece(b"<0xab>")), "stream") == L.E_UNSUPPORTED
    got = make_op(backend, "decode").evaluate([odd, backend.data([np.array([[_n_pieces(mdl)]], np.int32)])[0]])   # the appended piece's id
    assert bytes(backend.host(got[2])) == b"<0xzz>"
    # trainer_spec.unk_surface (44): over 1 023 bytes, and present but empty (the package never decided what that does to the start state)
    surface = bytes([0xE2, 0x02]) + _varint(1024) + b"?" * 1024
    grown = np.concatenate([mdl, np.frombuffer(bytes([0x12]) + _varint(len(surface)) + surface, np.uint8)])
    assert code(grown) == L.E_UNSUPPORTED
    assert code(_append_field(mdl, 2, bytes([0xE2, 0x02, 0]))) == L.E_UNSUPPORTED
    # arguments
    assert code(mdl, inputs=[mdl]) == L.E_ARG
    assert code(mdl, inputs=[mdl, np.zeros(4, np.int32)]) == L.E_ARG
    for n in (0, 1, 7, len(mdl) // 2, len(mdl) - 1):
        assert code(mdl[:n]) == L.E_ARG, n
        assert code(mdl[:n], "stream") == L.E_ARG, n
    # an appended, well-formed unknown field changes nothing, and an empty denormalizer_spec neither
    want = cut(Z["tt_rnd2_dec_ends"], Z["tt_rnd2_dec_chars"])
    check(backend, make_op(backend, "decode"), _append_field(_append_field(mdl, 9, b"abc"), 5, b""), Z["tt_rnd2_ids"], want, "unknown field")


def test_too_many_pieces(backend):
    """4 194 303 pieces or more are refused (an id has 22 bits elsewhere in the library); one fewer is accepted.  The pieces are empty
    messages: about 8 MB, built here."""
    from openvino_tokenizers_amd import _lib as L
    most = 4194302
    ids = np.array([[7, most - 1, most, most + 5]], np.int32)
    with pytest.raises(L.OvtkError) as err:
        make_op(backend, "decode").evaluate([np.tile(np.array([0x0A, 0], np.uint8), most + 1), backend.data([ids])[0]])
    assert err.value.code == L.E_UNSUPPORTED
    for kind in OPS:
        check(backend, make_op(backend, kind), np.tile(np.array([0x0A, 0], np.uint8), most), ids, [b""], f"{most} empty pieces {kind}")


def test_two_halves_on_two_streams(gpu_backend):
    import torch
    ops = {k: make_op(gpu_backend, k) for k in OPS}
    tickets = []
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for k, (kind, s) in enumerate(zip(OPS, streams)):
        ids = torch.as_tensor(Z[f"tt_mix{4 + k}_ids"], device="cuda")
        torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(s):
            tickets.append((kind, 4 + k, ops[kind].enqueue([model("tt"), ids])))
    for kind, k, ticket in tickets:
        got = [gpu_backend.host(x) for x in ticket()]
        blocking = [gpu_backend.host(x) for x in make_op(gpu_backend, kind).evaluate([model("tt"), torch.as_tensor(Z[f"tt_mix{k}_ids"], device="cuda")])]
        want = cut(Z[f"tt_mix{k}_{OPS[kind]}_ends"], Z[f"tt_mix{k}_{OPS[kind]}_chars"])
        assert all(np.array_equal(a, b) for a, b in zip(got, blocking)) and bytes(got[2]) == b"".join(want)


# ---------------------------------------------------------------------------------------------- neighbours
@pytest.mark.parametrize("name", ["nfkc", "bytes", "edit"])
def test_tokenizer_then_detokenizer(backend, name):
    """ops.SentencepieceTokenizer -> a dense matrix padded with an id outside the vocabulary -> ops.SentencepieceDetokenizer: what
    the package's decode(encode(row)) gave, recorded as the round-trip golden."""
    from openvino_tokenizers_amd.ops import SentencepieceTokenizer
    z = np.load(G / "golden_sentencepiece.npz")
    ends = z["ends"][:120].astype(np.int32)
    begins = np.concatenate([[0], ends[:-1]]).astype(np.int32)
    keep = np.flatnonzero(ends - begins <= 300)   # (the row of 5 000 bytes has a matrix of its own in the golden)
    long_row = [k for k in range(120) if k not in keep]
    assert len(long_row) == 1
    mdl = model(name)
    idx, val, shape = [backend.host(x) for x in SentencepieceTokenizer(lib=backend.lib).evaluate(
        [mdl] + backend.data([begins[keep], ends[keep], z["chars"][:ends[-1]]]))]
    pad = int(Z[f"{name}_rt_right_ids"].max())
    dense = np.full((int(shape[0]), int(shape[1]) + 2), pad, np.int32)
    dense[idx[:, 0], idx[:, 1]] = val
    # golden row j of rt_right is sentence j with the long row left out
    want = cut(Z[f"{name}_rt_right_dec_ends"], Z[f"{name}_rt_right_dec_chars"])[:len(keep)]
    assert np.array_equal(keep, [k for k in range(120) if k != long_row[0]])
    check(backend, make_op(backend, "decode"), mdl, dense, want, f"round trip {name}")


def test_pipeline_step(backend):
    from openvino_tokenizers_amd.pipeline import Pipeline, SentencepieceDetokenizeStep, fuse
    for stream, key in ((False, "dec"), (True, "str")):
        step = SentencepieceDetokenizeStep(bytes(model("tt")), stream=stream, lib=backend.lib)
        assert fuse([step]) == [step]
        b, e, c = [backend.host(x) for x in Pipeline([step]).run("tokens", backend.data([Z["tt_mix2_ids"]]))]
        assert cut(e, c) == cut(Z[f"tt_mix2_{key}_ends"], Z[f"tt_mix2_{key}_chars"]) and b[0] == 0


def test_live_against_package(emu_lib):
    """Fresh random id matrices through the emulator build against the installed package."""
    spm = pytest.importorskip("sentencepiece")
    from tests.conftest import Backend
    backend = Backend("emu", emu_lib)
    rng = np.random.default_rng(11)
    for name in MODELS:
        mdl = model(name)
        sp = spm.SentencePieceProcessor(model_proto=bytes(mdl))
        V = sp.get_piece_size()
        byte_ids = [i for i in range(V) if sp.is_byte(i)]
        op, sop = make_op(backend, "decode"), make_op(backend, "stream")
        for shape in ((33, 5), (9, 70), (3, 600)):
            ids = rng.integers(0, V + 40, shape).astype(np.int32)
            if byte_ids:   # half of the rows: mostly byte pieces, lead bytes twice as likely
                pool = np.array(byte_ids + [i for i in byte_ids if int(sp.id_to_piece(i)[3:5], 16) >= 0xC2], np.int32)
                dense = rng.random(shape) < 0.75
                dense[1::2] = False
                ids[dense] = pool[rng.integers(0, len(pool), int(dense.sum()))]
            check(backend, op, mdl, ids, [sp.decode([int(x) for x in r if x < V]).encode() for r in ids], f"live {name} {shape}")
            raw = []
            for r in ids:
                pieces = [sp.id_to_piece(int(x)).encode() for x in r if x < V]   # src/sentence_piece.cpp:496-517
                raw.append(b"".join(bytes([int(t[3:5], 16)]) if len(t) == 6 and t[:3] == b"<0x" and t[5:] == b">" else t for t in pieces))
            check(backend, sop, mdl, ids, raw, f"live stream {name} {shape}")


def test_old_detokenizer_unchanged(backend):
    """ovtk_detokenize_run, whose kernels this op's are modelled on and do not touch, still gives the GPT-2 golden's bytes: the CPU
    oracle's VocabDecoder -> FuzeRagged over the same ids, which is what it gave before."""
    from openvino_tokenizers_amd.ops import FusedDetokenizer, VocabDecoder
    from oracle import oracle as O
    from tools.harness import pack_strings
    from tools.make_tokenizers import load_tokenizer
    z = np.load(G / "golden_detok_gpt2_small.npz")
    vocab = load_tokenizer("gpt2_small")["vocab"]
    skip = z["skip_tokens"].tolist()
    r = O.vocab_decoder(z["ids"], vocab, skip)
    fb, fe = O.fuze(r[0], r[1], r[2], r[3])
    got = FusedDetokenizer(VocabDecoder(skip_tokens=skip, lib=backend.lib)).evaluate(backend.data([z["ids"]]) + list(pack_strings(vocab)))
    for want, g in zip((fb, fe, r[4]), got):
        assert np.array_equal(backend.host(g), want)
