"""SentencepieceTokenizer on BPE sentencepiece models (csrc/sp_bpe_kernels.hpp) against the `sentencepiece` package:
tests/gen_golden_sentencepiece_bpe.py recorded its ids for three small BPE models trained in-process, and asserted its plain-Python
restatement of the merge rules against the package on every row.  Every comparison is of whole arrays, no tolerance anywhere.

A wave form of the merge kernel is 64 normalized bytes, a lane per byte; a segment is a stretch between two cuts (in front of a "▁"
that does not follow a "▁"), and the sentence's first one begins with the dummy prefix: "k" * 61 is a segment of 64 bytes."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from tests.test_sentencepiece import OPTIONS, _append_field, _run_raw, check, make_op, pack

G = Path(__file__).resolve().parent / "golden"
MODELS = ("bytes", "unk", "edit")


class Golden:
    def __init__(self):
        z = np.load(G / "golden_sentencepiece_bpe.npz")
        cut = lambda ends, data: [data[x:y] for x, y in zip(np.concatenate([[0], ends[:-1]]), ends)]   # noqa: E731
        self.rows = [bytes(r) for r in cut(z["ends"], z["chars"])]
        self.hand = {str(k): int(v) for k, v in zip(z["hand_names"], z["hand_index"])}
        self.ids = {(m, o): [r.astype(np.int32).tolist() for r in cut(z[f"{m}_{o}_ends"], z[f"{m}_{o}_ids"])] for m in MODELS for o in OPTIONS}
        self.models = {m: np.frombuffer((G / f"spm_bpe_{m}.model").read_bytes(), np.uint8) for m in MODELS}
        self.decoded = [bytes(r) for r in cut(z["bytes_decoded_ends"], z["bytes_decoded_chars"])]


_golden = None


@pytest.fixture(scope="module")
def gold():
    global _golden
    if _golden is None:
        _golden = Golden()
    return _golden


def one(backend, gold, model, name, opt="plain"):
    row = gold.rows[gold.hand[name]]
    want = gold.ids[model, opt][gold.hand[name]]
    check(backend, gold.models[model], [row], [want], f"{name} {model} {opt}", **OPTIONS[opt])
    return want


def leftover_segments(lib, run):
    """What the merge kernel's status block counted for the left-over path during run(), read through the library's profile."""
    lib.ovtk_profile_enable(1)
    try:
        lib.ovtk_profile_reset()
        run()
        n = int(lib.ovtk_profile_dump(None, C.c_int64(0)))
        buf = C.create_string_buffer(n + 1)
        lib.ovtk_profile_dump(buf, C.c_int64(n + 1))
    finally:
        lib.ovtk_profile_enable(0)
    counts = {line.split()[0]: int(line.split()[2]) for line in buf.value.decode().splitlines()}
    assert counts.get("spbpe_merge", 0) >= 1, counts
    return counts.get("spbpe_leftover_segments", 0)


# ---------------------------------------------------------------------------------------------- the package's goldens
@pytest.mark.parametrize("opt", list(OPTIONS))
@pytest.mark.parametrize("model", MODELS)
def test_matches_package_golden(backend, gold, model, opt):
    assert len(gold.rows) == 2000
    check(backend, gold.models[model], gold.rows, gold.ids[model, opt], f"{model} {opt}", **OPTIONS[opt])


def test_live_against_package(emu_lib, gold):
    """Fresh random sentences, invalid UTF-8 among them, through the emulator build against the installed package."""
    spm = pytest.importorskip("sentencepiece")
    from tests.conftest import Backend
    backend = Backend("emu", emu_lib)
    rng = np.random.default_rng(11)
    alphabet = [c.encode() for c in "katomiresuloanbé üñαβдя  \t😀漢ﬁ①Ａaaξψωχ▁▁<>"] + [b"\x80", b"\xe2", b"\xf0\x9f", b"\xff", b"  "]
    rows = [b"".join(alphabet[k] for k in rng.integers(0, len(alphabet), rng.integers(0, 40))) for _ in range(360)]
    rows += [b"".join(alphabet[k] for k in rng.integers(0, 12, n)) for n in range(50, 90)]   # words around a wave form's length
    for model in MODELS:
        sp = spm.SentencePieceProcessor(model_proto=bytes(gold.models[model]))
        for opt, kw in OPTIONS.items():
            check(backend, gold.models[model], rows, [sp.encode(r, **kw) for r in rows], f"live {model} {opt}", **kw)


# ---------------------------------------------------------------------------------------------- hand-made rows
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_batch_sizes(backend, gold, n):
    for model in ("bytes", "unk"):
        check(backend, gold.models[model], gold.rows[50:50 + n], gold.ids[model, "bos_eos"][50:50 + n], f"{n} rows", add_bos=True, add_eos=True)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", ["empty", "two_spaces", "one_byte", "tab_only"])
def test_tiny_rows(backend, gold, model, name):
    for opt in OPTIONS:
        want = one(backend, gold, model, name, opt)
        if name in ("empty", "two_spaces"):
            assert want == {"plain": [], "bos": [1], "eos": [2], "bos_eos": [1, 2], "reverse": []}[opt]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", ["seg_63", "seg_64", "seg_65", "seg_129", "literal_space_symbol", "space_symbols", "two_spaces_inside",
                                  "four_byte_end", "four_byte_at_wave_end", "long_unknowns"])
def test_segment_shapes(backend, gold, model, name):
    """Segments of 1 and 2 symbols ("▁" alone behind a word, "▁k"), of one lane less than a wave form, exactly one, one more and
    two and one more; a four-byte character that ends a segment, and one that would cross a form's last lane."""
    for opt in ("plain", "reverse"):
        one(backend, gold, model, name, opt)


def test_segments_at_and_across_a_form_s_last_lane(backend, gold):
    """Words of 1 .. 70 letters behind one another: segments that end on every lane of a form, the last lane among them, and
    segments that lie across two forms.  The ids of a word do not depend on where it stands."""
    model = gold.models["bytes"]
    words = [b"k" * n for n in range(1, 71)]
    alone = [_ids_of(backend, model, w) for w in words]
    for shift in (0, 1, 2):
        row = b" ".join(words[shift:])
        check(backend, model, [row], [[x for ids in alone[shift:] for x in ids]], f"shift {shift}")


def _ids_of(backend, model, row, **kw):
    got = make_op(backend, **kw).evaluate([model] + backend.data(list(pack([row]))))
    return backend.host(got[1]).tolist()


@pytest.mark.parametrize("name", ["counter", "counter_in_text", "counter_twice", "same_pair_thrice", "chain_8", "chain_9", "chain_23", "chain_10",
                                  "chain_in_text", "inner_space_piece"])
def test_counter_example_and_ties(backend, gold, name):
    """ξψ (-1.25), ξψω (-2.25), ωχ (-3.25): the package merges ξψ, then ξψω, and leaves χ; every local maximum at once would give ξψ ωχ.
    The same candidate at several places of one segment: the leftmost goes first."""
    want = one(backend, gold, "edit", name)
    one(backend, gold, "edit", name, "reverse")
    if name == "counter":
        assert len(want) == 3   # ▁, ξψω, χ


@pytest.mark.parametrize("model", MODELS)
def test_long_segment_takes_the_leftover_path(backend, gold, model):
    name = "long_segment"
    row, want = gold.rows[gold.hand[name]], gold.ids[model, "plain"][gold.hand[name]]
    assert len(row) > 2 * 64 and b" " not in row
    n = leftover_segments(backend.lib, lambda: check(backend, gold.models[model], [row], [want], f"{name} {model}"))
    assert n == 1
    short = gold.rows[gold.hand["one_byte"]]
    assert leftover_segments(backend.lib, lambda: check(backend, gold.models[model], [short], [gold.ids[model, "plain"][gold.hand["one_byte"]]])) == 0
    one(backend, gold, model, "long_segment_in_text", "bos_eos")
    one(backend, gold, model, "row_700", "reverse")


def _piece(text, score_bits):
    return bytes([0x0A, len(text)]) + text + bytes([0x15]) + score_bits   # piece, score; the type stays NORMAL


def test_cuts_on_and_off(backend, gold):
    """`bytes` proves the cut rule; with one more piece that holds "▁" behind another character -- it matches nothing in these rows --
    nothing is a cut and every sentence is one segment.  The ids are the same."""
    off = _append_field(gold.models["bytes"], 1, _piece("♞▁♞".encode(), bytes([0, 0, 0, 0xBF])))   # -0.5: no other piece's score
    rows = gold.rows[300:420] + [gold.rows[gold.hand["long_segment_in_text"]]]
    want = gold.ids["bytes", "plain"][300:420] + [gold.ids["bytes", "plain"][gold.hand["long_segment_in_text"]]]
    assert max(map(len, rows)) > 64
    on_n = leftover_segments(backend.lib, lambda: check(backend, gold.models["bytes"], rows, want, "cuts on"))
    off_n = leftover_segments(backend.lib, lambda: check(backend, off, rows, want, "cuts off"))
    assert off_n > on_n >= 1   # (without cuts every sentence longer than a form is a left-over segment)


def test_offsets_not_from_zero_and_gaps(backend, gold):
    rows = gold.rows[100:140]
    chars, begins, ends = b"\xf0\x9f junk ", [], []
    for r in rows:
        begins.append(len(chars))
        chars += r
        ends.append(len(chars))
        chars += b" \xe2 gap"
    order = np.arange(len(rows))[::-1]   # ... and not ascending either
    strings = (np.array(begins, np.int32)[order], np.array(ends, np.int32)[order], np.frombuffer(chars, np.uint8))
    for model in MODELS:
        check(backend, gold.models[model], None, [gold.ids[model, "plain"][100 + k] for k in order], "offsets", strings=strings)


# ---------------------------------------------------------------------------------------------- the C ABI's edges
def test_capacity(backend, gold):
    from openvino_tokenizers_amd import _lib as L
    op = check(backend, gold.models["unk"], gold.rows[100:120], gold.ids["unk", "plain"][100:120], "capacity")
    need = sum(map(len, gold.ids["unk", "plain"][100:120]))
    rc, n, idx, val, shape = _run_raw(backend.lib, op._h, gold.rows[100:120], need - 1)
    assert rc == L.E_CAPACITY and n == need
    assert (idx == -7).all() and (val == -7).all() and (shape == -7).all()
    rc, n, idx, val, shape = _run_raw(backend.lib, op._h, gold.rows[100:120], need)
    assert rc == 0 and n == need and shape.tolist() == [20, max(map(len, gold.ids["unk", "plain"][100:120]))]


def test_bound_holds(backend, gold):
    """Rows of nothing but unknown characters under byte fallback: an id per byte, the most a sentence can give."""
    rows = ["😀🚀𝔘𓀀".encode() * 5, "漢字".encode() * 11, b"\xff\x80" * 9, "‰".encode()]
    op = make_op(backend, add_bos=True, add_eos=True)
    got = [backend.host(x) for x in op.evaluate([gold.models["bytes"]] + backend.data(list(pack(rows))))]
    per_row = np.bincount(got[0][:, 0], minlength=len(rows))
    assert all(n >= len(r) for n, r in zip(per_row, rows))   # (the dummy prefix and bos / eos on top)
    bound = op.bound(len(rows), sum(map(len, rows)))
    assert len(got[1]) <= bound
    assert op.bound(0, 0) == 0 and backend.lib.ovtk_sentencepiece_bound(op._h, -1, 0) == -1


def test_refusals(backend, gold):
    from openvino_tokenizers_amd import _lib as L
    model = gold.models["bytes"]
    ins = backend.data(list(pack([b"kato"])))

    def refused(m, **kw):
        with pytest.raises(L.OvtkError) as err:
            make_op(backend, **kw).evaluate([m] + ins)
        return err.value

    unused = refused(np.frombuffer((G / "spm_bpe_refuse_unused.model").read_bytes(), np.uint8))
    assert unused.code == L.E_UNSUPPORTED and "UNUSED" in str(unused)
    tie = refused(np.frombuffer((G / "spm_bpe_refuse_tie.model").read_bytes(), np.uint8))
    assert tie.code == L.E_UNSUPPORTED and "share one float32 score" in str(tie)
    for model_type in (3, 4):   # trainer_spec.model_type (3) = WORD, CHAR
        assert refused(_append_field(model, 2, bytes([0x18, model_type]))).code == L.E_UNSUPPORTED
    # what the unigram path refuses, a BPE model is refused for too
    assert refused(_append_field(model, 1, _piece("♞♞".encode(), bytes(4)) + bytes([0x18, 4]))).code == L.E_UNSUPPORTED   # USER_DEFINED
    assert refused(_append_field(model, 2, bytes([0xC0, 0x01, 1]))).code == L.E_UNSUPPORTED   # treat_whitespace_as_suffix
    assert refused(model, nbest_size=5).code == L.E_UNSUPPORTED
    assert refused(model, reverse=True, add_bos=True).code == L.E_UNSUPPORTED
    # a CONTROL piece of one character: PieceToId would answer with it for that character
    assert refused(_append_field(model, 1, _piece("♞".encode(), bytes(4)) + bytes([0x18, 3]))).code == L.E_UNSUPPORTED
    for cut in (0, 1, 7, len(model) // 2, len(model) - 1):
        assert refused(model[:cut]).code == L.E_ARG, cut


# ---------------------------------------------------------------------------------------------- neighbours
def test_pipeline_step_dense(backend, gold):
    from openvino_tokenizers_amd.pipeline import SentencepieceModelStep
    rows, want = gold.rows[200:265], gold.ids["bytes", "bos_eos"][200:265]
    b, e, c = pack(rows)
    rb = np.arange(len(rows), dtype=np.int32)
    step = SentencepieceModelStep(bytes(gold.models["bytes"]), add_bos=True, add_eos=True, pad_id=77, lib=backend.lib)
    kind, (ids, mask) = step.apply("strings", backend.data([rb, rb + 1, b, e, c]) + [None])
    width = max(map(len, want))
    dense, ones = np.full((len(rows), width), 77, np.int32), np.zeros((len(rows), width), np.int32)
    for r, row in enumerate(want):
        dense[r, :len(row)] = row
        ones[r, :len(row)] = 1
    assert kind == "dense" and np.array_equal(backend.host(ids), dense) and np.array_equal(backend.host(mask), ones)


def test_round_trip_through_the_detokenizer(backend, gold):
    """ids of `bytes` from this op -> SentencepieceDetokenizer -> the texts sp.decode gave for the package's ids."""
    from openvino_tokenizers_amd.ops import SentencepieceDetokenizer
    n = len(gold.decoded)
    rows = gold.rows[:n]
    idx, val, shape = [backend.host(x) for x in make_op(backend).evaluate([gold.models["bytes"]] + backend.data(list(pack(rows))))]
    pad = 2   # </s>: a CONTROL piece decodes to nothing
    dense = np.full((int(shape[0]), max(int(shape[1]), 1)), pad, np.int32)
    dense[idx[:, 0], idx[:, 1]] = val
    got = [backend.host(x) for x in SentencepieceDetokenizer(lib=backend.lib).evaluate([gold.models["bytes"], backend.data([dense])[0]])]
    texts = [bytes(got[2][b:e]) for b, e in zip(got[0], got[1])]
    assert texts == gold.decoded
