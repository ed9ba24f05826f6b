"""SentencepieceTokenizer for unigram models (src/sentence_piece.cpp:188-350, 4-input form) and RaggedToSparse
(src/ragged_to_sparse.cpp:27-47) against the `sentencepiece` package: tests/gen_golden_sentencepiece.py recorded its ids for three
small models trained in-process.  Every comparison is of whole arrays, no tolerance anywhere."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

G = Path(__file__).resolve().parent / "golden"
MODELS = ("nfkc", "bytes", "edit")
OPTIONS = {"plain": {}, "bos": {"add_bos": True}, "eos": {"add_eos": True}, "bos_eos": {"add_bos": True, "add_eos": True}, "reverse": {"reverse": True}}
UNK = 0   # the fixtures' <unk>


class Golden:
    def __init__(self):
        z = np.load(G / "golden_sentencepiece.npz")
        cut = lambda ends, data: [data[x:y] for x, y in zip(np.concatenate([[0], ends[:-1]]), ends)]   # noqa: E731
        self.rows = [bytes(r) for r in cut(z["ends"], z["chars"])]
        self.hand = {str(k): int(v) for k, v in zip(z["hand_names"], z["hand_index"])}
        self.ids = {(m, o): [r.astype(np.int32).tolist() for r in cut(z[f"{m}_{o}_ends"], z[f"{m}_{o}_ids"])] for m in MODELS for o in OPTIONS}
        self.models = {m: np.frombuffer((G / f"spm_unigram_{m}.model").read_bytes(), np.uint8) for m in MODELS}
        self.unused = [str(x) for x in z["edit_unused"]]


_golden = None


@pytest.fixture(scope="module")
def gold():
    global _golden
    if _golden is None:
        _golden = Golden()
    return _golden


def pack(rows):
    ends = np.cumsum([len(r) for r in rows], dtype=np.int64).astype(np.int32) if rows else np.zeros(0, np.int32)
    begins = np.concatenate([[0], ends[:-1]]).astype(np.int32) if rows else np.zeros(0, np.int32)
    return begins, ends, np.frombuffer(b"".join(rows), np.uint8)


def sparse_of(ids):
    """src/sentence_piece.cpp:331-347 over the rows' ids."""
    indices = np.array([(r, k) for r, row in enumerate(ids) for k in range(len(row))], np.int64).reshape(-1, 2)
    values = np.array([x for row in ids for x in row], np.int32)
    return indices, values, np.array([len(ids), max(map(len, ids), default=0)], np.int64)


def make_op(backend, **kw):
    from openvino_tokenizers_amd.ops import SentencepieceTokenizer
    return SentencepieceTokenizer(lib=backend.lib, **kw)


def check(backend, model, rows, want, what="", strings=None, op=None, **kw):
    op = op or make_op(backend, **kw)
    b, e, c = strings if strings is not None else pack(rows)
    got = [backend.host(x) for x in op.evaluate([model] + backend.data([b, e, c]))]
    ref = sparse_of(want)
    for name, g, r in zip(("indices", "values", "dense_shape"), got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, g.shape, r.shape)
        if not np.array_equal(g, r):
            k = int(np.argwhere(g != r)[0][0])
            raise AssertionError(f"{what}: {name} differs first at {k}: got {g[k]}, want {r[k]}" +
                                 (f" (row {ref[0][k][0]}: {rows[ref[0][k][0]]!r})" if name == "values" and rows else ""))
    return op


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
    rng = np.random.default_rng(7)
    alphabet = [c.encode() for c in "katomiresuloanbé üñαβдя  \t😀漢ﬁ①Ａaξψ▁<>"] + [b"\x80", b"\xe2", b"\xf0\x9f", b"\xff", b"  "]
    rows = [b"".join(alphabet[k] for k in rng.integers(0, len(alphabet), rng.integers(0, 40))) for _ in range(400)]
    for model in MODELS:
        sp = spm.SentencePieceProcessor(model_proto=bytes(gold.models[model]))
        for opt, kw in OPTIONS.items():
            check(backend, gold.models[model], rows, [sp.encode(r, **kw) for r in rows], f"live {model} {opt}", **kw)


# ---------------------------------------------------------------------------------------------- hand-made rows
def one(backend, gold, model, name, opt="plain"):
    row = gold.rows[gold.hand[name]]
    want = gold.ids[model, opt][gold.hand[name]]
    check(backend, gold.models[model], [row], [want], f"{name} {model} {opt}", **OPTIONS[opt])
    return want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_batch_sizes(backend, gold, n):
    for model in ("nfkc", "bytes"):
        check(backend, gold.models[model], gold.rows[50:50 + n], gold.ids[model, "bos_eos"][50:50 + n], f"{n} rows", add_bos=True, add_eos=True)


@pytest.mark.parametrize("model", ["nfkc", "bytes"])
@pytest.mark.parametrize("name", ["empty", "two_spaces", "one_byte"])
def test_tiny_rows(backend, gold, model, name):
    """An empty normalized sentence has no ids of its own; bos and eos still stand (pinned from the package)."""
    for opt in OPTIONS:
        want = one(backend, gold, model, name, opt)
        if name != "one_byte":
            assert want == {"plain": [], "bos": [1], "eos": [2], "bos_eos": [1, 2], "reverse": []}[opt]


def test_all_rows_empty(backend, gold):
    check(backend, gold.models["nfkc"], [b"", b"  ", b""], [[], [], []], "no ids at all")   # dense_shape {3, 0}


def test_longer_after_normalization(backend, gold):
    one(backend, gold, "nfkc", "longer_normalized")
    one(backend, gold, "bytes", "longer_normalized")


@pytest.mark.parametrize("model", ["nfkc", "bytes"])
@pytest.mark.parametrize("name", ["unknown_first", "unknown_last"])
def test_unknown_at_the_edges(backend, gold, model, name):
    want = one(backend, gold, model, name)
    edge = want[-4:] if name == "unknown_last" else want[:5]   # (behind the dummy prefix; four byte pieces under byte fallback)
    assert UNK in edge[-1:] + edge[:2] if model == "nfkc" else sum(3 <= x < 259 for x in edge) == 4


def test_unknowns_apart_do_not_merge(backend, gold):
    assert one(backend, gold, "nfkc", "unknowns_apart").count(UNK) == 4
    one(backend, gold, "bytes", "unknowns_apart")


def test_unknown_run_of_four_byte_characters(backend, gold):
    assert one(backend, gold, "nfkc", "unknown_run_4byte").count(UNK) == 1
    assert sum(3 <= x < 259 for x in one(backend, gold, "bytes", "unknown_run_4byte")) == 16


@pytest.mark.parametrize("model", ["nfkc", "bytes"])
@pytest.mark.parametrize("name", ["control_as_text", "byte_piece_as_text", "literal_space_symbol"])
def test_special_pieces_are_ordinary_text(backend, gold, model, name):
    want = one(backend, gold, model, name)
    if name == "control_as_text":
        assert 1 not in want and 2 not in want   # <s> and </s> written in a sentence are characters
    if name == "byte_piece_as_text" and model == "bytes":
        assert want.count(3 + 0x41) == 1   # the letter A of "<0x0A>" and nothing else: "<0x41>" is six characters


@pytest.mark.parametrize("model", ["nfkc", "bytes"])
@pytest.mark.parametrize("name", ["lone_continuation", "truncated_lead"])
def test_malformed_utf8(backend, gold, model, name):
    one(backend, gold, model, name)


def test_unused_piece_that_would_have_won(backend, gold):
    single, multi = gold.unused
    assert len(single) == 1 and len(multi) >= 3
    pick = [k for k, r in enumerate(gold.rows[:600]) if multi.replace("▁", " ").strip().encode() in r][:8]
    assert pick, "no golden row holds the UNUSED piece"
    differs = [k for k in pick if gold.ids["edit", "plain"][k] != gold.ids["bytes", "plain"][k]]
    assert differs, "the UNUSED piece changes no golden row"
    check(backend, gold.models["edit"], [gold.rows[k] for k in pick], [gold.ids["edit", "plain"][k] for k in pick], "unused")


def test_chain_takes_the_leftover_path(backend, gold):
    """a, aa, ... to ten pieces: a position with more matches than an edge list holds."""
    one(backend, gold, "edit", "chain_10")
    one(backend, gold, "edit", "chain_in_text")
    one(backend, gold, "edit", "chain_in_text", "reverse")


def test_equal_sums_tie(backend, gold):
    want = one(backend, gold, "edit", "tie")
    assert len(want) == 2   # "▁", then the piece from the earlier start
    one(backend, gold, "edit", "tie_in_text")


@pytest.mark.parametrize("model", ["nfkc", "bytes"])
def test_row_of_5000_bytes(backend, gold, model):
    assert len(gold.rows[gold.hand["row_5000"]]) > 4096
    one(backend, gold, model, "row_5000", "bos_eos")


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
    for model in ("nfkc", "bytes"):
        check(backend, gold.models[model], None, [gold.ids[model, "plain"][100 + k] for k in order], "offsets", strings=strings)


# ---------------------------------------------------------------------------------------------- the C ABI's edges
def _run_raw(lib, h, rows, capacity, fill=-7):
    from openvino_tokenizers_amd import _lib as L
    b, e, c = pack(rows)
    s = L.Strings(b.ctypes.data, e.ctypes.data, c.ctypes.data if c.size else None, len(b), len(c))
    idx, val, shape = np.full(2 * max(capacity, 1), fill, np.int64), np.full(max(capacity, 1), fill, np.int32), np.full(2, fill, np.int64)
    out = L.SparseI32Out(idx.ctypes.data, val.ctypes.data, shape.ctypes.data, capacity, 0)
    rc = lib.ovtk_sentencepiece_run(h, C.byref(s), C.byref(out), L.MEM_HOST, None)
    return rc, int(out.n), idx, val, shape


def test_capacity(backend, gold):
    from openvino_tokenizers_amd import _lib as L
    op = check(backend, gold.models["nfkc"], gold.rows[100:120], gold.ids["nfkc", "plain"][100:120], "capacity")
    need = sum(map(len, gold.ids["nfkc", "plain"][100:120]))
    rc, n, idx, val, shape = _run_raw(backend.lib, op._h, gold.rows[100:120], need - 1)
    assert rc == L.E_CAPACITY and n == need
    assert (idx == -7).all() and (val == -7).all() and (shape == -7).all()
    rc, n, idx, val, shape = _run_raw(backend.lib, op._h, gold.rows[100:120], need)
    assert rc == 0 and n == need and shape.tolist() == [20, max(map(len, gold.ids["nfkc", "plain"][100:120]))]


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


def _append_field(model, outer, payload):
    """The model with one more sub-message field: protobuf merges it into the one already there."""
    assert len(payload) < 128
    return np.concatenate([model, np.frombuffer(bytes([outer << 3 | 2, len(payload)]) + payload, np.uint8)])


def test_refusals(backend, gold):
    from openvino_tokenizers_amd import _lib as L
    model = gold.models["bytes"]
    ins = backend.data(list(pack([b"kato"])))

    def code(m, n_inputs=4, **kw):
        with pytest.raises(L.OvtkError) as err:
            make_op(backend, **kw).evaluate(([m] + ins + ins + ins)[:n_inputs])
        return err.value.code

    assert code(np.frombuffer((G / "spm_refuse_bpe.model").read_bytes(), np.uint8)) == L.E_UNSUPPORTED
    piece = "♞♞".encode()
    user_defined = bytes([0x0A, len(piece)]) + piece + bytes([0x15, 0, 0, 0, 0, 0x18, 4])   # piece, score 0.0, type USER_DEFINED
    assert code(_append_field(model, 1, user_defined)) == L.E_UNSUPPORTED
    assert code(_append_field(model, 2, bytes([0xC0, 0x01, 1]))) == L.E_UNSUPPORTED   # trainer_spec.treat_whitespace_as_suffix (24) = true
    assert code(model, nbest_size=5) == L.E_UNSUPPORTED
    assert code(model, reverse=True, add_bos=True) == L.E_UNSUPPORTED
    assert code(model, reverse=True, add_eos=True) == L.E_UNSUPPORTED
    assert code(model, n_inputs=8) == L.E_UNSUPPORTED
    assert code(model, n_inputs=2) == L.E_ARG
    assert code(model, n_inputs=6) == L.E_ARG
    for cut in (0, 1, 7, len(model) // 2, len(model) - 1):
        assert code(model[:cut]) == L.E_ARG, cut
    # an appended, well-formed unknown field changes nothing
    check(backend, _append_field(model, 9, b"abc"), [b"kato mire"], [_ids_of(backend, model, b"kato mire")], "unknown field")


def _ids_of(backend, model, row):
    got = make_op(backend).evaluate([model] + backend.data(list(pack([row]))))
    return backend.host(got[1]).tolist()


# ---------------------------------------------------------------------------------------------- RaggedToSparse
@pytest.mark.parametrize("case", ["0", "1", "65", "empty_rows", "offset"])
def test_ragged_to_sparse(backend, case):
    from openvino_tokenizers_amd.ops import RaggedToSparse
    rng = np.random.default_rng(3)
    lens = {"0": [], "1": [5], "65": rng.integers(0, 200, 65).tolist(), "empty_rows": [3, 0, 0, 70, 0, 1], "offset": [2, 129, 0, 4]}[case]
    ends = np.cumsum(lens, dtype=np.int64).astype(np.int32) + (17 if case == "offset" else 0)
    begins = (ends - np.array(lens, np.int32)).astype(np.int32)
    # src/ragged_to_sparse.cpp:38-45
    want = np.array([(i, j) for i in range(len(begins)) for j in range(ends[i] - begins[i])], np.int32).reshape(-1, 2)
    (got,) = RaggedToSparse(lib=backend.lib).evaluate(backend.data([begins, ends]))
    got = backend.host(got)
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------- neighbours
def test_unigram_op_unchanged(backend):
    """The kernels shared with UnigramTokenizer still give its golden ids."""
    from openvino_tokenizers_amd.ops import UnigramTokenizer
    z = np.load(G / "golden_unigram_small.npz")
    n = len(z["ends"])
    begins = np.concatenate([[0], z["ends"][:-1]]).astype(np.int32)
    vb = np.concatenate([[0], z["vocab_ends"][:-1]]).astype(np.int32)
    rb = np.arange(n, dtype=np.int32)
    op = UnigramTokenizer(unk_token_id=int(z["unk_id"]), lib=backend.lib)
    got = op.evaluate(backend.data([rb, rb + 1, begins, z["ends"].astype(np.int32), z["chars"]]) +
                      [vb, z["vocab_ends"].astype(np.int32), z["vocab_chars"], z["scores"]])
    assert np.array_equal(backend.host(got[1]), z["id_ends"]) and np.array_equal(backend.host(got[2]), z["ids"])


def test_pipeline_step_dense(backend, gold):
    from openvino_tokenizers_amd.pipeline import SentencepieceModelStep
    rows, want = gold.rows[200:265], gold.ids["nfkc", "bos_eos"][200:265]
    b, e, c = pack(rows)
    rb = np.arange(len(rows), dtype=np.int32)
    step = SentencepieceModelStep(bytes(gold.models["nfkc"]), add_bos=True, add_eos=True, pad_id=77, lib=backend.lib)
    kind, (ids, mask) = step.apply("strings", backend.data([rb, rb + 1, b, e, c]) + [None])
    width = max(map(len, want))
    dense, ones = np.full((len(rows), width), 77, np.int32), np.zeros((len(rows), width), np.int32)
    for r, row in enumerate(want):
        dense[r, :len(row)] = row
        ones[r, :len(row)] = 1
    assert kind == "dense" and np.array_equal(backend.host(ids), dense) and np.array_equal(backend.host(mask), ones)
