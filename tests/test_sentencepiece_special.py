"""SentencepieceTokenizer's 8-input form (src/sentence_piece.cpp:200-230, :286-329; csrc/sp_special_kernels.hpp): the added tokens are cut
out of every row as the reference's generated pattern cuts them, the parts are encoded one by one, the tokens' ids stand between them.
tests/gen_golden_sentencepiece_special.py recorded the ids that PCRE2 and the `sentencepiece` package give, and asserted its
literal-matcher restatement equal to PCRE2 on every row.  Every comparison is of whole arrays, no tolerance anywhere."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from tests.gen_golden_sentencepiece_special import MODELS, OPTIONS, TOKEN_LISTS, ids_of_cut, literal_cut, pcre2_cut, word_10_46
from tests.test_sentencepiece import _append_field, pack, sparse_of
from tests.test_sentencepiece import make_op as make_op4

G = Path(__file__).resolve().parent / "golden"
BOS, EOS = 1, 2   # the fixtures' <s> and </s>


def cut_at(ends, data):
    return [data[x:y] for x, y in zip(np.concatenate([[0], ends[:-1]]), ends)]


class Golden:
    def __init__(self):
        z = np.load(G / "golden_sentencepiece_special.npz")
        self.rows = [bytes(r) for r in cut_at(z["ends"], z["chars"])]
        self.row_list = [str(x) for x in z["row_list"]]
        self.hand = {str(k): int(v) for k, v in zip(z["hand_names"], z["hand_index"])}
        self.ids = {(m, o): [r.astype(np.int32).tolist() for r in cut_at(z[f"{m}_{o}_ends"], z[f"{m}_{o}_ids"])] for m in MODELS for o in OPTIONS}
        self.models = {m: np.frombuffer((G / f).read_bytes(), np.uint8) for m, f in MODELS.items()}
        self.tokens = {str(k): ([bytes(t) for t in cut_at(z[f"tok_{k}_ends"], z[f"tok_{k}_chars"])], z[f"tok_{k}_ids"].tolist()) for k in z["list_names"]}
        assert self.tokens == {k: ([t.encode() for t, _ in v], [i for _, i in v]) for k, v in TOKEN_LISTS.items()}

    def of_list(self, which):
        return [k for k, w in enumerate(self.row_list) if w == which]


_golden = None


@pytest.fixture(scope="module")
def gold():
    global _golden
    if _golden is None:
        _golden = Golden()
    return _golden


def make_op(backend, **kw):
    """An op that takes the 8-input form (a default op keeps refusing it: test_existing_forms_are_unchanged)."""
    return make_op4(backend, special_tokens=True, **kw)


def token_inputs(tokens, ids):
    """tok_begins, tok_ends, tok_chars, tok_ids: constants of the graph, host memory."""
    b, e, c = pack(list(tokens))
    return [b, e, c, np.array(ids, np.int32)]


def check8(backend, model, rows, tokens, ids, want, what="", strings=None, op=None, **kw):
    op = op or make_op(backend, **kw)
    b, e, c = strings if strings is not None else pack(rows)
    got = [backend.host(x) for x in op.evaluate([model] + backend.data([b, e, c]) + token_inputs(tokens, ids))]
    ref = sparse_of(want)
    for name, g, r in zip(("indices", "values", "dense_shape"), got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, g.shape, r.shape)
        if not np.array_equal(g, r):
            k = int(np.argwhere(g != r)[0][0])
            raise AssertionError(f"{what}: {name} differs first at {k}: got {g[k]}, want {r[k]}" +
                                 (f" (row {ref[0][k][0]}: {rows[ref[0][k][0]]!r})" if name == "values" and rows else ""))
    return op


def ids4(backend, model, row, **kw):
    """The ids of one sentence from a 4-input call."""
    return backend.host(make_op4(backend, **kw).evaluate([model] + backend.data(list(pack([row]))))[1]).tolist()


def composed(backend, model, row, tokens, ids, add_bos=False, add_eos=False, reverse=False):
    """What the op's loop gives for a row, its parts encoded by 4-input calls of the same backend; the cut by the restatement the
    golden generator asserted equal to PCRE2 (\\w of PCRE2 10.46; malformed UTF-8 by the convention of include/ovtk_amd.h)."""
    out = []
    for kind, v in literal_cut(row, tokens, word_10_46):
        out += ids4(backend, model, v, add_bos=add_bos) if kind == "part" else [ids[v]]
    out += [EOS] if add_eos else []
    return out[::-1] if reverse and len(out) > 1 else out


# ---------------------------------------------------------------------------------------------- PCRE2's and the package's goldens
@pytest.mark.parametrize("opt", list(OPTIONS))
@pytest.mark.parametrize("model", list(MODELS))
def test_matches_golden(backend, gold, model, opt):
    assert len(gold.rows) == 590
    for which, (tokens, ids) in gold.tokens.items():
        at = gold.of_list(which)
        check8(backend, gold.models[model], [gold.rows[k] for k in at], tokens, ids, [gold.ids[model, opt][k] for k in at],
               f"{model} {opt} {which}", **OPTIONS[opt])


def test_live_against_package_and_pcre2(emu_lib, gold):
    """Fresh random rows through the emulator build against the system PCRE2 and the installed package.  The alphabet is the golden
    generator's: nothing on which PCRE2 10.39 and 10.46 differ."""
    spm = pytest.importorskip("sentencepiece")
    from tests.conftest import Backend
    from tests.gen_golden_sentencepiece_special import GLUE, WORDS
    backend = Backend("emu", emu_lib)
    rng = np.random.default_rng(17)
    for which, (tokens, ids) in gold.tokens.items():
        pool = WORDS + GLUE + [t.decode() for t in tokens] * 3
        rows = ["".join(pool[k] for k in rng.integers(0, len(pool), rng.integers(0, 30))).encode() for _ in range(120)]
        cuts = [pcre2_cut(r, tokens) for r in rows]
        assert cuts == [literal_cut(r, tokens) for r in rows]
        for model in MODELS:
            sp = spm.SentencePieceProcessor(model_proto=bytes(gold.models[model]))
            for opt in ("bos_eos", "reverse_bos"):
                check8(backend, gold.models[model], rows, tokens, ids, [ids_of_cut(sp, c, ids, **OPTIONS[opt]) for c in cuts],
                       f"live {model} {opt} {which}", **OPTIONS[opt])


# ---------------------------------------------------------------------------------------------- hand-made rows
HAND = ["people", "sopx", "xsop", "xsopx", "at_start", "at_end", "whole_row", "whole_row_letters", "back_to_back", "spaces_between", "empty",
        "after_digit", "after_underscore", "after_e_acute", "quoted_metacharacters", "parts_63", "parts_64", "parts_65", "long_part_behind_a_cut",
        "ctl_wrapped", "ctl_unk", "ctl_back_to_back", "ctl_empty", "prefix_orders", "prefix_empty", "dup_first_id", "dup_empty", "none_text",
        "none_empty", "none_spaces"]


@pytest.mark.parametrize("name", HAND)
def test_hand_made_rows(backend, gold, name):
    k = gold.hand[name]
    tokens, ids = gold.tokens[gold.row_list[k]]
    for model in MODELS:
        for opt in (OPTIONS if model == "bpe_bytes" else ("plain", "reverse_eos")):
            check8(backend, gold.models[model], [gold.rows[k]], tokens, ids, [gold.ids[model, opt][k]], f"{name} {model} {opt}", **OPTIONS[opt])


def test_hand_made_rows_are_all_listed(gold):
    assert sorted(HAND) == sorted(gold.hand)


def test_what_the_rows_pin(gold):
    """No split inside `people`; one free side is enough and none gives no match; an empty row has no bos; a part of spaces has no
    ids of its own but its bos; the first id of a duplicated token holds; of two tokens at one place the earlier one wins."""
    ids = lambda name, opt="plain": gold.ids["bpe_bytes", opt][gold.hand[name]]   # noqa: E731
    assert ids("people")[-2:] == [9001, 9002] and ids("people").count(9002) == 1   # (the " " between them normalizes to nothing)
    assert ids("sopx")[0] == 9001 and ids("xsop")[-1] == 9001 and 9001 not in ids("xsopx")
    assert ids("whole_row") == [9003] and ids("whole_row", "bos_eos") == [9003, EOS] and ids("whole_row", "reverse_eos") == [EOS, 9003]
    for opt, want in {"plain": [], "bos": [], "eos": [EOS], "bos_eos": [EOS], "reverse": [], "reverse_eos": [EOS], "reverse_bos": []}.items():
        assert ids("empty", opt) == want and ids("none_empty", opt) == want
    assert ids("spaces_between") == [9004, 9003] and ids("spaces_between", "bos") == [9004, BOS, 9003]
    assert ids("spaces_between", "reverse_bos") == [9003, BOS, 9004]
    assert [x for x in ids("dup_first_id") if x in (11, 12, 13)] == [11, 12, 11]
    assert [x for x in ids("prefix_orders") if x in (31, 32, 33, 34)] == [31, 33, 31, 34]
    assert ids("back_to_back").count(9004) == 1 and ids("back_to_back")[ids("back_to_back").index(9004) + 1] == 9003


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_batch_sizes(backend, gold, n):
    tokens, ids = gold.tokens["chat"]
    at = gold.of_list("chat")[20:20 + n]
    for model in ("bpe_bytes", "nfkc"):
        check8(backend, gold.models[model], [gold.rows[k] for k in at], tokens, ids, [gold.ids[model, "bos_eos"][k] for k in at], f"{n} rows",
               add_bos=True, add_eos=True)


def test_offsets_not_from_zero_and_gaps(backend, gold):
    tokens, ids = gold.tokens["chat"]
    at = gold.of_list("chat")[:40]
    chars, begins, ends = b"\xf0\x9f sop ", [], []
    for k in at:
        begins.append(len(chars))
        chars += gold.rows[k]
        ends.append(len(chars))
        chars += b"x\xe2 [INST] gap "   # (a letter against the row's end: \b looks at the row, not at the tensor)
    order = np.arange(len(at))[::-1]   # ... and not ascending either
    strings = (np.array(begins, np.int32)[order], np.array(ends, np.int32)[order], np.frombuffer(chars, np.uint8))
    for model in MODELS:
        check8(backend, gold.models[model], None, tokens, ids, [gold.ids[model, "reverse_eos"][at[k]] for k in order], "offsets", strings=strings,
               reverse=True, add_eos=True)


def test_every_part_gets_its_own_dummy_prefix(backend, gold):
    """The ids of A<s>B are the ids of A, the token's id, the ids of B, each from a 4-input call."""
    tokens, ids = gold.tokens["ctl"]
    for model in MODELS:
        m = gold.models[model]
        a, b = ids4(backend, m, b"kato mire"), ids4(backend, m, b"mire kato")
        whole = ids4(backend, m, b"kato miremire kato")
        assert a + b != whole   # (B alone begins with the dummy prefix)
        check8(backend, m, [b"kato mire<s>mire kato"], tokens, ids, [a + [1] + b], model)
        a1, b1 = ids4(backend, m, b"kato mire", add_bos=True), ids4(backend, m, b"mire kato", add_bos=True)
        check8(backend, m, [b"kato mire<s>mire kato"], tokens, ids, [a1 + [1] + b1 + [EOS]], model, add_bos=True, add_eos=True)


def test_a_nonspacing_mark_is_a_word_character(backend, gold):
    """U+0301 (Mn) behind `sop`: a word character under PCRE2 10.46, which the reference pins, so `xsoṕ` holds no match.  The
    expected value is the restatement's with \\w = L | N | Mn | Pc -- NOT the system PCRE2's, which is 10.39 and knows no Mn in \\w.
    A connector other than "_" (U+203F, Pc) likewise."""
    tokens, ids = gold.tokens["chat"]
    for tail in ("́", "‿"):
        row = f"xsop{tail} sop{tail} .sop".encode()
        cut = literal_cut(row, tokens, word_10_46)
        assert [k for k, _ in cut] == ["part", "tok", "part", "tok"] and cut[0][1] == f"xsop{tail} ".encode()   # (`sop` + tail: free in front)
        for model in MODELS:
            for opt in ("plain", "reverse_eos"):
                check8(backend, gold.models[model], [row], tokens, ids, [composed(backend, gold.models[model], row, tokens, ids, **OPTIONS[opt])],
                       f"Mn {model} {opt}", **OPTIONS[opt])


def test_malformed_utf8_rows(backend, gold):
    """Undefined in the reference (pcre2_jit_match does not validate); here by SpecialTokensSplit's convention (include/ovtk_amd.h):
    no match begins at a continuation byte, a stray byte is no word character.  The emulator and the GPU agree with the restatement."""
    tokens, ids = gold.tokens["chat"]
    rows = [b"\x80sop", b"\xc3sop", b"\xc3\xa9sop\xc3", b"sop\xa9x", b"x\xe2\x96sop", b"\xf0\x9f\x98sop\xf0\x9f\x98\x80", b"\xffsopx", b"sop\xc3",
            b"\xe2\x96\x81sopk", b"k\xa9[INST]\xe9", b"\xf8\x88\x80\x80sopx", b"\xc3\xa9sopx", b"\xe9sopx \xe9\xa9sopx"]
    tokens2 = tokens + [b"\xc3\xa9s"]   # a token that begins with a lead byte
    ids2 = ids + [9006]
    for model in ("bpe_bytes", "nfkc"):
        want = [composed(backend, gold.models[model], r, tokens2, ids2, add_eos=True) for r in rows]
        check8(backend, gold.models[model], rows, tokens2, ids2, want, f"malformed {model}", add_eos=True)


# ---------------------------------------------------------------------------------------------- the C ABI's edges
def _run_raw8(lib, h, rows, capacity, fill=-7):
    from openvino_tokenizers_amd import _lib as L
    b, e, c = pack(rows)
    s = L.Strings(b.ctypes.data, e.ctypes.data, c.ctypes.data if c.size else None, len(b), len(c))
    idx, val, shape = np.full(2 * max(capacity, 1), fill, np.int64), np.full(max(capacity, 1), fill, np.int32), np.full(2, fill, np.int64)
    out = L.SparseI32Out(idx.ctypes.data, val.ctypes.data, shape.ctypes.data, capacity, 0)
    rc = lib.ovtk_sentencepiece_run(h, C.byref(s), C.byref(out), L.MEM_HOST, None)
    return rc, int(out.n), idx, val, shape


def test_capacity(backend, gold):
    from openvino_tokenizers_amd import _lib as L
    tokens, ids = gold.tokens["chat"]
    at = gold.of_list("chat")[:30]
    rows, want = [gold.rows[k] for k in at], [gold.ids["bpe_unk", "reverse_eos"][k] for k in at]
    op = check8(backend, gold.models["bpe_unk"], rows, tokens, ids, want, "capacity", reverse=True, add_eos=True)
    need = sum(map(len, want))
    rc, n, idx, val, shape = _run_raw8(backend.lib, op._h, rows, need - 1)
    assert rc == L.E_CAPACITY and n == need
    assert (idx == -7).all() and (val == -7).all() and (shape == -7).all()
    rc, n, idx, val, shape = _run_raw8(backend.lib, op._h, rows, need)
    assert rc == 0 and n == need and shape.tolist() == [30, max(map(len, want))]
    assert val[:n].tolist() == [x for r in want for x in r]


def test_bound_holds(backend, gold):
    """Rows of nothing but tokens, and single characters between tokens -- every part pays a dummy prefix and a bos, under byte fallback
    every unknown byte an id -- under bos + eos."""
    tokens, ids = [b"#", b"<|x|>"], [9001, 9004]   # (the shortest token: one byte)
    rows = [b"#" * 40, b"<|x|>" * 9, ".#" * 30 + ".", "😀#" * 12, "漢#字#" * 6, b"\xff#\x80#" * 8, b"", b"#"]
    rows = [r if isinstance(r, bytes) else r.encode() for r in rows]
    m = gold.models["bpe_bytes"]
    op = make_op(backend, add_bos=True, add_eos=True)
    got = [backend.host(x) for x in op.evaluate([m] + backend.data(list(pack(rows))) + token_inputs(tokens, ids))]
    want = [composed(backend, m, r, tokens, ids, add_bos=True, add_eos=True) for r in rows]
    assert got[1].tolist() == [x for r in want for x in r]
    assert len(want[0]) == 41 and len(want[2]) >= 31 * 2 + 30 + 1   # (tokens only: an id each; a part ".": bos and at least one id)
    for k in range(len(rows)):   # row by row and the batch
        assert len(want[k]) <= op.bound(1, len(rows[k])), rows[k]
    assert len(got[1]) <= op.bound(len(rows), sum(map(len, rows)))
    assert op.bound(0, 0) == 0 and backend.lib.ovtk_sentencepiece_bound(op._h, -1, 0) == -1


def test_refusals(backend, gold):
    from openvino_tokenizers_amd import _lib as L
    model = gold.models["bpe_bytes"]
    ins = backend.data(list(pack([b"kato"])))

    def refused(m, tokens, ids=None, **kw):
        with pytest.raises(L.OvtkError) as err:
            make_op(backend, **kw).evaluate([m] + ins + token_inputs(tokens, ids if ids is not None else list(range(len(tokens)))))
        return err.value

    empty = refused(model, [b"<s>", b"", b"</s>"])
    assert empty.code == L.E_UNSUPPORTED and "empty" in str(empty)
    for bad in (b"\xff", b"<\xc3>", b"\xed\xa0\x80", b"\xc0\xaf", b"\xf4\x90\x80\x80", b"abc\xe2\x96"):
        err = refused(model, [b"<s>", bad])
        assert err.code == L.E_UNSUPPORTED and "UTF-8" in str(err), bad
    assert refused(model, [b"<%d>" % k for k in range(4097)]).code == L.E_UNSUPPORTED
    assert refused(model, [b"x" * 1024]).code == L.E_UNSUPPORTED
    negative = refused(model, [b"<s>", b"</s>"], [1, -1])   # (the reference would emit -1; the slot lists keep negative ids for parts)
    assert negative.code == L.E_UNSUPPORTED and "negative" in str(negative)
    no_eos = _append_field(model, 2, bytes([0xFA, 0x02, 3]) + b"<z>")   # trainer_spec.eos_piece (47) = "<z>": no such piece
    assert refused(no_eos, [b"<s>"], add_eos=True).code == L.E_UNSUPPORTED
    assert refused(model, [b"<s>"], nbest_size=5).code == L.E_UNSUPPORTED
    # a model refused in the 4-input form is refused here too
    assert refused(np.frombuffer((G / "spm_bpe_refuse_tie.model").read_bytes(), np.uint8), [b"<s>"]).code == L.E_UNSUPPORTED
    assert refused(_append_field(model, 2, bytes([0x18, 4])), [b"<s>"]).code == L.E_UNSUPPORTED   # trainer_spec.model_type = CHAR
    assert refused(model[:len(model) // 2], [b"<s>"]).code == L.E_ARG
    # the limits themselves run: 1 024 tokens of 1 023 bytes and more
    many = [b"<%04d>" % k + b"y" * 1017 for k in range(1024)]
    assert len(many[0]) == 1023
    row = b"kato" + many[1000] + b"mire" + many[3][:-1]
    check8(backend, model, [row], many, list(range(20000, 21024)),
           [ids4(backend, model, b"kato") + [21000] + ids4(backend, model, b"mire" + many[3][:-1])], "limits")


def test_existing_forms_are_unchanged(backend, gold):
    from openvino_tokenizers_amd import _lib as L
    from tests.test_sentencepiece_bpe import Golden as BpeGolden
    old = BpeGolden()
    rows, want = old.rows[100:160], old.ids["bytes", "bos_eos"][100:160]
    got = [backend.host(x) for x in make_op4(backend, add_bos=True, add_eos=True).evaluate([old.models["bytes"]] + backend.data(list(pack(rows))))]
    for g, r in zip(got, sparse_of(want)):
        assert np.array_equal(g, r)
    ins = backend.data(list(pack([b"kato"])))
    for n_inputs in (2, 6):
        with pytest.raises(L.OvtkError) as err:
            make_op(backend).evaluate(([gold.models["nfkc"]] + ins + ins)[:n_inputs])
        assert err.value.code == L.E_ARG
    with pytest.raises(L.OvtkError) as err:   # an op made without special_tokens=True answers 8 inputs as it always did
        make_op4(backend).evaluate(([gold.models["nfkc"]] + ins + ins + ins)[:8])
    assert err.value.code == L.E_UNSUPPORTED
    op8 = check8(backend, gold.models["nfkc"], [b"kato"], [b"kato"], [0], [[0]], "the same 8 inputs, opted in")
    # the handle is made at the first evaluate, for that call's form: the other form on the same op is an error, never the wrong answer
    with pytest.raises(L.OvtkError) as err:
        op8.evaluate([gold.models["nfkc"]] + ins)
    assert err.value.code == L.E_ARG
    op4 = make_op(backend)
    op4.evaluate([gold.models["nfkc"]] + ins)
    with pytest.raises(L.OvtkError) as err:
        op4.evaluate([gold.models["nfkc"]] + ins + token_inputs([b"kato"], [0]))
    assert err.value.code == L.E_ARG
    with pytest.raises(L.OvtkError) as err:   # reverse + add_bos: refused in the 4-input form only
        make_op4(backend, reverse=True, add_bos=True).evaluate([gold.models["nfkc"]] + ins)
    assert err.value.code == L.E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- neighbours
def test_pipeline_step_dense(backend, gold):
    from openvino_tokenizers_amd.pipeline import SentencepieceModelStep
    at = gold.of_list("chat")[:65]
    rows, want = [gold.rows[k] for k in at], [gold.ids["bpe_bytes", "bos_eos"][k] for k in at]
    b, e, c = pack(rows)
    rb = np.arange(len(rows), dtype=np.int32)
    step = SentencepieceModelStep(bytes(gold.models["bpe_bytes"]), add_bos=True, add_eos=True, pad_id=77, lib=backend.lib,
                                  special_tokens=TOKEN_LISTS["chat"])
    kind, (ids, mask) = step.apply("strings", backend.data([rb, rb + 1, b, e, c]) + [None])
    width = max(map(len, want))
    dense, ones = np.full((len(rows), width), 77, np.int32), np.zeros((len(rows), width), np.int32)
    for r, row in enumerate(want):
        dense[r, :len(row)] = row
        ones[r, :len(row)] = 1
    assert kind == "dense" and np.array_equal(backend.host(ids), dense) and np.array_equal(backend.host(mask), ones)
