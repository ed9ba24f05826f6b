"""Sentence pairs in one call (ovtk_encode_pair_dense_* / ovtk_wordpiece_encode_pair_dense_enqueue; ops.FusedPairEncodeDense,
ops.FusedPairWordpieceDense): the encode on the n first rows followed by the n second ones, and the tail the reference's
add_second_input builds (python/openvino_tokenizers/tokenizer_transformations.py:22-304) written by the encode's last pass.

Expected values come from the oracle alone: its ragged ids of the 2n rows -> O.truncate on the halves (src/truncate.cpp:69-144) ->
O.combine_segments with five segments and their type ids (src/combine_segments.cpp:36-134) -> O.ragged_to_dense three times
(src/ragged_to_dense.cpp:70-174).  Whole arrays, no tolerance."""
from functools import lru_cache

import numpy as np
import pytest

from openvino_tokenizers_amd import _lib as L
from openvino_tokenizers_amd import ops as K
from oracle import oracle as O
from tests.placement import Arena
from tests.util import BpeTok, one_string_per_row, pack_strings
from tools.make_tokenizers import load_tokenizer
from tools.workloads import TextModel

MODES = ["only_first", "only_second", "longest_first"]
SIDES = ["right", "left"]
MAX_LENGTHS = [0, 1, 9, 16]
# 5 rows: a 4-row work item of the last pass straddles the boundary between first and second rows; 65: a 64-row tile does; 300: the
# span kernel's path
ROW_COUNTS = [1, 3, 5, 65, 300]
CONSTANTS = [((), (), ()), ((101,), (102,), (103,)), ((0,), (2, 2), (2,))]   # (the last: RoBERTa's <s> A </s></s> B </s>)
TYPE_IDS = [5, 0, 6, 1, 7]
PAD, TYPE_PAD = 50256, 9
SPECIAL = b"<|endoftext|>"
KINDS = ["bpe", "bpe-special", "wordpiece"]


def u8(s):
    return np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), np.uint8)


# ------------------------------------------------------------------------------------------------------------------ the batches
@lru_cache(maxsize=None)
def _stream():
    _, _, c = TextModel(4242, "zipf").batch(1, 60000)
    return c.tobytes().lower()


def pair_texts(n, seed, special=False):
    """n first and n second texts of 0..~20 tokens.  Row 0: an empty first text; row 1: an empty second one; row 2: both empty (n = 1: the
    one pair is ordinary); row 3: the same text twice, long enough to be cut -- a tie; the rest: lengths drawn independently, so that
    long / short, short / long and long / long pairs all occur."""
    rng = np.random.default_rng(seed * 1000 + n)
    text = _stream()

    def draw(lo, hi):
        k = int(rng.integers(lo, hi + 1))
        at = int(rng.integers(0, len(text) - k))
        s = text[at:at + k].strip()
        if special and s and rng.integers(4) == 0:
            cut = int(rng.integers(0, len(s) + 1))
            s = s[:cut] + SPECIAL + s[cut:]
        return s
    first = [draw(0, 90) if rng.integers(3) else draw(0, 12) for _ in range(n)]
    second = [draw(0, 90) if rng.integers(3) else draw(0, 12) for _ in range(n)]
    if n >= 3:
        first[0], second[0] = b"", draw(30, 60)
        first[1], second[1] = draw(30, 60), b""
        first[2], second[2] = b"", b""
    if n >= 5:
        first[3] = second[3] = draw(70, 90)
    return first, second


@lru_cache(maxsize=None)
def bpe_tok():
    return BpeTok.load("gpt2_small")


@lru_cache(maxsize=None)
def bert_tok():
    return load_tokenizer("bert_small")


def special_pattern():
    return O.special_tokens_pattern([(SPECIAL.decode(), False, False)])


def oracle_ragged_ids(kind, strings):
    """The oracle's ragged ids of the rows (the ops' front: [SpecialTokensSplit ->] RegexSplit -> BPETokenizer, or the BERT chain)."""
    rows = len(strings)
    if not any(strings):   # (no text: the ragged tensor's one-row quirk is not the dense tensors' -- every row has no ids)
        return np.zeros(rows, np.int32), np.zeros(rows, np.int32), np.zeros(1, np.int32)
    inputs = one_string_per_row(strings)
    if kind == "wordpiece":
        from tests.test_ops_parity import bert_words
        tok = bert_tok()
        rb, re_, ids = O.WordpieceTokenizer(tok["vocab"], tok["suffix_indicator"], tok["max_bytes_per_word"])(*bert_words(inputs), tok["unk_id"])
    elif kind == "bpe-special":
        s = O.SpecialTokensSplit(special_pattern())(*inputs)
        rb, re_, ids = bpe_tok().oracle()(*O.RegexSplit(bpe_tok().pattern, "isolate")(*s[:5], skips=s[5])[:5])
    else:
        rb, re_, ids = bpe_tok().oracle()(*O.RegexSplit(bpe_tok().pattern, "isolate")(*inputs)[:5])
    assert len(rb) == rows
    return np.asarray(rb, np.int32), np.asarray(re_, np.int32), np.concatenate([np.asarray(ids, np.int32), np.zeros(1, np.int32)])


@lru_cache(maxsize=None)
def batch(kind, n, seed=7, ordinary=True):
    """-> (strings of the 2n rows, the oracle's ragged ids of them); computed once, shared and left unchanged."""
    if n == 1 and not ordinary:
        first, second = [b""], [b""]
    else:
        first, second = pair_texts(n, seed, special=kind == "bpe-special")
    strings = first + second
    rb, re_, ids = oracle_ragged_ids(kind, strings)
    for a in (rb, re_, ids):
        a.setflags(write=False)
    return strings, (rb, re_, ids)


def const_segment(v):
    return np.zeros(1, np.int32), np.full(1, len(v), np.int32), np.asarray(list(v) + [0], np.int32)


def expected(ragged, n, max_length, side, mode, consts, pad_right, target):
    """The oracle's chain behind the ragged ids.  target: None, or a function of the longest combined row."""
    rb, re_, ids = ragged
    (ab, ae), (bb, be) = O.truncate([(rb[:n], re_[:n]), (rb[n:], re_[n:])], max_length, side, mode)
    front, between, behind = consts
    cb, ce, cd, ci = O.combine_segments([const_segment(front), (ab, ae, ids), const_segment(between), (bb, be, ids), const_segment(behind)], TYPE_IDS)
    longest = int((ce - cb).max()) if n else 0
    width = longest if target is None else target(longest)
    cd, ci = np.concatenate([cd, np.zeros(1, np.int32)]), np.concatenate([ci, np.zeros(1, np.int32)])
    want_ids, want_mask = O.ragged_to_dense(cb, ce, cd, width, PAD, pad_right)
    want_types, _ = O.ragged_to_dense(cb, ce, ci, width, TYPE_PAD, pad_right)
    return [want_ids, np.asarray(want_mask).astype(bool), want_types], width


TARGETS = [None, lambda longest: longest + 3, lambda longest: max(longest - 2, 0)]   # the longest row, above it, below it


def cases():
    """3 modes x 2 sides x 4 max_lengths; the other settings go round inside so that every padding side meets every target_dim and every
    set of constants meets every mode and every max_length."""
    out = []
    k = 0
    for mi, mode in enumerate(MODES):
        for side in SIDES:
            for li, max_length in enumerate(MAX_LENGTHS):
                out.append(dict(mode=mode, side=side, max_length=max_length, pad_right=k % 2 == 0, target=TARGETS[(k // 2) % 3],
                                consts=CONSTANTS[(mi + li + k // 4) % 3]))
                k += 1
    return out


def front_ops(kind, lib):
    """The handles in front of the tail: built once per test (their tables are not what these tests are about), shared by its cases."""
    if kind == "wordpiece":
        tok = bert_tok()
        return (K.RegexSplit("remove", lib=lib), K.RegexSplit("isolate", lib=lib),
                K.WordpieceTokenizer(tok["suffix_indicator"], tok["max_bytes_per_word"], lib=lib))
    return (K.RegexSplit("isolate", lib=lib), K.BPETokenizer(**bpe_tok().attrs, lib=lib), K.SpecialTokensSplit(lib=lib) if kind == "bpe-special" else None)


def make_op(kind, lib, handles, **tail):
    return (K.FusedPairWordpieceDense if kind == "wordpiece" else K.FusedPairEncodeDense)(*handles, **tail)


def call(op, kind, data, n, **kw):
    if kind == "wordpiece":
        from tests.test_ops_parity import BERT_PUNCT, BERT_WS
        tok = bert_tok()
        return op.evaluate(data, n, u8(BERT_WS), u8(BERT_PUNCT), list(pack_strings(tok["vocab"])) + [np.asarray(tok["unk_id"], np.int32)], **kw)
    if kind == "bpe-special":
        kw["special_pattern"] = u8(special_pattern())
    return op.evaluate(data, n, bpe_tok().pattern_u8(), bpe_tok().consts, **kw)


def tail_of(c):
    return dict(max_length=c["max_length"], trunc_side=c["side"], trunc_mode=c["mode"], pad_right=c["pad_right"], pad_value=PAD,
                type_pad_value=TYPE_PAD, front=c["consts"][0], between=c["consts"][1], behind=c["consts"][2], type_ids=TYPE_IDS)


def same(what, got, want, host):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g = host(g)
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}, output {i}: {g.dtype}{g.shape}, expected {w.dtype}{w.shape}"
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            raise AssertionError(f"{what}, output {i}: first difference at {tuple(bad)}: got {g[bad[0]]}, expected {w[bad[0]]}")


def branches_seen(ragged, n, max_length):
    """Which branches of longest_first (truncate.cpp:103-115) the batch takes at max_length, and its ties over an odd budget."""
    rb, re_, _ = ragged
    fl, sl = (re_ - rb)[:n].astype(np.int64), (re_ - rb)[n:].astype(np.int64)
    over = fl + sl > max_length
    half, half_up = max_length // 2, max_length // 2 + max_length % 2
    first_only = over & (fl >= half_up) & (sl <= half)
    second_only = over & (fl < half_up) & (sl > half)
    both = over & ~first_only & ~second_only
    ties = over & (fl == sl) & (fl > max_length / 2) & (max_length % 2 == 1)
    return int(first_only.sum()), int(second_only.sum()), int(both.sum()), int(ties.sum())


@pytest.mark.parametrize("kind", ["bpe", "wordpiece"])
def test_pair_dense_equals_the_chain(backend, kind):
    if backend.name == "hip-host":
        pytest.skip("device tensors only")
    gpu = backend.name != "emu"
    for k in (["bpe", "bpe-special"] if kind == "bpe" else ["wordpiece"]):
        front = front_ops(k, backend.lib)
        for n in ROW_COUNTS:
            todo = [batch(k, n)] + ([batch(k, 1, ordinary=False)] if n == 1 else [])
            for strings, ragged in todo:
                lens = (ragged[1] - ragged[0])
                if n >= 3:   # an empty first row, an empty second row, a row where both are empty
                    assert lens[0] == 0 and lens[n] > 0 and lens[1] > 0 and lens[n + 1] == 0 and lens[2] == 0 and lens[n + 2] == 0
                if n >= 65:   # every branch of truncate.cpp:103-115 occurs, and a tie with first == second > max_length / 2 at an odd max_length
                    for m in (9, 16):
                        assert all(x > 0 for x in branches_seen(ragged, n, m)[:3]), (k, n, m, branches_seen(ragged, n, m))
                if n >= 5:
                    assert branches_seen(ragged, n, 9)[3] > 0 and lens[3] == lens[n + 3] and lens[3] > 4
                data = backend.data(one_string_per_row(strings))
                for ci, c in enumerate(cases()):
                    # (the emulator runs every lane on one CPU thread: every case up to 65 pairs, every fourth at 300 -- each mode, side and
                    # max_length still occurs there --; the GPU runs them all)
                    if not gpu and n == 300 and ci % 4 != ci // 4 % 4:
                        continue
                    want, width = expected(ragged, n, c["max_length"], c["side"], c["mode"], c["consts"], c["pad_right"], c["target"])
                    op = make_op(k, backend.lib, front, **tail_of(c))
                    # (on the GPU every case runs twice: the second call runs on what the memo learned; on the emulator two of the cases do)
                    for again in range(2 if gpu or n == 65 else 1):
                        got = call(op, k, data, n, target_dim=None if c["target"] is None else width, row_capacity=max(width, 1))
                        assert op.n_ids == int(lens.sum()), "n_ids: the ids of all 2n rows before truncation"
                        same(f"{k}, {n} pairs, case {ci} {c['mode']} {c['side']} max_length {c['max_length']} pad_right {c['pad_right']} "
                             f"width {width} constants {c['consts']}, call {again}", got, want, backend.host)


def test_pair_dense_arguments(backend):
    if backend.name == "hip-host":
        pytest.skip("device tensors only")
    n = 5
    for kind in ("bpe", "wordpiece"):
        strings, ragged = batch(kind, n)
        data = backend.data(one_string_per_row(strings))
        front = front_ops(kind, backend.lib)
        c = dict(mode="longest_first", side="right", max_length=9, pad_right=True, consts=CONSTANTS[1])
        want, width = expected(ragged, n, 9, "right", "longest_first", CONSTANTS[1], True, None)
        # as many second rows as first ones, or the two-call form
        for n_first in (n - 1, n + 1, 2 * n, -1):
            with pytest.raises(L.OvtkError, match="two-call form") as ei:
                call(make_op(kind, backend.lib, front, **tail_of(c)), kind, data, n_first)
            assert ei.value.code == L.E_ARG
        # five constants in a slot
        for slot in range(3):
            consts = [(1,), (2,), (3,)]
            consts[slot] = (1, 2, 3, 4, 5)
            with pytest.raises(L.OvtkError) as ei:
                call(make_op(kind, backend.lib, front, **tail_of(dict(c, consts=consts))), kind, data, n)
            assert ei.value.code == L.E_UNSUPPORTED
        # an unknown mode
        for mode in (3, -1):
            with pytest.raises(L.OvtkError, match="Unknown truncation mode") as ei:
                call(make_op(kind, backend.lib, front, **tail_of(dict(c, mode=mode))), kind, data, n)
            assert ei.value.code == L.E_ARG
        # too little room: the width it needs
        with pytest.raises(L.OvtkError) as ei:
            call(make_op(kind, backend.lib, front, **tail_of(c)), kind, data, n, row_capacity=width - 1)
        assert ei.value.code == L.E_CAPACITY and ei.value.width == width
        # ... also for a batch without text (the width comes from finish, as ever)
        blank = backend.data(one_string_per_row([b""] * (2 * n)))
        with pytest.raises(L.OvtkError) as ei:
            call(make_op(kind, backend.lib, front, **tail_of(c)), kind, blank, n, row_capacity=2)
        assert ei.value.code == L.E_CAPACITY and ei.value.width == 3
        got = call(make_op(kind, backend.lib, front, **tail_of(c)), kind, blank, n)
        assert np.array_equal(backend.host(got[0]), np.tile(np.asarray([101, 102, 103], np.int32), (n, 1))) and backend.host(got[1]).all()
        assert np.array_equal(backend.host(got[2]), np.tile(np.asarray([5, 6, 7], np.int32), (n, 1)))
        # no mask, no type ids
        got = call(make_op(kind, backend.lib, front, **tail_of(c)), kind, data, n, mask=False, type_ids=False)
        assert got[1] is None and got[2] is None
        same("ids alone", got[:1], want[:1], backend.host)
        got = call(make_op(kind, backend.lib, front, **tail_of(c)), kind, data, n, row_capacity=width)
        same("all three", got, want, backend.host)
        # no rows
        empty = [np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8)]
        got = call(make_op(kind, backend.lib, front, **tail_of(c)), kind, backend.data(empty) if backend.name == "emu" else _empty_device(), 0)
        assert [tuple(backend.host(g).shape) for g in got] == [(0, 0)] * 3


def _empty_device():
    import torch
    return [torch.zeros(0, dtype=torch.int32, device="cuda") for _ in range(4)] + [torch.zeros(0, dtype=torch.uint8, device="cuda")]


@pytest.mark.parametrize("shift,fill", [(3, 0x20), (15, 0xE2), pytest.param(1, 0x00, marks=pytest.mark.gpu), pytest.param(7, 0xFF, marks=pytest.mark.gpu)])
@pytest.mark.parametrize("kind", ["bpe-special", "wordpiece"])
def test_pair_dense_between_guard_bands(backend, kind, shift, fill, monkeypatch):
    """The call with its inputs and its three outputs at the odd offsets their element types allow, exactly as large as they must be,
    between guard bands: the same result, and no byte outside them changed."""
    if backend.name == "hip-host":
        pytest.skip("device tensors only")
    n = 65
    strings, ragged = batch(kind, n)
    c = dict(mode="longest_first", side="left", max_length=9, pad_right=False, consts=CONSTANTS[2])
    want, width = expected(ragged, n, 9, "left", "longest_first", CONSTANTS[2], False, None)
    arena = Arena(backend, fill, 2 << 20)
    data = [arena.place(a, shift) for a in one_string_per_row(strings)]
    with arena.outputs(monkeypatch, shift):
        got = call(make_op(kind, backend.lib, front_ops(kind, backend.lib), **tail_of(c)), kind, data, n, row_capacity=width)
    same(f"{kind} at {shift}", got, want, backend.host)
    arena.check()
