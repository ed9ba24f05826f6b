"""pipeline.add_second_input / Pipeline.run_pair: the mirror of the reference's add_second_input
(python/openvino_tokenizers/tokenizer_transformations.py:22-304) over the step lists of pipeline.py, op by op and fused, and the
result against HF `tokenizers` (tests/gen_golden_pair.py).  Whole arrays, no tolerance."""
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from openvino_tokenizers_amd import pipeline as P
from oracle import oracle as O
from tests.util import BpeTok, pack_strings
from tools.make_tokenizers import load_tokenizer
from tools.workloads import TextModel

G = Path(__file__).parent / "golden"
SPECIAL = "<|endoftext|>"


def _kinds(steps):
    return [type(s).__name__ for s in steps]


@lru_cache(maxsize=None)
def _stream():
    _, _, c = TextModel(99, "zipf").batch(1, 40000)
    return c.tobytes().lower()


def texts(n, seed, special=False):
    rng = np.random.default_rng(seed)
    t = _stream()
    out = []
    for i in range(n):
        k = int(rng.integers(0, 100)) if rng.integers(3) else int(rng.integers(0, 10))
        at = int(rng.integers(0, len(t) - k))
        s = t[at:at + k].strip()
        if special and i % 5 == 1:
            s = s[:len(s) // 2] + SPECIAL.encode() + s[len(s) // 2:]
        out.append(s)
    if n > 2:
        out[2] = b""
    return out


def bert_steps(lib, max_length=14, side="right", target_dim=None):
    tok = load_tokenizer("bert_small")
    consts = list(pack_strings(tok["vocab"])) + [np.asarray(tok["unk_id"], np.int32)]
    return [P.RegexSplitStep(P.BERT_WS, "remove", lib=lib), P.RegexSplitStep(P.BERT_PUNCT, "isolate", lib=lib),
            P.WordPieceTokenizationStep(consts, tok["suffix_indicator"], tok["max_bytes_per_word"], lib=lib),
            P.TruncationStep(max_length, side, lib=lib), P.CombineSegmentsStep(prefix=[2], suffix=[3], lib=lib),
            P.PaddingStep(pad_value=0, target_dim=target_dim, lib=lib)]


def bpe_steps(lib, with_special, max_length=15, side="left"):
    tok = BpeTok.load("gpt2_small")
    steps = [P.SpecialTokensSplitStep(O.special_tokens_pattern([(SPECIAL, False, False)]), lib=lib)] if with_special else []
    return steps + [P.RegexSplitStep(tok.pattern, "isolate", lib=lib), P.BPETokenizationStep(tok.consts, lib=lib, **tok.attrs),
                    P.TruncationStep(max_length, side, lib=lib), P.CombineSegmentsStep(prefix=[7], suffix=[9], lib=lib),
                    P.PaddingStep(pad_value=50256, pad_right=False, lib=lib)]


GRAPHS = {
    # name -> (steps, single signature, pair signature, pair type ids, the fused kinds)
    "bert": (lambda lib: bert_steps(lib), [2, -1, 3], [2, -1, 3, -2, 3], [0, 0, 0, 1, 1], ["FusedPairWordpieceDenseStep"]),
    "roberta": (lambda lib: bpe_steps(lib, False), [7, -1, 9], [7, -1, 9, 9, -2, 9], [0, 0, 0, 0, 0, 0], ["FusedPairEncodeDenseStep"]),
    "gpt2-special": (lambda lib: bpe_steps(lib, True), [7, -1, 9], [7, -1, 9, -2, 9], [0, 0, 0, 1, 1], ["FusedPairEncodeDenseStep"]),
}


def same(what, got, want, host):
    assert len(got) == len(want) == 3, what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = host(g), host(w)
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}, output {i}: {g.dtype}{g.shape}, expected {w.dtype}{w.shape}"
        assert np.array_equal(g, w), f"{what}, output {i}: first difference in row {int(np.argwhere(g != w)[0][0])}"


@pytest.mark.parametrize("graph", list(GRAPHS))
def test_add_second_input_fused_equals_op_by_op(backend, graph):
    """Pipeline(add_second_input(steps, ...)).run_pair op by op = .fused().run_pair: nA == nB (the one call on device tensors), 1 against 7
    in both directions and 7 against an empty second input (the two-call form)."""
    make, single, pair, types, kinds = GRAPHS[graph]
    pipe = P.Pipeline(P.add_second_input(make(backend.lib), single, pair, types, type_pad_value=4))
    fused = pipe.fused()
    assert _kinds(fused.steps) == kinds
    assert _kinds(pipe.steps)[-3:] == ["PairTruncationStep", "PairCombineSegmentsStep", "PairPaddingStep"]
    special = graph == "gpt2-special"
    for na, nb in ((5, 5), (300, 300), (1, 7), (7, 1), (7, 0)):
        first, second = backend.data(pack_strings(texts(na, 10 + na, special))), backend.data(pack_strings(texts(nb, 20 + nb, special)))
        want = pipe.run_pair(first, second)
        assert tuple(backend.host(want[0]).shape)[0] == max(na, nb)
        for call in range(2):
            same(f"{graph}, {na} against {nb}, call {call}", fused.run_pair(first, second), want, backend.host)
        if nb == 0:   # what the reference gives: [front] A [the single signature's end], max_length still reduced, no added constant
            solo = P.Pipeline(make(backend.lib))
            solo.steps[-3].max_length -= len(pair) - len(single) - 1
            ids, mask = solo.run("strings", [np.arange(na, dtype=np.int32), np.arange(1, na + 1, dtype=np.int32)] + list(first) + [None])[:2]
            assert np.array_equal(backend.host(want[0]), backend.host(ids)) and np.array_equal(backend.host(want[1]), backend.host(mask))
    with pytest.raises(ValueError, match="1 against n"):
        pipe.run_pair(backend.data(pack_strings(texts(3, 1))), backend.data(pack_strings(texts(2, 2))))
    with pytest.raises(ValueError, match="1 against n"):
        fused.run_pair(backend.data(pack_strings(texts(3, 1))), backend.data(pack_strings(texts(2, 2))))


def test_add_second_input_checks(emu_lib):
    lib = emu_lib
    steps = bert_steps(lib)
    before = list(steps)
    fused_before = _kinds(P.fuse(steps))
    ok = P.add_second_input(steps, [2, -1, 3], [2, -1, 3, -2, 3], [0, 0, 0, 1, 1])
    assert steps == before and all(a is b for a, b in zip(steps, before)) and ok is not steps
    assert ok[3].max_length == steps[3].max_length - 1 and steps[3].max_length == 14
    assert P.add_second_input(bpe_steps(lib, False), [7, -1, 9], [7, -1, 9, 9, -2, 9], [0] * 6)[2].max_length == 15 - 2
    with pytest.raises(ValueError, match="widen"):
        P.add_second_input(steps, [2, -1, 3], [2, -1, 4, -2, 3], [0, 0, 0, 1, 1])
    with pytest.raises(ValueError, match="exactly two sequence entries"):
        P.add_second_input(steps, [2, -1, 3], [2, -1, 3, -2, 3, -3, 3], [0, 0, 0, 1, 1, 2, 2])
    with pytest.raises(ValueError, match="exactly two sequence entries"):
        P.add_second_input(steps, [2, -1, 3], [2, -1, 3, 3], [0, 0, 0, 1])
    with pytest.raises(ValueError, match="exactly one sequence entry"):
        P.add_second_input(steps, [2, -1, -2], [2, -1, -2, 3], [0, 0, 1, 1])
    with pytest.raises(ValueError, match="TruncationStep in front of the CombineSegmentsStep"):
        P.add_second_input(steps[:3] + steps[4:], [2, -1, 3], [2, -1, 3, -2, 3], [0, 0, 0, 1, 1])
    with pytest.raises(ValueError, match="TruncationStep in front of the CombineSegmentsStep"):
        P.add_second_input(steps[:4] + steps[5:], [2, -1, 3], [2, -1, 3, -2, 3], [0, 0, 0, 1, 1])
    # a list without a pair tail fuses as before
    assert _kinds(P.fuse(steps)) == fused_before == ["FusedSplitWordpieceStep", "FusedEncodeTailStep"]
    assert _kinds(P.fuse(bpe_steps(lib, True))) == ["FusedEncodeDenseStep"]
    # more than four constants in a slot, or two type ids in one: the chain stays op by op behind the fused encode
    wide = P.add_second_input(bpe_steps(lib, False), [7, -1, 9], [7, -1, 9, 9, 9, 9, 9, -2, 9], [0] * 9)
    assert _kinds(P.fuse(wide)) == ["FusedSplitBPEStep", "PairTruncationStep", "PairCombineSegmentsStep", "PairPaddingStep"]
    mixed = P.add_second_input(bpe_steps(lib, False), [7, -1, 9], [7, -1, 9, 9, -2, 9], [0, 0, 0, 1, 1, 1])
    assert _kinds(P.fuse(mixed))[0] == "FusedSplitBPEStep"


def test_pair_matches_tokenizers(backend):
    """The BERT-small pair graph against HF tokenizers (tests/gen_golden_pair.py: `[CLS] A [SEP] B [SEP]`, longest_first to 20 ids, both
    directions, padding).  Rows that hit the one documented difference -- equal lengths over the odd budget of 17, tests/
    test_truncate_combine.py:30-45 -- are left out of that comparison and checked against the reference's rule: the odd id goes to the
    first sequence."""
    z = np.load(G / "golden_pair_bert_small.npz")
    first, second = [z[f"first_{k}"] for k in ("begins", "ends", "chars")], [z[f"second_{k}"] for k in ("begins", "ends", "chars")]
    n = len(first[0])
    # token counts, from the oracle
    from tests.test_ops_parity import bert_words
    tok = load_tokenizer("bert_small")
    wp = O.WordpieceTokenizer(tok["vocab"], tok["suffix_indicator"], tok["max_bytes_per_word"])

    def counts(b, e, c):
        rows = np.arange(len(b) + 1, dtype=np.int32)
        rb, re_, _ = wp(*bert_words([rows[:-1], rows[1:], b, e, c]), tok["unk_id"])
        return (re_ - rb).astype(np.int64)
    la, lb = counts(*first), counts(*second)
    budget = 20 - 3
    ties = (la == lb) & (la + lb > budget)
    assert 20 <= ties.sum() <= 0.05 * n
    for side in ("right", "left"):
        steps = P.add_second_input(bert_steps(backend.lib, max_length=18, side=side), [2, -1, 3], [2, -1, 3, -2, 3], [0, 0, 0, 1, 1])
        assert steps[3].max_length == budget
        ids, mask, types = (backend.host(x) for x in P.Pipeline(steps).fused().run_pair(backend.data(first), backend.data(second)))
        want_ids, want_types, want_mask = z[f"ids_{side}"], z[f"type_ids_{side}"], z[f"mask_{side}"].astype(bool)
        assert ids.shape == want_ids.shape
        keep = ~ties
        assert np.array_equal(ids[keep], want_ids[keep]) and np.array_equal(types[keep], want_types[keep]) and np.array_equal(mask[keep], want_mask[keep])
        # the tie rows: full rows, [CLS] + 9 of the first + [SEP] (type 0), 8 of the second + [SEP] (type 1) -- HF: 8 and 9
        assert mask[ties].all() and (types[ties].sum(1) == budget // 2 + 1).all() and (want_types[ties].sum(1) == budget // 2 + 2).all()
        assert (ids[ties][:, 1 + budget // 2 + 1] == 3).all()
