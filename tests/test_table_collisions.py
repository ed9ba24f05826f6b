"""The device hash tables (csrc/tables.hpp) on inputs that COLLIDE: the second cuckoo candidate, probe chains, wraps at a table's end, full
buckets, refused memo slots, keys that share all 32 hash bits -- the paths a natural vocabulary reaches only by chance, and the ones where
the device code repeats the host's by hand.

tests/emu/table_collisions.cpp (host code, the project's own hash functions and builders) searches the inputs and records what makes each
of them a case; tests/golden/table_collisions.json is its output (tests/gen_golden_table_collisions.py).  Here:
  * `test_cases_still_collide` builds and runs the program again: every recorded fact must come out as committed, no family may be empty;
  * the parity tests feed each case to the op that owns the table -- emulator, HIP with host and with device buffers -- against the oracle
    (UnigramTokenizer: against tests/unigram_ref.py, the oracle directory has no Unigram op), twice per handle;
  * `test_three_merges_with_one_mix_are_refused` (case c) creates the handle in a child process with a time limit: before build_bpe
    counted the keys per mix its cuckoo loop never ended on this input.
The cases' letters are those of the helper's JSON: merge a-c, memo d-e, string_map f-h, bucket_trie i-k, edge_trie l-m.
"""
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from openvino_tokenizers_amd import _lib as L
from openvino_tokenizers_amd.ops import (BPETokenizer, FusedSplitBPE, RegexSplit, TrieTokenizer, UnigramTokenizer, VocabEncoder,
                                         WordpieceTokenizer)
from oracle import oracle as O
from tests.unigram_ref import UnigramRef
from tests.util import BpeTok, assert_same
from tools.make_tokenizers import GPT2_PATTERN
from tools.workloads import ragged_rows

ROOT = Path(__file__).resolve().parent.parent
CASES = json.loads((ROOT / "tests" / "golden" / "table_collisions.json").read_text())


def unhex(xs):
    return [bytes.fromhex(x) for x in xs]


def base_tok(i):
    """Base token i of the helper's synthetic BPE vocabularies: four lower-case letters, i in base 26."""
    return bytes(97 + (i // 26 ** k) % 26 for k in (3, 2, 1, 0))


def synthetic_bpe(n_base, merges, **attrs):
    """n_base base tokens, then the merged token of every (left id, right id) at the next spare id."""
    vocab = [base_tok(i) for i in range(n_base)] + [base_tok(l) + base_tok(r) for l, r in merges]
    return BpeTok(vocab, [(base_tok(l), base_tok(r)) for l, r in merges], pattern=GPT2_PATTERN, **attrs)


# ------------------------------------------------------------------------------------------------ the guard
def test_cases_still_collide():
    subprocess.run(["make", "-C", str(ROOT / "openvino_tokenizers_amd" / "csrc"), "-s", "collisions"], check=True)
    r = subprocess.run([str(ROOT / "tests" / "emu" / "build" / "table_collisions")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    now = json.loads(r.stdout)
    assert now == CASES, "the helper's facts differ from tests/golden/table_collisions.json: a hash function or a builder changed"
    m, memo, sm, bt, et = (CASES[k] for k in ("merge", "memo", "string_map", "bucket_trie", "edge_trie"))
    # merge table: (a) one mix, one in each of the two candidate slots; (b) at least one eviction; (c) three with one mix, refused
    assert len(m["a"]["merges"]) == 2 and sorted(m["a"]["slots"]) == sorted(m["a"]["candidate_slots"]) and len(set(m["a"]["slots"])) == 2
    assert m["b"]["kicks"] >= 1 and len(m["b"]["merges"]) >= 3
    assert len(m["c"]["triple"]) == 3 and len(set(m["c"]["left_high_words"])) == 3 and m["c"]["unsupported"] is True
    # piece memo: one slot; (d) different mixes, (e) the same 32 bits (and so the same tag); the later token refused
    for k in ("d", "e"):
        c = memo[k]
        assert c["fixed"]["x_stored"] and c["fixed"]["y_refused"] and c["fixed"]["refused"] >= 1 and c["learned"]["slot_free"]
        assert (c["mix_x"] == c["mix_y"]) == (k == "e") and (c["tag_x"] == c["tag_y"]) == (k == "e") and c["x_hex"] != c["y_hex"]
    # string map: (f) a chain of four, (g) one that wraps, (h) one full hash for two keys and for a present and an absent one
    assert sm["f"]["chain_length"] >= 4 and not sm["f"]["wrap"] and sm["f"]["slots"] == sorted(sm["f"]["slots"]) and sm["f"]["absent"]
    assert sm["g"]["chain_length"] >= 2 and sm["g"]["wrap"] and sm["g"]["slots"][0] == sm["g"]["mask"] and 0 in sm["g"]["slots"] and sm["g"]["absent"]
    assert sm["h"]["hashes"][0] == sm["h"]["hashes"][1] and sm["h"]["absent_hash"] == sm["h"]["hashes"][2] and len(set(sm["h"]["keys"])) == 4
    # bucket trie: (i) a walk into the next bucket, (j) from the last bucket to bucket 0, (k) a miss behind a full bucket
    assert bt["i"]["crossing"] and bt["i"]["overflowing_buckets"]
    assert bt["j"]["wrapping"] and bt["j"]["n_buckets"] - 1 in bt["j"]["overflowing_buckets"]
    assert bt["k"]["absent_past_full_bucket"] and bt["k"]["full_buckets"] >= 1
    # TrieEdge table: (l) a probe of three slots or more, (m) one that wraps -- in a WordPiece trie and in the BPE trie
    assert max(et["wordpiece_l"][t]["longest_chain"] for t in ("root", "sub")) >= 3 and (et["wordpiece_l"]["root"]["chained"] or et["wordpiece_l"]["sub"]["chained"])
    assert et["wordpiece_m"]["root"]["wrapping"] or et["wordpiece_m"]["sub"]["wrapping"]
    assert et["bpe"]["trie"]["longest_chain"] >= 3 and et["bpe"]["trie"]["chained"] and et["bpe"]["trie"]["wrapping"]


# ------------------------------------------------------------------------------------------------ BPE: merge table, memo, trie
def _bpe_rows(pieces, n_rows, rng):
    """Rows of one to four pieces each: every piece in a row of its own first, then random ones."""
    rows = [[p] for p in pieces]
    while len(rows) < n_rows:
        rows.append([pieces[int(k)] for k in rng.integers(0, len(pieces), int(rng.integers(1, 5)))])
    strings = [p for r in rows for p in r]
    ends = np.cumsum([len(r) for r in rows]).astype(np.int32)
    return (ends - np.asarray([len(r) for r in rows], np.int32)).astype(np.int32), ends, strings


def check_bpe(backend, tok, pieces, what, bpe=None, calls=2, n_rows=40):
    """The pieces through BPETokenizer (rows of several pieces) and through the fused encode (a piece per row: letters only, so the GPT-2
    pattern leaves each whole; a call of a few rows and one of more than 256, which takes the span kernel), `calls` times each on ONE
    handle, against the oracle.  Returns the handle."""
    rng = np.random.default_rng(7)
    orc = tok.oracle()
    bpe = bpe or BPETokenizer(**tok.attrs, lib=backend.lib)
    rb, re_, strings = _bpe_rows(pieces, n_rows, rng)
    b, e, c = O.pack_strings(strings)
    ref = orc(rb, re_, b, e, c)
    for call in range(calls):
        assert_same(ref, bpe.evaluate(backend.data([rb, re_, b, e, c]) + tok.consts), backend.host, f"{what}: BPETokenizer, call {call}")
    fused = FusedSplitBPE(RegexSplit("isolate", lib=backend.lib), bpe)
    for n in (len(pieces), 300):
        rows = [pieces[k % len(pieces)] for k in range(n)]
        b, e, c = O.pack_strings(rows)
        rb, re_ = ragged_rows(n)
        ref = orc(*O.RegexSplit(tok.pattern, "isolate")(rb, re_, b, e, c)[:5])
        assert len(ref[2]) >= n
        for call in range(calls):
            assert_same(ref, fused.evaluate(backend.data([rb, re_, b, e, c]) + [tok.pattern_u8()], tok.consts), backend.host, f"{what}: fused, {n} rows, call {call}")
    return bpe


def _pair_pieces(merges, absent):
    cat = lambda l, r: base_tok(l) + base_tok(r)   # noqa: E731
    pieces = [cat(l, r) for l, r in merges] + [cat(l, r) for l, r in absent]
    pieces += [cat(l, r) + base_tok(l) for l, r in merges] + [base_tok(r) + cat(l, r) for l, r in merges]   # a merge inside a longer piece
    pieces += [base_tok(l) for l, _ in merges]
    return list(dict.fromkeys(pieces))


@pytest.mark.parametrize("case", ["a", "b"])
def test_merge_table(backend, case):
    """(a) two merges with one merge_mix, one in each candidate slot: the lookup must take the second candidate for one of them, and compare
    the whole key (the absent pairs land on the same slots).  (b) a table whose build evicted.  cache_capacity = 0: no memo, every piece of
    every call goes through the merge table (and a vocabulary of 47 817 tokens is not encoded at create)."""
    c = CASES["merge"][case]
    tok = synthetic_bpe(c["n_base"], c["merges"], cache_capacity=0)
    pieces = _pair_pieces(c["merges"], c["absent"])
    orc = tok.oracle()
    b, e, s = O.pack_strings(pieces)
    rb, re_ = ragged_rows(len(pieces))
    ids = orc(rb, re_, b, e, s)
    for k in range(len(c["merges"])):   # the case is what it says: every merge applies, the absent pairs stay two ids
        assert ids[2][ids[0][k]:ids[1][k]].tolist() == [c["n_base"] + k]
    for k in range(len(c["merges"]), len(c["merges"]) + len(c["absent"])):
        assert ids[1][k] - ids[0][k] == 2
    check_bpe(backend, tok, pieces, f"merge table ({case})")


@pytest.mark.parametrize("case", ["d", "e"])
def test_piece_memo_refuses_at_create(backend, case):
    """X and Y are vocabulary tokens of one memo slot ((e): of one 32-bit piece_mix, so of one tag too).  build_piece_table keeps X and
    refuses Y: Y must come out of the merge path, and a lookup of Y must not take X's entry."""
    c = CASES["memo"][case]
    f = c["fixed"]
    vocab = unhex(f["vocab"])
    tok = BpeTok(vocab, [tuple(unhex(m)) for m in f["merges"]], pattern=GPT2_PATTERN, cache_capacity=c["cache_capacity"])
    x, y = bytes.fromhex(c["x_hex"]), bytes.fromhex(c["y_hex"])
    pieces = [y, x] + unhex(c["near"]) + vocab[:8] + [x + y[:4], y + x[4:]]
    bpe = BPETokenizer(**tok.attrs, lib=backend.lib)
    bpe._ensure([None] * 5 + tok.consts)
    fixed, learned = C.c_int64(), C.c_int64()
    L.check(backend.lib, backend.lib.ovtk_bpe_memo_entries(bpe._h, C.byref(fixed), C.byref(learned)))
    assert fixed.value == f["stored"] == len(vocab) - 1 and f["refused"] == 1   # the handle's table is the helper's
    check_bpe(backend, tok, pieces, f"memo ({case}), fixed", bpe=bpe)


@pytest.mark.parametrize("case", ["d", "e"])
def test_piece_memo_refuses_when_learning(backend, case):
    """The same X and Y where neither is a token: pieces of two ids each, their slot free at create.  A handle that learns (memo_learn = -1)
    sees Y first: Y takes the slot.  X is then refused by memo_insert -- the count of learned entries stays -- and must still encode
    correctly, as must Y from the entry and the look-alikes."""
    c = CASES["memo"][case]
    f = c["learned"]
    vocab = unhex(f["vocab"])
    tok = BpeTok(vocab, [tuple(unhex(m)) for m in f["merges"]], pattern=GPT2_PATTERN, cache_capacity=c["cache_capacity"])
    x, y = bytes.fromhex(c["x_hex"]), bytes.fromhex(c["y_hex"])
    bpe = BPETokenizer(**tok.attrs, lib=backend.lib, memo_learn=-1)
    orc = tok.oracle()

    def run(pieces, what):
        b, e, s = O.pack_strings(pieces)
        rb, re_ = ragged_rows(len(pieces))
        assert_same(orc(rb, re_, b, e, s), bpe.evaluate(backend.data([rb, re_, b, e, s]) + tok.consts), backend.host, what)
        fixed, learned = C.c_int64(), C.c_int64()
        L.check(backend.lib, backend.lib.ovtk_bpe_memo_entries(bpe._h, C.byref(fixed), C.byref(learned)))
        assert fixed.value == f["stored"]
        return learned.value

    assert run([y, vocab[0], y], "Y first") == 1
    assert run([x, y, x, vocab[1]], "X behind Y") == 1          # X found its slot taken
    assert run([y, x], "both again") == 1
    check_bpe(backend, tok, [x, y] + unhex(c["near"]) + vocab[:8] + [x + y[:4]], f"memo ({case}), learned", bpe=bpe)


def test_bpe_trie_probe_chains(backend):
    """(l, m) the open-addressed TrieEdge table of a BPE handle: tokens whose walk probes three slots, one whose probe wraps to slot 0."""
    c = CASES["edge_trie"]["bpe"]
    tok = synthetic_bpe(c["n_base"], c["merges"], cache_capacity=0)
    t = c["trie"]
    words = unhex(t["chained"]) + unhex(t["wrapping"])
    pieces = words + [w + v for w in words for v in words[:2]] + [base_tok(0) + base_tok(1), base_tok(1) + base_tok(0)] + [base_tok(i) for i in range(0, c["n_base"], 9)]
    check_bpe(backend, tok, list(dict.fromkeys(pieces)), "BPE trie")


# ------------------------------------------------------------------------------------------------ case (c): build_bpe ends
CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from openvino_tokenizers_amd import _lib as L
from openvino_tokenizers_amd.ops import BPETokenizer
from tests.test_table_collisions import CASES, synthetic_bpe
c = CASES["merge"]["c"]
tok = synthetic_bpe(c["n_base"], c["merges"], cache_capacity=0)
bpe = BPETokenizer(**tok.attrs, lib=L.load(sys.argv[2]))
try:
    bpe._ensure([None] * 5 + tok.consts)
    print(json.dumps({"code": 0, "message": ""}))
except L.OvtkError as err:
    print(json.dumps({"code": err.code, "message": str(err)}))
"""


def test_three_merges_with_one_mix_are_refused(emu_lib):
    """(c) merge_h1 and merge_h2 are functions of merge_mix alone: three merges with one mix have two slots between them at every table
    size.  ovtk_bpe_create must say so -- OVTK_E_UNSUPPORTED, the three merges by index -- and must return at all: the handle is created
    in a child process under a time limit (host code, the same in both builds: the emulator library only)."""
    c = CASES["merge"]["c"]
    try:
        r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), str(ROOT / "tests" / "emu" / "build" / "libovtk_emu.so")],
                           capture_output=True, text=True, timeout=60)
    except subprocess.TimeoutExpired:
        pytest.fail("ovtk_bpe_create did not return within 60 s on three merges with one merge_mix")
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.splitlines()[-1])
    assert got["code"] == L.E_UNSUPPORTED, got
    assert "merges " + ", ".join(map(str, c["triple"])) + " " in got["message"], got["message"]


# ------------------------------------------------------------------------------------------------ VocabEncoder
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("case", ["f", "g", "h"])
def test_string_map(backend, case, dtype):
    """(f) four keys of one home slot, (g) a chain from the last slot round to slot 0, (h) two keys with one 32-bit hash_bytes and an absent
    key that shares all 32 bits with a present one.  Queries: every key, the absent keys that land on the chains, keys cut short and
    lengthened, the empty string."""
    c = CASES["string_map"][case]
    keys, absent = unhex(c["keys"]), unhex(c["absent"])
    values = (np.arange(len(keys)) * 1000003 + (2 ** 40 if dtype == np.int64 else 7)).astype(dtype)
    queries = keys + absent + [k[:-1] for k in keys] + [k + b"\0" for k in keys] + [b""] + keys[::-1] + absent
    b, e, s = O.pack_strings(queries)
    ref = O.VocabEncoder(keys, values)(b, e, s, -5)
    assert ref[:len(keys)].tolist() == values.tolist() and set(ref[len(keys):len(keys) + len(absent)].tolist()) == {-5}
    op = VocabEncoder(lib=backend.lib)
    kb, ke, kc = O.pack_strings(keys)
    for call in range(2):
        got = op.evaluate(backend.data([b, e, s]) + [kb, ke, kc, values, np.asarray(-5, dtype)])
        assert_same([ref], got, backend.host, f"VocabEncoder ({case}), call {call}")


# ------------------------------------------------------------------------------------------------ the bucket trie
def _trie_strings(c):
    rng = np.random.default_rng(3)
    vocab = unhex(c["vocab"])
    special = unhex(c["crossing"]) + unhex(c["wrapping"]) + unhex(c["absent_past_full_bucket"])
    strings = special + [s + t for s in special for t in special] + vocab
    strings += [b"".join(vocab[int(k)] for k in rng.integers(0, len(vocab), int(rng.integers(1, 12)))) for _ in range(30)]
    strings += [bytes(rng.choice(list(b"abcd"), size=int(rng.integers(1, 80))).tolist()) for _ in range(20)] + [b""]
    return vocab, strings


@pytest.mark.parametrize("case", ["i", "j", "k"])
def test_bucket_trie_trie_tokenizer(backend, case):
    """(i) a bucket that received more than four edges: a token's walk crosses into the next bucket; (j) the last bucket overflows into
    bucket 0; (k) an edge that is not there, looked for behind a full bucket.  TrieWalk::chain reads buckets by halves and spells the
    bucket hash out once more."""
    vocab, strings = _trie_strings(CASES["bucket_trie"][case])
    indices = np.arange(1, len(vocab) + 1, dtype=np.int32)
    b, e, s = O.pack_strings(strings)
    n = len(strings)
    rb = np.concatenate([np.arange(n), [0]]).astype(np.int32)    # every string a row, and one row of the first nine
    re_ = np.concatenate([np.arange(n) + 1, [9]]).astype(np.int32)
    ref = O.TrieTokenizer(vocab, indices)(rb, re_, b, e, s)
    vb, ve, vc = O.pack_strings(vocab)
    op = TrieTokenizer(lib=backend.lib)
    for call in range(2):
        got = op.evaluate(backend.data([rb, re_, b, e, s]) + [vb, ve, vc, indices])
        assert_same(list(ref), got, backend.host, f"TrieTokenizer ({case}), call {call}")


@pytest.mark.parametrize("case", ["i", "j", "k"])
def test_bucket_trie_unigram(backend, case):
    """The same vocabularies under UnigramTokenizer, whose walk (uni_trie_step) is a second copy of the bucket walk.  Scores are multiples
    of 1/8: every sum is exact.  `z` is in no token: unknown edges between the colliding ones."""
    vocab, strings = _trie_strings(CASES["bucket_trie"][case])
    strings += [s + b"z" + s for s in strings[:6]]
    scores = (-((np.arange(len(vocab)) * 5) % 11 + 1) / 8.0).astype(np.float32)
    b, e, s = O.pack_strings(strings)
    rb = np.arange(len(strings), dtype=np.int32)
    ref = UnigramRef(vocab, scores, unk_token_id=2)(rb, rb + 1, b, e, s)
    vb, ve, vc = O.pack_strings(vocab)
    op = UnigramTokenizer(unk_token_id=2, lib=backend.lib)
    for call in range(2):
        got = op.evaluate(backend.data([rb, rb + 1, b, e, s]) + [vb, ve, vc, scores])
        assert_same(list(ref), got, backend.host, f"UnigramTokenizer ({case}), call {call}")


# ------------------------------------------------------------------------------------------------ WordPiece's two TrieEdge tables
@pytest.mark.parametrize("case", ["wordpiece_l", "wordpiece_m"])
def test_wordpiece_trie_probe_chains(backend, case):
    """(l) a probe chain of three slots, (m) one that wraps, in the root trie or the `##` trie; edges that are not there whose probe passes
    taken slots.  Words: the strings themselves, and each behind a first piece so that the `##` trie is walked with it."""
    c = CASES["edge_trie"][case]
    vocab = unhex(c["vocab"])
    special = [w for t in ("root", "sub") for k in ("chained", "wrapping", "absent") for w in unhex(c[t][k])]
    words = special + [h + w for w in special for h in (b"a", b"b", b"dc")] + [w + t for w in special for t in (b"a", b"cd")]
    words += [v[2:] if v.startswith(b"##") else v for v in vocab] + [b"abcdabcdabcd", b"z", b"az"]
    words = list(dict.fromkeys(words))
    b, e, s = O.pack_strings(words)
    rb, re_ = ragged_rows(len(words))
    ref = O.WordpieceTokenizer(vocab)(rb, re_, b, e, s, 99)
    vb, ve, vc = O.pack_strings(vocab)
    op = WordpieceTokenizer(lib=backend.lib)
    for call in range(2):
        got = op.evaluate(backend.data([rb, re_, b, e, s]) + [vb, ve, vc, np.asarray(99, np.int32)])
        assert_same(list(ref), got, backend.host, f"WordpieceTokenizer ({case}), call {call}")
