"""Generates tests/golden/launch_census.json: which kernels a fused encode launches, and how often.

The host side of the fused encodes (csrc/api_encode.cpp start_encode, csrc/api_ops.cpp start_wordpiece_encode) chooses a sequence of
kernel launches from the handles, the batch and two process-wide switches (ovtk_set_short_path, ovtk_set_row_tickets).  The library's
profiler counts launches per tag (ovtk_profile_enable / ovtk_profile_dump); on the emulator build the sequence is deterministic, so
tag -> launch count, per cell of the matrix below, characterises that choice.  tests/test_launch_plan.py replays the matrix and
compares exactly.  Emulator only: on a GPU what a handle's piece store has learned by call k depends on wave timing.

A cell: the two switches are set -> profile reset -> three calls on the same batch -> the profile, and what ovtk_short_path_stats()
counted during the calls.  Cells that share their handles run in a fixed order (groups(), below): what a handle has learned, and what
its predictors expect, carries over from cell to cell as it does in a process that keeps its handles.  A group's first cell creates
the handles (a BPE handle with a memo encodes its own vocabulary: `lookup_pieces`).

The fixture is generated from the build whose launch sequence is the one to keep -- for a change of the host code: the parent commit's
emulator library, loaded by path -- and committed as generated:
    python -m tests.gen_golden_launch_census [path/to/libovtk_emu.so]
"""
from __future__ import annotations

import ctypes as C
import json
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "launch_census.json"
CALLS = 3
DFA_PATTERN = r"[a-z]+|\p{N}+|\s+|[^\sa-z\p{N}]+"   # no hand-written scanner and no span family: the compiled DFA
WIDE_ID = 70000   # an added-token id above 65 535: the handle's ids fit neither merge_kernel's u16 nor the u16 staging entries

# front -> (tokenizer, pattern or None for the tokenizer's own, text model)
FRONTS = {
    "gpt2": ("gpt2_small", None, "zipf"),
    "gpt2-digits": ("gpt2_small", r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+|\p{N}| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+", "zipf"),
    "llama3": ("llama3_small", None, "mixed"),
    "qwen2": ("llama3_small", "qwen2", "mixed"),
    "o200k": ("llama3_small", "o200k", "mixed"),
    "deepseek-v3": ("llama3_small", "deepseek-v3", "mixed"),
    "dfa": ("gpt2_small", DFA_PATTERN, "zipf"),
    "max-splits-1": ("gpt2_small", None, "zipf"),
    "bpe-alone": ("gpt2_small", None, "zipf"),
    "wordpiece": ("bert_small", None, "zipf"),
}


STEPS = [(0, 0, 300), (1, 0, 300), (2, 0, 300), (1, 8, 300), (0, 8, 300), (1, 0, 40), (2, 0, 40), (1, 8, 40)]
FEW_STEPS = [(1, 0, 40), (1, 0, 300), (2, 0, 300), (1, 8, 300)]


def groups():
    """The matrix.  A group is one set of handles (creating a BPE handle is most of a cell's time on the emulator) taken through
    steps of (short-path mode, row tickets, rows), three calls each, in this order: every front x memo / no memo through STEPS
    with ragged outputs -- 40 rows: the one-launch form, 300: the large one --, and on GPT-2 / Llama-3 the other things a plan depends
    on through FEW_STEPS: ids wider than 16 bits, SpecialTokensSplit in front, dense and wire outputs."""
    out = []
    for front in FRONTS:
        for memo in (True, False):
            if front == "wordpiece" and not memo:
                continue   # (a WordPiece handle has its word memo whatever its parameters say)
            # (the count and write passes of a split with max_splits walk a row per lane: slow on the emulator)
            steps = [s for s in STEPS if s[2] == 40] if front == "max-splits-1" else FEW_STEPS if front == "qwen2" else STEPS
            out.append(dict(front=front, memo=memo, variant="ragged", steps=steps))
    for front, variants in (("gpt2", ("wide-ids", "special", "dense", "wire", "special-dense")), ("llama3", ("wide-ids", "special"))):
        for variant in variants:
            for memo in ((True, False) if variant == "wide-ids" else (True,)):
                out.append(dict(front=front, memo=memo, variant=variant, steps=FEW_STEPS))
    return out


def group_id(g):
    return f"{g['front']}/{g['variant']}/{'memo' if g['memo'] else 'no-memo'}"


def step_id(step):
    return "mode%d/tickets%d/rows%d" % step


@lru_cache(maxsize=None)
def _batch(model, rows, special):
    from tools.workloads import TextModel, ragged_rows
    b, e, c = TextModel(97, model).batch(rows, 32)
    if model == "zipf":
        c = np.frombuffer(c.tobytes().lower(), np.uint8).copy()
    if special:   # one row in seven holds the special token
        from tools.harness import pack_strings
        texts = [bytes(c[b[i]:e[i]]) for i in range(rows)]
        for i in range(0, rows, 7):
            texts[i] = texts[i][:len(texts[i]) // 2] + b"<|endoftext|>" + texts[i][len(texts[i]) // 2:]
        b, e, c = pack_strings(texts)
    rb, re_ = ragged_rows(rows)
    return [rb, re_, b, e, c]


class _Buf:
    """A host buffer with the one method FusedSplitBPE.enqueue_wire asks of its wire (the emulator's device memory is host memory)."""

    def __init__(self, nbytes):
        self.a = np.zeros(nbytes, np.uint8)

    def data_ptr(self):
        return self.a.ctypes.data


def _profile(lib):
    n = int(lib.ovtk_profile_dump(None, C.c_int64(0)))
    buf = C.create_string_buffer(n + 1)
    lib.ovtk_profile_dump(buf, C.c_int64(n + 1))
    out = {}
    for line in buf.value.decode().splitlines():
        tag, _, launches = line.split()
        out[tag] = int(launches)
    return out


def _stats(lib):
    t, x = C.c_int64(), C.c_int64()
    lib.ovtk_short_path_stats(C.byref(t), C.byref(x))
    return int(t.value), int(x.value)


def _runner(lib, g):
    """Creates the group's handles lazily (at the first call, as the ops do) -> run(rows)."""
    from openvino_tokenizers_amd import ops
    from oracle import oracle as O
    from tools.harness import BERT_PUNCT, BERT_WS, BpeTok, pack_strings
    from tools.make_tokenizers import load_tokenizer
    from tools.workloads import MODEL_PATTERNS
    tok_name, pattern, model = FRONTS[g["front"]]
    front, variant = g["front"], g["variant"]
    u8 = lambda s: np.frombuffer(s.encode(), np.uint8)   # noqa: E731
    data = lambda rows: _batch(model, rows, variant.startswith("special"))   # noqa: E731
    if front == "wordpiece":
        tok = load_tokenizer(tok_name)
        fused = ops.FusedSplitWordpiece(ops.RegexSplit("remove", lib=lib), ops.RegexSplit("isolate", lib=lib),
                                        ops.WordpieceTokenizer(tok["suffix_indicator"], tok["max_bytes_per_word"], lib=lib))
        consts = list(pack_strings(tok["vocab"])) + [np.asarray(tok["unk_id"], np.int32)]
        return lambda rows: fused.evaluate(data(rows), u8(BERT_WS), u8(BERT_PUNCT), consts)
    t = load_tokenizer(tok_name)
    added = dict(t["added"])
    if variant == "wide-ids":
        added[b"<|wide|>"] = WIDE_ID
    tok = BpeTok(t["vocab"], t["merges"], added, t["pattern"], **t["attrs"])
    pat = u8(MODEL_PATTERNS.get(pattern, pattern) if pattern else tok.pattern)
    attrs = dict(tok.attrs)
    if not g["memo"]:
        attrs["cache_capacity"] = 0
    bpe = ops.BPETokenizer(**attrs, lib=lib)
    split = ops.RegexSplit("isolate", max_splits=1 if front == "max-splits-1" else -1, lib=lib)
    special_pat = u8(O.special_tokens_pattern([("<|endoftext|>", False, False)]))
    if front == "bpe-alone":   # the two ops one after the other
        return lambda rows: bpe.evaluate(list(split.evaluate(data(rows) + [pat])[:5]) + tok.consts)
    if variant in ("ragged", "wide-ids"):
        fused = ops.FusedSplitBPE(split, bpe)
        return lambda rows: fused.evaluate(data(rows) + [pat], tok.consts)
    if variant == "special":
        fused = ops.FusedSpecialSplitBPE(ops.SpecialTokensSplit(lib=lib), split, bpe)
        return lambda rows: fused.evaluate(data(rows) + [special_pat], pat, tok.consts)
    if variant in ("dense", "special-dense"):
        sp = ops.SpecialTokensSplit(lib=lib) if variant == "special-dense" else None
        fused = ops.FusedEncodeDense(split, bpe, special=sp, max_length=64, prefix=(1,), suffix=(2,))
        return lambda rows: fused.evaluate(data(rows), pat, tok.consts, special_pattern=special_pat if sp else None)
    assert variant == "wire"
    fused = ops.FusedSplitBPE(split, bpe)
    pad, id_bytes = 1 << 16, 4

    def to_wire(rows):
        max_rows = (rows + 3) // 4 * 4
        wire = _Buf(16 + 4 * max_rows + id_bytes * pad)
        return fused.enqueue_wire(data(rows) + [pat], tok.consts, wire, max_rows, pad, id_bytes, stream=0)()
    return to_wire


def census(lib, g):
    """Runs one group on `lib` (an emulator build) -> {step: {tag: launches, + the short-path counters of the step's calls}}.
    The first step's profile holds the launches of the handles' creation too."""
    from openvino_tokenizers_amd import _lib as L
    out = {}
    try:
        lib.ovtk_profile_enable(1)
        run = _runner(lib, g)
        for step in g["steps"]:
            mode, tickets, rows = step
            L.check(lib, lib.ovtk_set_short_path(mode))
            L.check(lib, lib.ovtk_set_row_tickets(tickets))
            lib.ovtk_profile_reset()
            t0, x0 = _stats(lib)
            for _ in range(CALLS):
                run(rows)
            got = _profile(lib)
            t1, x1 = _stats(lib)
            got["short_path.tried"], got["short_path.exact"] = t1 - t0, x1 - x0
            out[step_id(step)] = got
        return out
    finally:
        lib.ovtk_profile_enable(0)
        lib.ovtk_set_short_path(1)
        lib.ovtk_set_row_tickets(0)


def main():
    import time
    from openvino_tokenizers_amd import _lib as L
    lib = L.load(Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "emu" / "build" / "libovtk_emu.so")
    out = {}
    for g in groups():
        t = time.time()
        out[group_id(g)] = census(lib, g)
        print(f"{group_id(g)}: {time.time() - t:.1f} s", flush=True)
    FIXTURE.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(f"{len(out)} groups, {sum(len(v) for v in out.values())} cells -> {FIXTURE}")


if __name__ == "__main__":
    main()
