"""compact_stretch_kernel (encode_kernels.hpp): the tail of a fused encode whose rows lookup_span_kernel staged, one wave per stretch
of rows_per_wave rows.  The result is what the oracle's chain RegexSplit -> BPETokenizer gives (src/regex_split.cpp:124-324,
src/bpe_tokenizer.cpp) and what the same call gives with the short path off -- begins, ends and ids, bit for bit.

rows_per_wave follows from OVTK_SPAN_ROWS, which the library reads once per process: every R runs in a child process of its own
(one child per R and tier: it walks every row count and every kind of input with three handles).  Kinds of input:
  warm          a text the handle has seen (short-path mode 2: span -> compact at any size): every stretch is a plain copy
  first-sight   new words at every call, mode 1: merge_kernel runs between the two, stretches have unused entries (the squeeze)
  pending-rows  empty rows and skipped strings inside a stretch: rows of the generic kernel, the stretch goes row by row
  capacity      room for one id less than the result has: OVTK_E_CAPACITY, nothing written behind the capacity
  i32           a handle with an id above 65 535 (4-byte staging entries), first sight and second sight
Mode 1 takes the one-launch form for up to 256 rows / 64 KB of text, so those calls get a chars tensor with unreferenced bytes behind
the text (65 KB in all).  With fewer than ~33 rows that makes launch_tail share an item among several waves (compact_split > 1), which
is compact_kernel's: there the first-sight, pending-rows and i32 kinds check the selection, not the new kernel.
The launch counters (ovtk_profile_dump: tag -> launches of the one call) say that the call was ONE set of launches, lookup_span ...
compact -- a call that fell back to a second set has two of each."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
EMU_SO = ROOT / "tests" / "emu" / "build" / "libovtk_emu.so"
R_VALUES = (1, 3, 4, 13, 16, 64)
N_ROWS = (1, 15, 16, 17, 63, 64, 65, 130, 257)
WIDE_ID = 70000
PAD_CHARS = 65 << 10
SENTINEL = -123456789


def _text(seed, n, kind):
    """n rows -> (ragged_begins, ragged_ends, begins, ends, chars, skips or None).  Rows of 1..200 bytes of short words; `pending`: every
    fifth row empty, every seventh string (the first one too) skipped."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)
    rows = []
    for i in range(n):
        want = int(rng.integers(1, 201))
        if kind == "pending" and i % 5 == 2:
            rows.append(b"")
            continue
        words = []
        while sum(len(x) + 1 for x in words) < want:
            if kind == "warm":   # few distinct words of at most five letters: every piece fits a memo entry
                words.append(bytes(letters[(rng.integers(0, 40) * np.arange(1, 1 + int(rng.integers(1, 6)))) % 26]))
            else:
                words.append(bytes(rng.choice(letters, size=int(rng.integers(1, 10)))) + (b"," if rng.integers(0, 9) == 0 else b""))
        rows.append(b" ".join(words)[:want])
    lens = np.array([len(r) for r in rows], np.int64)
    e = np.cumsum(lens).astype(np.int32)
    b = (e - lens).astype(np.int32)
    c = np.frombuffer(b"".join(rows), np.uint8).copy()
    rb = np.arange(n, dtype=np.int32)
    skips = (np.arange(n) % 7 == 0) if kind == "pending" else None
    return rb, rb + 1, b, e, c, skips


def _child(tier, R):
    from openvino_tokenizers_amd import _lib as L
    from openvino_tokenizers_amd import ops
    from oracle import oracle as O
    from tests.gen_golden_launch_census import _profile, _stats
    from tools.harness import BpeTok
    from tools.make_tokenizers import load_tokenizer

    assert os.environ.get("OVTK_SPAN_ROWS") == str(R)
    lib = L.load(EMU_SO) if tier == "emu" else L.load()
    t = load_tokenizer("gpt2_small")
    tok = BpeTok(t["vocab"], t["merges"], dict(t["added"]), t["pattern"], **t["attrs"])
    wide = BpeTok(t["vocab"], t["merges"], {**dict(t["added"]), b"<|wide|>": WIDE_ID}, t["pattern"], **t["attrs"])
    pat = tok.pattern_u8()
    rs = O.RegexSplit(tok.pattern, "isolate")

    def handle(tk):
        return ops.FusedSplitBPE(ops.RegexSplit("isolate", lib=lib), ops.BPETokenizer(**tk.attrs, lib=lib)), tk

    h_first, h_warm, h_wide = handle(tok), handle(tok), handle(wide)
    failures, checks = [], [0]

    def check(ok, what):
        checks[0] += 1
        if not ok:
            failures.append(what)

    def reference(tk, inp):
        rb, re_, b, e, c, skips = inp
        return tk.oracle()(*rs(rb, re_, b, e, c, **({"skips": skips} if skips is not None else {}))[:5])

    def run(h, inp, padded):
        fused, tk = h
        rb, re_, b, e, c, skips = inp
        if padded:
            c = np.concatenate([c, np.zeros(PAD_CHARS - len(c), np.uint8)])
        args = [rb, re_, b, e, c] + ([skips.astype(np.uint8)] if skips is not None else [])
        return fused.evaluate(args + [pat], tk.consts)

    def same(ref, got, what):
        ok = len(ref) == len(got) and all(r.shape == np.asarray(g).shape and np.array_equal(r, g) for r, g in zip(ref, got))
        check(ok, f"{what}: differs from the oracle")

    def counted(h, inp, padded, ref, what, also=()):
        """One call with the launch counters around it: one set of launches, lookup_span first and compact last."""
        lib.ovtk_profile_reset()
        t0, x0 = _stats(lib)
        same(ref, run(h, inp, padded), what)
        prof = _profile(lib)
        t1, x1 = _stats(lib)
        check(prof.get("lookup_span") == 1 and prof.get("compact") == 1 and all(prof.get(k) == 1 for k in also),
              f"{what}: launches {prof}, not one set span ... compact")
        return t1 - t0, x1 - x0

    def long_path(h, inp, ref, what):
        L.check(lib, lib.ovtk_set_short_path(0))
        same(ref, run(h, inp, False), what + " (short path off)")

    def capacity(h, inp, n_ids, what):
        """ovtk_encode_run with room for n_ids - 1 ids.  The emulator's device memory is host memory: there the kernels write the
        arrays below themselves, and the words behind the capacity show what they did."""
        fused, tk = h
        rb, re_, b, e, c, _ = inp
        m = ops._Mem(c)
        rsin, keep = ops._ragged_in(m, [rb, re_, b, e, c])
        cap = n_ids - 1
        ob, oe = np.full(len(rb), SENTINEL, np.int32), np.full(len(rb), SENTINEL, np.int32)
        ids = np.full(cap + 64, SENTINEL, np.int32)
        out = L.RaggedI32Out(ob.ctypes.data, oe.ctypes.data, ids.ctypes.data, cap, 0, 0)
        rc = lib.ovtk_encode_run(fused.split._h, fused.bpe._h, C.byref(rsin), None, C.byref(out), L.MEM_DEVICE if tier == "emu" else L.MEM_HOST,
                                 m.stream)
        check(rc == L.E_CAPACITY, f"{what}: rc {rc}, not OVTK_E_CAPACITY")
        check(bool((ids[cap:] == SENTINEL).all()), f"{what}: ids written behind the capacity")

    try:
        lib.ovtk_profile_enable(1)
        # (a handle's very first call sizes its workspace and may launch twice: not one of the counted calls)
        L.check(lib, lib.ovtk_set_short_path(1))
        for h in (h_first, h_wide):
            run(h, _text(7, 40, "first"), True)
        for n in N_ROWS:
            tag = f"R={R} n_rows={n}"
            # first sight (u16 staging), then rows of the generic kernel, on one handle in mode 1
            first, pend = _text(1000 + n, n, "first"), _text(2000 + n, n, "pending")
            ref_first, ref_pend = reference(tok, first), reference(tok, pend)
            L.check(lib, lib.ovtk_set_short_path(1))
            counted(h_first, first, True, ref_first, f"{tag} first-sight")
            same(ref_pend, run(h_first, pend, True), f"{tag} pending-rows, first call")
            counted(h_first, pend, True, ref_pend, f"{tag} pending-rows", also=("lookup_fused",))   # (the handle now expects such rows)
            long_path(h_first, first, ref_first, f"{tag} first-sight")
            long_path(h_first, pend, ref_pend, f"{tag} pending-rows")
            # i32 staging: first and second sight
            L.check(lib, lib.ovtk_set_short_path(1))
            ref_wide = reference(wide, first)
            counted(h_wide, first, True, ref_wide, f"{tag} i32 first-sight")
            counted(h_wide, first, True, ref_wide, f"{tag} i32 second-sight")
            long_path(h_wide, first, ref_wide, f"{tag} i32")
            # warm: mode 2 until a call needs no other kernel, then the counted call; the capacity one id short
            warm = _text(3000 + n, n, "warm")
            ref_warm = reference(tok, warm)
            L.check(lib, lib.ovtk_set_short_path(2))
            for _ in range(4):
                x0 = _stats(lib)[1]
                same(ref_warm, run(h_warm, warm, False), f"{tag} warm, learning")
                if _stats(lib)[1] > x0:
                    break
            tried, exact = counted(h_warm, warm, False, ref_warm, f"{tag} warm")
            check((tried, exact) == (1, 1), f"{tag} warm: short-path counters +{tried} / +{exact}, not span -> compact alone")
            capacity(h_warm, warm, len(ref_warm[2]), f"{tag} capacity")
            tried, exact = counted(h_warm, warm, False, ref_warm, f"{tag} warm, after the capacity error")
            check((tried, exact) == (1, 1), f"{tag} warm, after the capacity error: short-path counters +{tried} / +{exact}")
            long_path(h_warm, warm, ref_warm, f"{tag} warm")
    finally:
        lib.ovtk_profile_enable(0)
        lib.ovtk_set_short_path(1)
    print(json.dumps({"checks": checks[0], "failures": failures}))
    return 1 if failures else 0


def _run_child(tier, R):
    env = dict(os.environ, OVTK_SPAN_ROWS=str(R))
    r = subprocess.run([sys.executable, "-m", "tests.test_compact_stretch", tier, str(R)], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"R = {R} on {tier}:\n{r.stdout[-4000:]}\n{r.stderr[-3000:]}"
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["checks"] > 20 * len(N_ROWS) and not res["failures"]


@pytest.mark.parametrize("R", R_VALUES)
def test_stretches_on_the_emulator(emu_lib, R):
    _run_child("emu", R)


@pytest.mark.gpu
@pytest.mark.parametrize("R", R_VALUES)
def test_stretches_on_the_gpu(hip_lib, R):
    _run_child("hip-host", R)


if __name__ == "__main__":
    sys.exit(_child(sys.argv[1], int(sys.argv[2])))
