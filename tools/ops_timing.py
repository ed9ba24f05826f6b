"""Times the ops of SURVEY 8(f) and the ops around the hot path that bench.py has no configuration for, one op = one library call,
on a config-2-shaped batch (65 536 rows x ~512 bytes of zipf text, a GPT-2 special token in one row in a hundred; the ids of that
batch for the ops behind the tokenizer), inputs and outputs in HBM:

    SentencepieceTokenizer (a fixture unigram model; beside it CharsMapNormalization followed by UnigramTokenizer on whole rows with the
    model's charsmap and pieces, the two calls the one call replaces, and the same op on a fixture BPE model, checked against the
    installed `sentencepiece` package on the first rows; --only-sentencepiece stops behind these rows),
    UTF8Validate (both modes), SpecialTokensSplit (the op: count pass, scan, write pass), RegexSplit (the op), StringTensorPack /
    StringTensorUnpack, TrieTokenizer, UnigramTokenizer, CharsMapNormalization, RegexNormalization, Truncate, CombineSegments, RaggedToDense (in bench.py too: --config r2d), the fused tail
    (ovtk_encode_tail_run: Truncate -> CombineSegments -> RaggedToDense x 2 in one call).

Per op one JSON line: wall time per call (Python + the library's host side + the kernels; the call returns when its results are
complete, so host waits are inside), the algorithmic bytes the op has to move (inputs read once + outputs written once) and the rate
they make, and whether a prefix of the result equals the oracle's.  The kernels' own durations: run this script under
`rocprofv3 --kernel-trace --stats` (profiles/README.md); VERDICT r04 weak 6 asked for both.

    python tools/ops_timing.py [--rows 65536] [--bytes 512] [--reps 10] [--check-rows 256] [--only-sentencepiece [--sp-profile]]

--only-sp-detok times SentencepieceDetokenizer and SentencepieceStreamDetokenizer instead, on one 16 384 x 2 048 id matrix (the
config-2 batch's first rows encoded with spm_unigram_bytes, padded with an id outside the vocabulary), and beside them, in the same
run, ovtk_detokenize_run with byte_fallback = 1 over the same piece list as a vocabulary -- a different algorithm with different
bytes, and the only yardstick there is.

    python tools/ops_timing.py --only-sp-detok [--detok-rows 16384] [--detok-seq 2048]

--only-tf-ops times the three ops of the TensorFlow front end and nothing else (the full run ends with them): StringToHashBucket over
whole rows and over the batch split on whitespace (a division and a mask as the modulo), EqualStr of the rows against one constant and
against themselves, RaggedToRagged on the row id of every word, and UTF8Validate on the same batch in the same run -- it also reads
every byte of the batch once: the yardstick for the whole-row hash.  The checks are tests/test_tf_string_ops.py's restatements on the
first rows.

--only-string-ops times BytesToChars (on the batch split by the GPT-2 pattern: the pieces a byte-level BPE graph hands it), CharsToBytes
(on its output), ContribStringSplit (the rows on " ") and ContribStringJoin (that back, along the last axis of the padded [rows, most
tokens] tensor), with UTF8Validate on the same batch in the same run.  The checks are tests/string_ops_ref.py on the first rows.

--only-numeric times NumericToString, one call per element type on 8 M values (--numeric-n): uniformly random bit patterns for f32 and
f64 (f64 once more with OVTK_NUM2STR_EXACT=1: every finite value through the exact big-integer comparison), values of a uniformly
random bit length for the integers, random bytes for boolean, and the batch's own token ids (the fused GPT-2 encode) as a realistic i32
column; UTF8Validate on the batch in the same run is the yardstick.  The checks are Python's '%g' and str on the first elements.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _proto_fields(buf):
    """(field, wire type, value) of one protobuf message; the value of a length-delimited field is its bytes."""
    at = 0

    def varint():
        nonlocal at
        v = shift = 0
        while True:
            x = buf[at]
            at += 1
            v |= (x & 0x7F) << shift
            shift += 7
            if not x & 0x80:
                return v
    while at < len(buf):
        tag = varint()
        wt = tag & 7
        if wt == 0:
            val = varint()
        elif wt == 2:
            ln = varint()
            val = bytes(buf[at:at + ln])
            at += ln
        else:
            ln = 8 if wt == 1 else 4
            val = bytes(buf[at:at + ln])
            at += ln
        yield tag >> 3, wt, val


def sp_model_tables(model):
    """A sentencepiece ModelProto's pieces, scores and precompiled charsmap (what csrc/sp_model.hpp reads, for the two-call baseline)."""
    pieces, scores, blob = [], [], b""
    for f, _, v in _proto_fields(bytes(model)):
        if f == 1:
            d = {ff: vv for ff, _, vv in _proto_fields(v)}
            pieces.append(d.get(1, b""))
            scores.append(np.frombuffer(d.get(2, bytes(4)), np.float32)[0])
        elif f == 3:
            blob = {ff: vv for ff, _, vv in _proto_fields(v)}.get(2, b"")
    return pieces, np.array(scores, np.float32), blob


def pair_timing(args):
    """Paired input (pipeline.add_second_input, tokenizer_transformations.py:22-304): wall time per batch of the one call
    (ovtk_*_pair_dense_enqueue / _finish), of the two-call form (the fused encode on all rows, then ovtk_encode_tail_run over the halves)
    and of the op-by-op chain -- the config-3 text (BERT fixture) and the config-2 text (GPT-2 fixture), each split into two halves of
    rows / 2 rows, in one run.  One JSON line per form; the three must agree bit for bit before anything is timed."""
    import json
    import time
    from openvino_tokenizers_amd import _lib as L
    from openvino_tokenizers_amd import pipeline as P
    from tools.harness import BpeTok, pack_strings
    from tools.make_tokenizers import load_tokenizer
    from tools.workloads import TextModel
    if args.emu:
        lib = L.load(Path(__file__).resolve().parent.parent / "tests" / "emu" / "build" / "libovtk_emu.so")
        sync, place = (lambda: None), (lambda a: a)
    else:
        import torch
        lib = L.load()
        sync, place = torch.cuda.synchronize, (lambda a: torch.as_tensor(a, device="cuda:0"))
    half = args.rows // 2
    small = "_small" if args.emu else ""

    def halves(lower):   # (config 3: ~256-byte lower-cased rows; config 2: ~--bytes-byte rows)
        b, e, c = TextModel(1234, "zipf").batch(2 * half, min(256, args.bytes) if lower else args.bytes, seed=1000)
        if lower:
            c = np.frombuffer(c.tobytes().lower(), np.uint8).copy()
        cut = int(e[half - 1])
        return [place(x) for x in (b[:half], e[:half], c[:cut])], [place(x) for x in (b[half:] - cut, e[half:] - cut, c[cut:])]
    bert = load_tokenizer("bert" + small)
    gpt2 = BpeTok.load("gpt2" + small)
    bert_consts = list(pack_strings(bert["vocab"])) + [np.asarray(bert["unk_id"], np.int32)]
    cls, sep = bert["vocab"].index(b"[CLS]"), bert["vocab"].index(b"[SEP]")
    graphs = {
        "BERT, config-3 text": (True, [P.RegexSplitStep(P.BERT_WS, "remove", lib=lib), P.RegexSplitStep(P.BERT_PUNCT, "isolate", lib=lib),
                                       P.WordPieceTokenizationStep(bert_consts, bert["suffix_indicator"], bert["max_bytes_per_word"], lib=lib),
                                       P.TruncationStep(126, "right", lib=lib), P.CombineSegmentsStep([cls], [sep], lib=lib), P.PaddingStep(0, lib=lib)],
                                [cls, -1, sep], [cls, -1, sep, -2, sep], [0, 0, 0, 1, 1]),
        "GPT-2, config-2 text": (False, [P.RegexSplitStep(gpt2.pattern, "isolate", lib=lib), P.BPETokenizationStep(gpt2.consts, lib=lib, **gpt2.attrs),
                                         P.TruncationStep(254, "right", lib=lib), P.CombineSegmentsStep([0], [2], lib=lib), P.PaddingStep(1, lib=lib)],
                                 [0, -1, 2], [0, -1, 2, 2, -2, 2], [0] * 6),
    }
    lines = []
    for name, (lower, steps, single, pair, types) in graphs.items():
        first, second = halves(lower)
        chain = P.Pipeline(P.add_second_input(steps, single, pair, types))
        one, two = chain.fused(), chain.fused()
        two.steps[-1].two_call = True
        forms = {"one call": one, "two calls": two, "op by op": chain}
        ref = None
        for form, pipe in forms.items():
            out = [np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in pipe.run_pair(first, second)]
            ref = ref or out
            assert all(np.array_equal(a, r) for a, r in zip(out, ref)), f"{name}: {form} differs from the one call"
        for form, pipe in forms.items():
            times = []
            for _ in range(args.reps):
                sync()
                t0 = time.perf_counter()
                pipe.run_pair(first, second)
                sync()
                times.append(time.perf_counter() - t0)
            lines.append(dict(graph=name, form=form, pairs=half, bytes_per_row=min(256, args.bytes) if lower else args.bytes, width=int(ref[0].shape[1]), reps=args.reps,
                              ms_median=round(1e3 * float(np.median(times)), 4), ms_min=round(1e3 * min(times), 4)))
            print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--bytes", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--check-rows", type=int, default=256)
    ap.add_argument("--only-sentencepiece", action="store_true", help="the SentencepieceTokenizer rows and nothing else")
    ap.add_argument("--sp-profile", action="store_true", help="behind the SentencepieceTokenizer rows: the library's per-launch profile of the 4- and the 8-input call")
    ap.add_argument("--only-sp-detok", action="store_true", help="the two sentencepiece detokenizers beside ovtk_detokenize_run and nothing else")
    ap.add_argument("--only-tf-ops", action="store_true", help="StringToHashBucket, EqualStr, RaggedToRagged beside UTF8Validate and nothing else")
    ap.add_argument("--only-string-ops", action="store_true", help="BytesToChars, CharsToBytes, ContribStringSplit, ContribStringJoin beside UTF8Validate and nothing else")
    ap.add_argument("--only-numeric", action="store_true", help="NumericToString per element type beside UTF8Validate and nothing else")
    ap.add_argument("--only-pair", action="store_true", help="paired input: the one call beside the two-call form and the op-by-op chain, and nothing else")
    ap.add_argument("--out", default=None, help="--only-pair: also append the JSON lines to this file")
    ap.add_argument("--numeric-n", type=int, default=8 << 20)
    ap.add_argument("--detok-rows", type=int, default=16384)
    ap.add_argument("--detok-seq", type=int, default=2048)
    ap.add_argument("--emu", action="store_true", help="the SIMT-emulator build on host arrays (a smoke test of this script; the times mean nothing)")
    args = ap.parse_args()
    if args.only_pair:
        pair_timing(args)
        return
    from openvino_tokenizers_amd import _lib as L
    from openvino_tokenizers_amd.ops import (BPETokenizer, CombineSegments, FusedEncodeTail, FusedSplitBPE, RaggedToDense, RegexSplit,
                                             SpecialTokensSplit, StringTensorPack, StringTensorUnpack, TrieTokenizer, Truncate, UTF8Validate)
    from oracle import oracle as O
    from tools.harness import BpeTok, pack_strings
    from tools.workloads import TextModel, ragged_rows

    if args.emu:
        lib = L.load(Path(__file__).resolve().parent.parent / "tests" / "emu" / "build" / "libovtk_emu.so")

        def sync():
            pass
    else:
        import torch
        lib = L.load()
        dev = torch.device("cuda", 0)
        sync = torch.cuda.synchronize
    tok = BpeTok.load("gpt2")
    if args.only_sp_detok:
        args.rows = args.detok_rows
    n = args.rows
    b, e, c = TextModel(1234, "zipf").batch(n, args.bytes, seed=1000)
    rng = np.random.default_rng(1)
    special = np.frombuffer(b"<|endoftext|>", np.uint8)
    for i in np.flatnonzero(rng.random(n) < 0.01):
        if e[i] - b[i] > 2 * len(special):
            at = int(b[i]) + int(rng.integers(0, e[i] - b[i] - len(special)))
            c[at:at + len(special)] = special
    rb, re_ = ragged_rows(n)
    host = [rb, re_, b, e, c]
    d = host if args.emu else [torch.as_tensor(x, device=dev) for x in host]
    k = min(args.check_rows, n)
    head = [rb[:k], re_[:k], b[:k], e[:k], c[: int(e[k - 1])]]

    def to_np(x):
        return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)

    def same(ref, got, upto=None):
        for r, g in zip(ref, got):
            g = to_np(g)
            r = np.asarray(r)
            m = len(r) if upto is None else min(len(r), upto)
            if not np.array_equal(r.reshape(-1)[:m], g.reshape(-1)[:m]):
                return False
        return True

    def timed(name, fn, algo_bytes, check=None, note=""):
        for _ in range(2):
            out = fn()
        sync()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            out = fn()
        sync()
        dt = (time.perf_counter() - t0) / args.reps
        ok = None if check is None else bool(check(out))
        print(json.dumps({"op": name, "ms_per_call": round(dt * 1e3, 4), "algorithmic_MB": round(algo_bytes / 1e6, 2),
                          "GB_per_s": round(algo_bytes / dt / 1e9, 1), "rows": n, "prefix_equals_oracle": ok, "note": note}), flush=True)
        return out

    n_c = len(c)

    def tf_ops():
        # ---- StringToHashBucket (src/string_to_hash_bucket.cpp:204-220), EqualStr (src/equal_str.cpp:29-61), RaggedToRagged
        # (src/ragged_to_ragged.cpp:43-98); UTF8Validate beside them: the other op that reads every byte of the batch once
        from openvino_tokenizers_amd.ops import EqualStr, RaggedToRagged, StringToHashBucket
        from tests.test_tf_string_ops import equal_ref, fingerprint64, ragged_ref
        uv = UTF8Validate(replace_mode=False, lib=lib)
        timed("UTF8Validate(replace_mode=False), the yardstick", lambda: uv.evaluate(d[2:5]), 2 * n_c + 16 * n, None,
              "reads every byte once and writes it once; count -> scan -> write, a wave per string")
        rows = [bytes(c[int(b[i]):int(e[i])]) for i in range(k)]
        row_hashes = [fingerprint64(r) for r in rows]
        for nb, how in ((1000, "64-bit division"), (1 << 20, "mask")):
            op = StringToHashBucket(nb, lib=lib)
            timed(f"StringToHashBucket(num_buckets={nb}), whole rows", lambda op=op: op.evaluate(d[2:5]), n_c + 16 * n,
                  lambda out, nb=nb: same([np.array([h % nb for h in row_hashes], np.int64)], [to_np(out[0])[:k]]),
                  f"a lane per row streams its own ~{args.bytes} bytes, 64 per round of the loop; the modulo is a {how}")
        ws_out = RegexSplit("remove", lib=lib).evaluate(d + [np.frombuffer(rb"\s+", np.uint8)])
        n_words = len(ws_out[2])
        wb, we = to_np(ws_out[2]), to_np(ws_out[3])
        kw = min(4096, n_words)
        word_hashes = [fingerprint64(bytes(c[int(wb[i]):int(we[i])])) for i in range(kw)]
        for nb, how in ((1000, "64-bit division"), (1 << 20, "mask")):
            op = StringToHashBucket(nb, lib=lib)
            timed(f"StringToHashBucket(num_buckets={nb}), the batch split on whitespace", lambda op=op: op.evaluate(list(ws_out[2:5])),
                  n_c + 16 * n_words, lambda out, nb=nb: same([np.array([h % nb for h in word_hashes], np.int64)], [to_np(out[0])[:kw]]),
                  f"{n_words} strings, a lane each: the 0-16 byte branches; the modulo is a {how}")
        eq = EqualStr(lib=lib)
        const = [np.array([3], np.int32), np.array([3 + len(rows[0])], np.int32), np.frombuffer(b"xyz" + rows[0], np.uint8)]
        const_d = const if args.emu else [torch.as_tensor(x, device=dev) for x in const]
        timed("EqualStr(rows, one constant)", lambda: eq.evaluate(d[2:5] + const_d), 12 * n, lambda out: same([equal_ref(rows, [rows[0]])], [to_np(out[0])[:k]]),
              "the constant is row 0: bytes are compared only where the lengths agree (offsets in, i32 out)")
        timed("EqualStr(rows, rows)", lambda: eq.evaluate(d[2:5] + d[2:5]), 2 * n_c + 20 * n, lambda out: same([equal_ref(rows, rows)], [to_np(out[0])[:k]]),
              "both operands the same tensors: every byte is fetched twice, eight at a time, a lane per row")
        counts = to_np(ws_out[1]).astype(np.int64) - to_np(ws_out[0])
        rowids = np.repeat(np.arange(n, dtype=np.int32), counts)
        rowids_d = rowids if args.emu else torch.as_tensor(rowids, device=dev)
        ref_r = ragged_ref(rowids, k)   # (stops at the first id >= k: rows 0 .. k - 2 are the whole batch's)
        r2r = RaggedToRagged(lib=lib)
        timed("RaggedToRagged(row id of every word)", lambda: r2r.evaluate([rowids_d, np.array([n], np.int32)]), 4 * len(rowids) + 8 * n,
              lambda out: same([ref_r[0][:k - 1], ref_r[1][:k - 1]], [to_np(out[0])[:k - 1], to_np(out[1])[:k - 1]]),
              f"{len(rowids)} ids, batch_size {n}: a lane per id, run starts write")
    def string_ops():
        # ---- BytesToChars (src/bytes_to_chars.cpp:284-339), CharsToBytes (src/chars_to_bytes.cpp:31-68), ContribStringSplit / Join
        # (src/contrib_string_ops.cpp:225-343, :62-199); UTF8Validate beside them: the same bytes read once and written once
        from openvino_tokenizers_amd.ops import BytesToChars, CharsToBytes, ContribStringJoin, ContribStringSplit
        from tests import string_ops_ref as R
        uv = UTF8Validate(replace_mode=False, lib=lib)
        timed("UTF8Validate(replace_mode=False), the yardstick", lambda: uv.evaluate(d[2:5]), 2 * n_c + 16 * n, None,
              "reads every byte once and writes it once; count -> scan -> write, a wave per string")
        rows = [bytes(c[int(b[i]):int(e[i])]) for i in range(k)]
        pieces = RegexSplit("isolate", lib=lib).evaluate(d + [tok.pattern_u8()])[:5]
        n_p = len(pieces[2])
        prb, pre_ = to_np(pieces[0])[:k], to_np(pieces[1])[:k]
        m = int(pre_[-1])
        head_ref = R.bytes_to_chars(prb, pre_, to_np(pieces[2])[:m], to_np(pieces[3])[:m], c)
        # every timed call is given its capacities: without them the mirror classes size the outputs themselves, a reduction over all
        # offsets and a host wait per call that the yardstick does not pay
        piece_bytes = int((to_np(pieces[3]).astype(np.int64) - to_np(pieces[2])).sum())
        b2c = timed("BytesToChars(the batch split by the GPT-2 pattern)", lambda: BytesToChars(lib=lib).evaluate(list(pieces), chars_capacity=2 * piece_bytes), 2 * n_c + 16 * n_p,
                    lambda out: same([head_ref[0], head_ref[1], head_ref[2]], [to_np(out[2])[:m], to_np(out[3])[:m], to_np(out[4])[:len(head_ref[2])]]),
                    f"{n_p} pieces: cover -> count (a lane per piece) -> two scans -> a lane per input byte, 2 048 bytes per block")
        timed("CharsToBytes(its output)", lambda: CharsToBytes(lib=lib).evaluate(list(b2c[:5]), chars_capacity=len(b2c[4])), 2 * n_c + 8 * n_p + 8 * n,
              lambda out: [bytes(to_np(out[2])[x:y]) for x, y in zip(to_np(out[0])[:k], to_np(out[1])[:k])] == rows,
              "the same passes backwards; every byte is checked against the map's 256 characters")
        sp_in = d[2:5] + [np.frombuffer(b" ", np.uint8), np.asarray([0], np.uint8)]
        head_sp = R.string_split(b[:k], e[:k], c, b" ", False)
        nv = len(head_sp[1])
        sized = ContribStringSplit(lib=lib)
        sized.evaluate(sp_in)   # (untimed: the sizes the timed calls are given)
        sp = timed('ContribStringSplit(rows, " ")', lambda: ContribStringSplit(lib=lib).evaluate(sp_in, values_capacity=sized.needed_values, chars_capacity=sized.needed_chars),
                   2 * n_c + 8 * n,
                   lambda out: same([head_sp[0], head_sp[1], head_sp[2], head_sp[3]], [to_np(out[0])[:nv], to_np(out[1])[:nv], to_np(out[2])[:nv], to_np(out[3])[:len(head_sp[3])]]),
                   "a wave per row, 64 positions a step: occurrences by ballot -> two scans -> the same walk writes (+ 16 bytes of indices and 8 of offsets per token)")
        idx, vb, ve, vc, dense = sp
        most = int(dense[1])
        if args.emu:
            db, de = np.zeros((n, most), np.int32), np.zeros((n, most), np.int32)
        else:
            db, de = torch.zeros((n, most), dtype=torch.int32, device=dev), torch.zeros((n, most), dtype=torch.int32, device=dev)
        db[idx[:, 0], idx[:, 1]], de[idx[:, 0], idx[:, 1]] = vb, ve
        counts = np.bincount(to_np(idx[:, 0])[:nv], minlength=k)[:k]
        jn_in = [db, de, vc, np.frombuffer(b" ", np.uint8), np.asarray([-1])]
        timed(f"ContribStringJoin([rows, {most}], axis -1)", lambda: ContribStringJoin(lib=lib).evaluate(jn_in, chars_capacity=len(vc) + n * (most - 1)), 2 * n_c + 8 * n * most,
              lambda out: [bytes(to_np(out[2])[x:y]) for x, y in zip(to_np(out[0])[:k], to_np(out[1])[:k])] == [r + b" " * int(most - q) for r, q in zip(rows, counts)],
              "a wave per row: count, scan, then the wave copies element after element (padding slots are empty elements, a separator each)")
    def numeric_ops():
        # ---- NumericToString (src/numeric_to_string.cpp:18-92); UTF8Validate beside it: the other count -> scan -> write op
        from openvino_tokenizers_amd.ops import NumericToString
        uv = UTF8Validate(replace_mode=False, lib=lib)
        timed("UTF8Validate(replace_mode=False), the yardstick", lambda: uv.evaluate(d[2:5]), 2 * n_c + 16 * n, None,
              "reads every byte once and writes it once; count -> scan -> write, a wave per string")
        m = args.numeric_n
        rng_n = np.random.default_rng(14)
        op = NumericToString(lib=lib)

        def column(name, arr, want, note, env=None):
            arr_d = arr if args.emu else torch.as_tensor(arr, device=dev)
            cap = op.bound(L.NUM_I8 + ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64", "bool"].index(arr.dtype.name), arr.size)
            texts = [want(v) for v in arr[:k].tolist()]
            ends = np.cumsum([len(t) for t in texts]).astype(np.int32)
            probe = op.evaluate([arr_d], chars_capacity=cap)
            n_text = len(probe[2])
            knob = os.environ.get("OVTK_NUM2STR_EXACT")
            if env:
                os.environ["OVTK_NUM2STR_EXACT"] = env
            try:
                timed(name, lambda: op.evaluate([arr_d], chars_capacity=cap), arr.nbytes + 8 * arr.size + n_text,
                      lambda out: same([ends, np.frombuffer(b"".join(texts), np.uint8)], [to_np(out[1])[:k], to_np(out[2])[:int(ends[-1])]]),
                      f"{arr.size} values, {n_text} bytes of text; {note}")
            finally:
                if env:
                    if knob is None:
                        del os.environ["OVTK_NUM2STR_EXACT"]
                    else:
                        os.environ["OVTK_NUM2STR_EXACT"] = knob

        def pct(v):
            return (("%g" % v) if v == v else ("-nan" if np.signbit(v) else "nan")).encode()
        f64 = rng_n.integers(0, 1 << 64, m, dtype=np.uint64).view(np.float64)
        f32 = rng_n.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32).view(np.float32)
        column("NumericToString(f64, random bit patterns)", f64, pct, "192-bit product per value; count formats, write formats again")
        column("NumericToString(f64, random bit patterns, exact path forced)", f64, pct, "OVTK_NUM2STR_EXACT=1: the big-integer comparison for every finite value", env="1")
        column("NumericToString(f32, random bit patterns)", f32, pct, "widened on the bits, then the f64 path")
        for name in ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64"):
            info = np.iinfo(name)
            bits = rng_n.integers(0, info.bits + 1, m).astype(np.uint64)
            mag = rng_n.integers(0, 1 << 64, m, dtype=np.uint64) >> (np.uint64(64) - np.maximum(bits, 1))
            mag[bits == 0] = 0
            arr = mag.astype(name) if info.min == 0 else (mag >> np.uint64(1)).astype(np.int64).astype(name) * rng_n.choice(np.array([-1, 1], name), m)
            column(f"NumericToString({name}, a uniformly random bit length)", arr, lambda v: str(v).encode(), "digit count from the bit length; two digits per division by 100")
        column("NumericToString(boolean, random bytes)", (rng_n.integers(0, 256, m, dtype=np.uint8) * rng_n.integers(0, 2, m, dtype=np.uint8)).view(np.bool_),
               lambda v: b"true" if v else b"false", "a byte in, 4 or 5 out")
        fused = FusedSplitBPE(RegexSplit("isolate", lib=lib), BPETokenizer(**tok.attrs, lib=lib))
        ids = to_np(fused.evaluate(d + [tok.pattern_u8()], tok.consts)[2]).astype(np.int32)
        column("NumericToString(i32, the batch's token ids)", ids, lambda v: str(v).encode(), "GPT-2 ids: 1 to 5 digits")
    if args.only_numeric:
        numeric_ops()
        return
    if args.only_string_ops:
        string_ops()
        return
    if args.only_tf_ops:
        tf_ops()
        return
    if args.only_sp_detok:
        # ---- SentencepieceDetokenizer / SentencepieceStreamDetokenizer (src/sentence_piece.cpp:395-433, :478-523)
        from openvino_tokenizers_amd.ops import (FusedDetokenizer, SentencepieceDetokenizer, SentencepieceStreamDetokenizer, SentencepieceTokenizer,
                                                 VocabDecoder)
        model = np.frombuffer((Path(__file__).resolve().parent.parent / "tests" / "golden" / "spm_unigram_bytes.model").read_bytes(), np.uint8)
        pieces = sp_model_tables(model)[0]
        V, S = len(pieces), args.detok_seq
        idx, val, shape = SentencepieceTokenizer(lib=lib).evaluate([model] + d[2:5])
        idx, val = to_np(idx), to_np(val)
        keep = idx[:, 1] < S
        ids_host = np.full((n, S), V, np.int32)
        ids_host[idx[keep, 0], idx[keep, 1]] = val[keep]
        ids = ids_host if args.emu else torch.as_tensor(ids_host, device=dev)
        n_ids = int(keep.sum())
        want = None
        try:
            import sentencepiece as spm
            sp = spm.SentencePieceProcessor(model_proto=bytes(model))
            want = [sp.decode([int(x) for x in row if x < V]).encode() for row in ids_host[:k]]
        except ImportError:
            pass

        def rows_equal(out):
            if want is None:
                return None
            ob, oe, oc = [to_np(x) for x in out]
            return [bytes(oc[ob[r]:oe[r]]) for r in range(k)] == want
        dec_op, str_op = SentencepieceDetokenizer(lib=lib), SentencepieceStreamDetokenizer(lib=lib)
        old = FusedDetokenizer(VocabDecoder(lib=lib), byte_fallback=True)
        vocab = list(pack_strings(pieces))
        n_out = len(dec_op.evaluate([model, ids])[2])
        cap = n_out + 64   # (the buffers are sized once: the stream op's text is longer where a space symbol stays three bytes)
        cap_raw = len(str_op.evaluate([model, ids])[2])
        n_old = len(old.evaluate([ids] + vocab)[2])
        for trial in range(3):
            timed(f"SentencepieceDetokenizer(spm_unigram_bytes), round {trial}", lambda: dec_op.evaluate([model, ids], chars_capacity=cap),
                  4 * n * S + n_out + 8 * n, rows_equal, f"{n} x {S} ids, {n_ids} in the vocabulary, {n_out} bytes out: first -> count -> scan -> write")
            timed(f"SentencepieceStreamDetokenizer(spm_unigram_bytes), round {trial}", lambda: str_op.evaluate([model, ids], chars_capacity=cap_raw),
                  4 * n * S + cap_raw + 8 * n, None, f"the same ids, {cap_raw} bytes out: count -> scan -> write over the raw pieces")
            timed(f"ovtk_detokenize_run(byte_fallback=1, the same pieces as a vocabulary), round {trial}", lambda: old.evaluate([ids] + vocab),
                  4 * n * S + n_old + 8 * n, None, f"{n_old} bytes out; VocabDecoder -> ByteFallback -> FuzeRagged in one call: other bytes (no spaces for the space symbol, control pieces kept)")
        return
    # ---- SentencepieceTokenizer (src/sentence_piece.cpp:188-350), the fixture unigram model with the nmt_nfkc charsmap: one call; beside
    # it the two calls it replaces, CharsMapNormalization then UnigramTokenizer over whole rows with the model's own tables (three
    # rounds of each, alternating: the spread of the pair is the yardstick for the one call).  The check: the one call's ids are the
    # pair's on the first rows (this text has no character the two treat differently).
    from openvino_tokenizers_amd.ops import CharsMapNormalization, SentencepieceTokenizer, UnigramTokenizer
    sp_model = np.frombuffer((Path(__file__).resolve().parent.parent / "tests" / "golden" / "spm_unigram_nfkc.model").read_bytes(), np.uint8)
    sp_pieces, sp_scores, sp_blob = sp_model_tables(sp_model)
    spb, spe, spc = pack_strings(sp_pieces)
    sp_op = SentencepieceTokenizer(lib=lib)
    sp_cm = CharsMapNormalization(True, True, True, charsmap=sp_blob, lib=lib)
    sp_uni = UnigramTokenizer(unk_token_id=0, lib=lib)

    def sp_pair():
        nb, ne, nc = sp_cm.evaluate(d[2:5])
        return sp_uni.evaluate([d[0], d[1], nb, ne, nc, spb, spe, spc, sp_scores])
    pair_head = [to_np(x) for x in sp_pair()]
    n_ids = int(len(pair_head[2]))
    head_ids = pair_head[2][:int(pair_head[1][k - 1])]
    bpe_model = np.frombuffer((Path(__file__).resolve().parent.parent / "tests" / "golden" / "spm_bpe_unk.model").read_bytes(), np.uint8)
    bpe_op = SentencepieceTokenizer(lib=lib)
    bpe_want = None
    try:
        import sentencepiece as spm
        bpe_sp = spm.SentencePieceProcessor(model_proto=bytes(bpe_model))
        bpe_want = np.array([x for r in range(k) for x in bpe_sp.encode(bytes(c[b[r]:e[r]]))], np.int32)
    except ImportError:
        pass

    def bpe_check(out):
        return bool(np.array_equal(to_np(out[1])[:len(bpe_want)], bpe_want)) and int(to_np(out[2])[0]) == n
    for trial in range(3):
        timed(f"CharsMapNormalization + UnigramTokenizer (whole rows, spm_unigram_nfkc), round {trial}", sp_pair, 3 * n_c + 32 * n + 4 * n_ids, None,
              "two calls, the normalized text and a host wait in between")
        timed(f"SentencepieceTokenizer(spm_unigram_nfkc), round {trial}", lambda: sp_op.evaluate([sp_model] + d[2:5]), n_c + 8 * n + 20 * n_ids,
              lambda out: same([head_ids], [to_np(out[1])], upto=len(head_ids)) and int(to_np(out[2])[0]) == n,
              f"{n_ids} ids: normalize (count, scan, write) -> edges -> relax -> scan -> sparse writer, one enqueue sequence")
        # the BPE fixture on the same batch, beside the unigram one (its yardstick); the check: the installed package on the first rows
        timed(f"SentencepieceTokenizer(spm_bpe_unk, a BPE model), round {trial}", lambda: bpe_op.evaluate([bpe_model] + d[2:5]), n_c + 8 * n + 20 * n_ids,
              bpe_check if bpe_want is not None else None, "normalize (count, scan, write) -> stretch scan -> merge (a wave per sentence) -> scan -> sparse writer, one enqueue sequence")
    # ---- the 8-input form (src/sentence_piece.cpp:200-230, :286-329; csrc/sp_special_kernels.hpp) beside the 4-input call on the same
    # batch in the same run: 1 % of the rows hold one of a handful of added tokens.  Alternating single calls, the median of `reps`.
    # The check: on the first rows, every part through the installed package and the tokens' ids between them.
    added = [b"<|endoftext|>", b"<s>", b"</s>", b"[INST]", b"[/INST]"]
    added_ids = [3000 + j for j in range(len(added))]
    c8 = c.copy()
    c8[c8 == ord("<")] = ord("(")   # (the 4-input call's batch is the same text; no token by accident)
    c8[c8 == ord("[")] = ord("(")
    rng8 = np.random.default_rng(2)
    for i in np.flatnonzero(rng8.random(n) < 0.01):
        t = np.frombuffer(added[int(rng8.integers(0, len(added)))], np.uint8)
        if e[i] - b[i] > 2 * len(t):
            at = int(b[i]) + int(rng8.integers(0, e[i] - b[i] - len(t)))
            # at character boundaries on both sides: a paste inside a multi-byte character would leave malformed UTF-8, where the
            # reference is undefined
            while at + len(t) <= e[i] and ((c8[at] & 0xC0) == 0x80 or (at + len(t) < e[i] and (c8[at + len(t)] & 0xC0) == 0x80)):
                at += 1
            if at + len(t) <= e[i]:
                c8[at:at + len(t)] = t
    d8 = [b, e, c8] if args.emu else [torch.as_tensor(x, device=dev) for x in (b, e, c8)]
    tb8, te8, tc8 = pack_strings(added)
    tok_in = [tb8, te8, tc8, np.array(added_ids, np.int32)]
    op4, op8 = SentencepieceTokenizer(lib=lib), SentencepieceTokenizer(lib=lib, special_tokens=True)
    want8 = None
    if bpe_want is not None:
        import re
        pat = re.compile(b"|".join(re.escape(t) for t in added))
        want8 = []
        for r in range(k):
            row, at = bytes(c8[b[r]:e[r]]), 0
            for m in pat.finditer(row):
                want8 += (bpe_sp.encode(row[at:m.start()]) if m.start() > at else []) + [added_ids[added.index(m.group())]]
                at = m.end()
            want8 += bpe_sp.encode(row[at:]) if at < len(row) else []
        want8 = np.array(want8, np.int32)
    for _ in range(2):
        out4, out8 = op4.evaluate([bpe_model] + d8), op8.evaluate([bpe_model] + d8 + tok_in)
    sync()
    t4, t8 = [], []
    for _ in range(args.reps):
        for ts, fn in ((t4, lambda: op4.evaluate([bpe_model] + d8)), (t8, lambda: op8.evaluate([bpe_model] + d8 + tok_in))):
            t0 = time.perf_counter()
            fn()
            sync()
            ts.append(time.perf_counter() - t0)
    n_tok = int(np.isin(to_np(out8[1]), added_ids).sum())
    ok8 = None if want8 is None else bool(np.array_equal(to_np(out8[1])[:len(want8)], want8)) and int(to_np(out8[2])[0]) == n
    for name, ts, note in (("SentencepieceTokenizer(spm_bpe_unk), 4 inputs, the special-token batch", t4, "the yardstick of the row below"),
                           ("SentencepieceTokenizer(spm_bpe_unk), 8 inputs, 5 added tokens in 1 % of the rows", t8,
                            f"{n_tok} token ids; cut (count, scan, host reads the slot count, write) -> the 4-input passes over the parts -> row lengths, scan, assemble")):
        print(json.dumps({"op": name, "ms_per_call": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "reps": len(ts),
                          "statistic": "median of single calls", "rows": n, "prefix_equals_package": ok8 if ts is t8 else None, "note": note}), flush=True)
    if args.sp_profile:
        # the library's own per-launch profile (ovtk_profile_*) of `reps` calls of each form: per tag the milliseconds summed over its
        # launches and their number -- what the two forms' kernels cost apart from the host side
        import ctypes as C
        for name, fn in (("4 inputs", lambda: op4.evaluate([bpe_model] + d8)), ("8 inputs", lambda: op8.evaluate([bpe_model] + d8 + tok_in))):
            sync()
            lib.ovtk_profile_enable(1)
            lib.ovtk_profile_reset()
            for _ in range(args.reps):
                fn()
            sync()
            size = int(lib.ovtk_profile_dump(None, C.c_int64(0)))
            buf = C.create_string_buffer(size + 1)
            lib.ovtk_profile_dump(buf, C.c_int64(size + 1))
            lib.ovtk_profile_enable(0)
            for line in buf.value.decode().splitlines():
                tag, ms, count = line.split()[:3]
                print(json.dumps({"profile_of": f"SentencepieceTokenizer(spm_bpe_unk), {name}, {args.reps} calls", "tag": tag, "ms_sum": float(ms),
                                  "launches": int(count)}), flush=True)
    if args.only_sentencepiece:
        return
    # ---- UTF8Validate (src/utf8_validate.cpp:18-143): strings in, strings out
    for mode in (False, True):
        op = UTF8Validate(replace_mode=mode, lib=lib)
        ref = O.utf8_validate(b[:k], e[:k], c, mode)
        timed(f"UTF8Validate(replace_mode={mode})", lambda op=op: op.evaluate(d[2:5]), 2 * n_c + 16 * n,
              lambda out, ref=ref: same(ref[:2], [to_np(out[0])[:k], to_np(out[1])[:k]]), "valid ASCII text: every byte is copied")
    # ---- SpecialTokensSplit, the op (src/special_tokens_split.cpp:61-162)
    sp_text = r"(\<\|endoftext\|\>)"   # what SpecialTokensSplitStep builds for this token (tokenizer_pipeline.py:138-159, quote_meta)
    sp_pat = np.frombuffer(sp_text.encode(), np.uint8)
    sp = SpecialTokensSplit(lib=lib)
    ref_sp = O.SpecialTokensSplit(sp_text)(*head)
    sp_out = timed("SpecialTokensSplit", lambda: sp.evaluate(d + [sp_pat]), n_c + 8 * n + 9 * n + 8 * n,
                   lambda out: same(ref_sp[:2], [to_np(out[0])[:k], to_np(out[1])[:k]]) and same([ref_sp[2], ref_sp[3]], [to_np(out[2]), to_np(out[3])], upto=len(ref_sp[2])),
                   "one row in a hundred holds the token; the op as the graph would run it alone (inside the fused encode: special_sparse_kernel, bench.py --config pipeline)")
    # ---- RegexSplit, the op (src/regex_split.cpp:124-324), GPT-2's pattern
    pat = tok.pattern_u8()
    rs = RegexSplit("isolate", lib=lib)
    ref_rs = O.RegexSplit(tok.pattern, "isolate")(*head)
    rs_out = timed("RegexSplit(isolate, GPT-2 pattern)", lambda: rs.evaluate(d + [pat]), n_c + 16 * n + 8 * (n_c // 4),
                   lambda out: same(ref_rs[:2], [to_np(out[0])[:k], to_np(out[1])[:k]]) and same([ref_rs[2], ref_rs[3]], [to_np(out[2]), to_np(out[3])], upto=len(ref_rs[2])),
                   "the op alone: pieces as begins / ends (inside the fused encode the pieces never exist)")
    # ---- BPETokenizer, the op (src/bpe_tokenizer.cpp:47-164): the pieces of the RegexSplit above in, ragged ids out -- what a graph
    # that is not fused runs behind RegexSplit
    bpe_op = BPETokenizer(**tok.attrs, lib=lib)
    ref_bpe = tok.oracle()(*ref_rs[:5])
    n_pieces = len(rs_out[2])
    timed("BPETokenizer (pre-split pieces)", lambda: bpe_op.evaluate(list(rs_out[:5]) + tok.consts), n_c + 8 * n_pieces + 16 * n + 4 * (n_c // 4),
          lambda out: same(ref_bpe[:2], [to_np(out[0])[:k], to_np(out[1])[:k]]) and same([ref_bpe[2]], [to_np(out[2])], upto=len(ref_bpe[2])),
          f"{n_pieces} pieces: lookup_kernel<kPieces> -> merge_kernel -> compact_kernel")
    del rs_out, sp_out
    # ---- StringTensorPack / Unpack (src/string_tensor_pack.cpp:40-86, string_tensor_unpack.cpp:45-78)
    pk = StringTensorPack(lib=lib)
    packed = timed("StringTensorPack", lambda: pk.evaluate(d[2:5], to_host=args.emu), 2 * n_c + 12 * n, None, "device to device")
    un = StringTensorUnpack(lib=lib)
    timed("StringTensorUnpack", lambda: un.evaluate([packed[0]]), 2 * n_c + 12 * n,
          lambda out: same([b[:k], e[:k]], [to_np(out[0])[:k], to_np(out[1])[:k]]), "packed u8 tensor on the device -> begins / ends / chars")
    # ---- TrieTokenizer (src/trie_tokenizer.cpp:23-81): the vocabulary's strings as the trie, longest match, unknown bytes skipped
    vb, ve, vc = pack_strings(tok.vocab)
    idx = np.arange(len(tok.vocab), dtype=np.int32)
    tr = TrieTokenizer(lib=lib)
    ref_tr = O.TrieTokenizer(tok.vocab, idx)(*head)
    tr_out = timed("TrieTokenizer", lambda: tr.evaluate(d + [vb, ve, vc, idx]), n_c + 16 * n + 4 * (n_c // 3),
                   lambda out: same(ref_tr[:2], [to_np(out[0])[:k], to_np(out[1])[:k]]) and same([ref_tr[2]], [to_np(out[2])], upto=len(ref_tr[2])),
                   f"V = {len(tok.vocab)} (the GPT-2-shaped vocabulary's strings), a lane per 64-byte segment + a lane per row that stitches them")
    del tr_out
    # ---- UnigramTokenizer (src/unigram_tokenizer.cpp:17-77): the same batch split on whitespace, a vocabulary from the batch's own lexicon
    # (all single bytes + its words and their prefixes, scores multiples of 1/64); the check is tests/unigram_ref.py on the first rows
    from collections import Counter
    from openvino_tokenizers_amd.ops import UnigramTokenizer
    from tests.unigram_ref import UnigramRef
    words = Counter(bytes(c).split())
    uni_vocab = [bytes([x]) for x in range(256)]
    known = set(uni_vocab)
    for wd in words:
        for ln in range(2, min(len(wd), 64) + 1):
            if wd[:ln] not in known:
                known.add(wd[:ln])
                uni_vocab.append(wd[:ln])
    uni_scores = (-np.random.default_rng(7).integers(0, 2048, len(uni_vocab)) / 64).astype(np.float32)
    steps = 0   # edges followed + probes that found none, over every character start of the batch's words
    for wd, times in words.items():
        here = 0
        for p0 in range(len(wd)):
            if p0 and (wd[p0] & 0xC0) == 0x80:
                continue
            ln = 0
            while p0 + ln < len(wd) and wd[p0:p0 + ln + 1] in known:
                ln += 1
            here += ln + (1 if p0 + ln < len(wd) else 0)
        steps += here * times
    ws_op = RegexSplit("remove", lib=lib)
    ws_out = ws_op.evaluate(d + [np.frombuffer(rb"\s+", np.uint8)])
    n_words = len(ws_out[2])
    uvb, uve, uvc = pack_strings(uni_vocab)
    uni = UnigramTokenizer(unk_token_id=0, lib=lib)
    wb, we = to_np(ws_out[2]), to_np(ws_out[3])
    ref_u = UnigramRef(uni_vocab, uni_scores, 0)(to_np(ws_out[0])[:k], to_np(ws_out[1])[:k], wb, we, c)
    timed("UnigramTokenizer", lambda: uni.evaluate(list(ws_out[:5]) + [uvb, uve, uvc, uni_scores]), n_c + 8 * n_words + 16 * n + 4 * n_words,
          lambda out: same(ref_u[:2], [to_np(out[0])[:k], to_np(out[1])[:k]]) and same([ref_u[2]], [to_np(out[2])], upto=len(ref_u[2])),
          f"V = {len(uni_vocab)} (256 bytes + the batch's {len(words)} words and their prefixes), {n_words} strings, {steps} trie steps: a lane per byte "
          "walks the trie, a lane per string relaxes and back-tracks")
    del ws_out
    # ---- CharsMapNormalization (src/charsmap_normalization.cpp:34-69): sentencepiece's nmt_nfkc_cf table (tests/golden/golden_charsmap.npz) with
    # XLM-RoBERTa's flags, on the batch as it is and with 5 % of its characters replaced by capitals, which the table rewrites; the check
    # is tests/charsmap_ref.py on the first rows
    from openvino_tokenizers_amd.ops import CharsMapNormalization
    from tests.charsmap_ref import CharsMapRef
    cm_blob = bytes(np.load(Path(__file__).resolve().parent.parent / "tests" / "golden" / "golden_charsmap.npz")["blob_nmt_nfkc_cf"])
    cm_flags = dict(add_dummy_prefix=True, remove_extra_whitespaces=True, escape_whitespaces=True)
    cm_ref = CharsMapRef(cm_blob, **cm_flags)
    c_rw = c.copy()
    c_rw[np.random.default_rng(3).random(n_c) < 0.05] = ord("Q")
    for label, text in (("as is", c), ("5 % rewritten", c_rw)):
        cm = CharsMapNormalization(lib=lib, **cm_flags)
        d_text = text if args.emu else torch.as_tensor(text, device=dev)
        ref_cm = cm_ref(b[:k], e[:k], text)
        cm_out = timed(f"CharsMapNormalization(nmt_nfkc_cf, {label})", lambda cm=cm, d_text=d_text: cm.evaluate([d[2], d[3], d_text, np.frombuffer(cm_blob, np.uint8)]),
                       n_c + 16 * n + int(n_c * 1.03), lambda out, ref_cm=ref_cm: same(ref_cm[:2], [to_np(out[0])[:k], to_np(out[1])[:k]]) and same([ref_cm[2]], [to_np(out[2])], upto=len(ref_cm[2])),
                       "a wave per row counts, a scan, a wave per row writes: the trie is walked twice")
        del cm_out
    # ---- RegexNormalization (src/regex_normalization.cpp:127-153): BERT's four regex normalizers (tokenizer_pipeline.py:224-278) and the
    # detokenizer's clean-up pattern (:1380-1384) on the same batch -- ASCII zipf text: `\s` and the clean-up pattern find matches in it,
    # the control-character, Han and \p{Mn} patterns find none (their figures are the no-match case).  The class-path patterns run
    # again with OVTK_REGEX_NORM_GENERAL=1; the check and the CPU baseline are tests/pcre2_substitute.py (one core) on the first rows
    from openvino_tokenizers_amd.ops import RegexNormalization
    from openvino_tokenizers_amd.pipeline import RegexDecodingStep, RegexNormalizationStep
    from tests.pcre2_substitute import normalize as pcre2_normalize

    class _Spec:
        def __init__(self, regex_search_pattern, replace_term, global_replace=True, lib=None):
            self.args = (regex_search_pattern, replace_term, global_replace)
    head_strings = [bytes(c[int(b[i]):int(e[i])]) for i in range(k)]
    knob = os.environ.get("OVTK_REGEX_NORM_GENERAL")
    for label, cls, ctor, class_path in (("\\s -> ' '", RegexNormalizationStep, "replace_whitespace_regex", True),
                                         ("control characters deleted", RegexNormalizationStep, "del_control_chars_regex", True),
                                         ("Han isolated", RegexNormalizationStep, "handle_chinese_chars_regex", True),
                                         ("\\p{Mn} deleted", RegexNormalizationStep, "strip_accents_regex", True),
                                         ("clean_up_tokenization_spaces", RegexDecodingStep, "clean_up_tokenization_spaces", False)):
        pattern, replace, g = getattr(cls, ctor).__func__(_Spec).args
        t0 = time.perf_counter()
        ref_rn = pcre2_normalize(head_strings, pattern, replace, g)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        cpu_bytes = sum(len(x) for x in head_strings)
        consts = [np.frombuffer(pattern.encode(), np.uint8), np.frombuffer(replace.encode(), np.uint8)]
        for forced in (("", "1") if class_path else ("",)):
            os.environ["OVTK_REGEX_NORM_GENERAL"] = forced
            rn = RegexNormalization(g, lib=lib)
            rn._ensure(*consts)   # (the knob is read at create)
            if knob is None:
                del os.environ["OVTK_REGEX_NORM_GENERAL"]
            else:
                os.environ["OVTK_REGEX_NORM_GENERAL"] = knob
            path = "general path forced" if forced else ("class path" if class_path else "general path")
            timed(f"RegexNormalization({label}, {path})", lambda rn=rn: rn.evaluate(d[2:5] + consts), 2 * n_c + 16 * n,
                  lambda out: same(ref_rn[:2], [to_np(out[0])[:k], to_np(out[1])[:k]]) and same([ref_rn[2]], [to_np(out[2])], upto=len(ref_rn[2])),
                  f"count -> scan -> write; PCRE2 on one core: {cpu_ms:.2f} ms for the first {k} rows ({cpu_bytes / cpu_ms / 1e6:.3f} GB/s)")
    # ---- the ids of the batch (the fused encode), then the ops behind the tokenizer
    fused = FusedSplitBPE(RegexSplit("isolate", lib=lib), BPETokenizer(**tok.attrs, lib=lib))
    ib, ie, ids = fused.evaluate(d + [pat], tok.consts)
    n_t = int(len(ids))
    ibh, ieh, idh = to_np(ib), to_np(ie), to_np(ids)
    max_len = 64
    tc = Truncate(lib=lib)
    ref_t = O.truncate([(ibh[:k], ieh[:k])], max_len, "right", "longest_first")
    t_out = timed("Truncate(max_length=64, right)", lambda: tc.evaluate([ib, ie, ids, np.array([max_len], np.int32), b"right", b"longest_first"]),
                  16 * n, lambda out: same(ref_t[0][:2], [to_np(out[0])[:k], to_np(out[1])[:k]]), "offsets only: the data tensor passes through")
    bos = (np.array([0], np.int32), np.array([1], np.int32), np.array([50256], np.int32))
    bos_d = bos if args.emu else tuple(torch.as_tensor(x, device=dev) for x in bos)   # (constants of the graph: resident like everything else)
    cs = CombineSegments(lib=lib)
    seg_ids = np.array([0, 0, 0], np.int32)
    ref_c = O.combine_segments([bos, (ref_t[0][0], ref_t[0][1], idh), bos], seg_ids)
    kept = int(np.minimum(ieh - ibh, max_len).sum())
    c_out = timed("CombineSegments(bos + truncated ids + eos)", lambda: cs.evaluate(list(bos_d) + [t_out[0], t_out[1], ids] + list(bos_d) + [seg_ids]),
                  4 * kept + 2 * 4 * (kept + 2 * n) + 16 * n,
                  lambda out: same(ref_c[:2], [to_np(out[0])[:k], to_np(out[1])[:k]]) and same([ref_c[2]], [to_np(out[2])], upto=len(ref_c[2])),
                  "ids + segment ids out")
    r2d = RaggedToDense(pad_right=True, lib=lib)
    T = max_len + 2
    ref_d = O.ragged_to_dense(ref_c[0], ref_c[1], ref_c[2], T, 50256, True)
    timed("RaggedToDense(pad right)", lambda: r2d.evaluate([c_out[0], c_out[1], c_out[2], np.array([T], np.int32), np.array([50256], np.int32)]),
          4 * (kept + 2 * n) + 5 * n * T + 8 * n, lambda out: same([ref_d[0]], [to_np(out[0])[:k]]), f"T = {T}: input_ids i32 + mask u8")
    tail = FusedEncodeTail(max_length=max_len, lib=lib)
    timed("ovtk_encode_tail_run (Truncate -> CombineSegments -> RaggedToDense x 2)",
          lambda: tail.evaluate([bos_d, (ib, ie, ids), bos_d], seg_ids, truncated=(1,), pad_value=50256, target_dim=T),
          4 * kept + 9 * n * T + 8 * n, lambda out: same([ref_d[0]], [to_np(out[0])[:k]]),
          "one call, one kernel behind the width measurement; input_ids + attention_mask + token_type_ids")
    tf_ops()
    print(json.dumps({"batch": {"rows": n, "text_bytes": n_c, "ids": n_t, "ids_kept_by_truncate": kept}}))


if __name__ == "__main__":
    main()
