"""Sentence pairs in one call: ops.FusedPairEncodeDense and ops.FusedPairWordpieceDense (re-exported by ops.py, which this module
is imported from -- import them from there or from the package).

The mirror of the reference's add_second_input (python/openvino_tokenizers/tokenizer_transformations.py:22-304) behind
ovtk_encode_pair_dense_enqueue / ovtk_wordpiece_encode_pair_dense_enqueue / ovtk_encode_pair_dense_finish.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .ops import _host, _Mem, _ragged_in

TRUNC_MODES = {"only_first": 0, "only_second": 1, "longest_first": 2}


class _FusedPairDense:
    """The paired graph in one call (the reference's add_second_input, tokenizer_transformations.py:22-304): the encode on the
    n first rows followed by the n second ones -> Truncate with two inputs (src/truncate.cpp:69-144) -> CombineSegments (front |
    first | between | second | behind, with their type ids) -> RaggedToDense x 3.  Returns [input_ids, attention_mask (bool),
    token_type_ids], each [n, T], written by the encode's last pass.  Device tensors (torch CUDA; host arrays with the emulator
    build).  trunc_mode: a name of TRUNC_MODES or its number."""

    def __init__(self, max_length=2**31 - 1, trunc_side="right", trunc_mode="longest_first", pad_right=True, pad_value=0, type_pad_value=0,
                 front=(), between=(), behind=(), type_ids=(0, 0, 0, 1, 1)):
        self.max_length, self.trunc_left, self.pad_right = int(max_length), trunc_side == "left", bool(pad_right)
        self.trunc_mode = TRUNC_MODES[trunc_mode] if isinstance(trunc_mode, str) else int(trunc_mode)
        self.pad_value, self.type_pad_value = int(pad_value), int(type_pad_value)
        self.front, self.between, self.behind = (np.asarray(list(x), np.int32) for x in (front, between, behind))
        self.type_ids = [int(t) for t in type_ids]
        if len(self.type_ids) != 5:
            raise L.OvtkError(L.E_ARG, "a pair has five segments: front, first, between, second, behind")

    def _launch(self, lib, rs, pskips, n_first, p, outs, cap, st, pending):   # the op's enqueue entry point
        raise NotImplementedError

    def _enqueue(self, lib, ragged_inputs, n_first, target_dim, row_capacity, stream, mask, type_ids):
        m = _Mem(ragged_inputs[4])
        if not m.torch and not hasattr(lib, "ovtk_emulator_build"):   # the emulator build's device memory IS host memory (tests)
            raise L.OvtkError(L.E_ARG, f"{type(self).__name__} needs device-resident (torch CUDA) inputs")
        rs, (rb, _, _, _, c) = _ragged_in(m, ragged_inputs)
        _, pskips = (m.inp(ragged_inputs[5], "bool") if len(ragged_inputs) == 6 else (None, None))
        rows = int(n_first)
        extra = len(self.front) + len(self.between) + len(self.behind)
        if row_capacity is None:
            row_capacity = (int(target_dim) if target_dim is not None else min(self.max_length, max(len(c), 1)) + extra)
        cap = max(rows * int(row_capacity), 1)
        ids, pids = m.alloc(cap, "i32")
        msk, pmask = m.alloc(cap, "bool") if mask else (None, None)
        typ, ptypes = m.alloc(cap, "i32") if type_ids else (None, None)
        p = L.PairDenseParams(C.c_int32(min(self.max_length, 2**31 - 1)), int(self.trunc_left), self.trunc_mode, int(self.pad_right),
                              self.pad_value, self.type_pad_value, -1 if target_dim is None else int(target_dim),
                              self.front.ctypes.data_as(C.c_void_p), len(self.front), self.between.ctypes.data_as(C.c_void_p), len(self.between),
                              self.behind.ctypes.data_as(C.c_void_p), len(self.behind), (C.c_int32 * 5)(*self.type_ids))
        pending = C.c_void_p()
        st = C.c_void_p(stream) if isinstance(stream, int) else (stream if stream is not None else m.stream)
        L.check(lib, self._launch(lib, rs, pskips, C.c_int64(rows), p, (pids, pmask, ptypes), C.c_int64(cap), st, pending))

        def ticket(_keep=(m, p)):
            width, n_ids = C.c_int32(0), C.c_int64(0)
            rc = lib.ovtk_encode_pair_dense_finish(pending, C.byref(width), C.byref(n_ids))
            if rc != L.OVTK_OK:
                err = L.OvtkError(rc, lib.ovtk_last_error().decode(errors="replace"))
                err.width = int(width.value)   # (OVTK_E_CAPACITY: the row width the outputs need)
                raise err
            self.n_ids = int(n_ids.value)   # (the last completed call's ids before truncation, all rows)
            n = rows * int(width.value)
            shape = (rows, int(width.value))
            out = [ids[:n].reshape(shape), None if msk is None else msk[:n].reshape(shape), None if typ is None else typ[:n].reshape(shape)]
            if out[1] is not None:
                out[1] = out[1].bool() if m.torch else out[1].astype(bool)
            return out
        return ticket

    def evaluate(self, *args, **kw):
        return self.enqueue(*args, **kw)()


class FusedPairEncodeDense(_FusedPairDense):
    """[SpecialTokensSplit ->] RegexSplit -> BPETokenizer on sentence pairs -> the paired tail, in one call
    (ovtk_encode_pair_dense_enqueue / ovtk_encode_pair_dense_finish)."""

    def __init__(self, split, bpe, special=None, **tail):
        super().__init__(**tail)
        self.split, self.bpe, self.special = split, bpe, special

    def enqueue(self, ragged_inputs, n_first, split_pattern, bpe_constant_inputs, special_pattern=None, target_dim=None, row_capacity=None,
                stream=None, mask=True, type_ids=True):
        """ragged_inputs: ragged_begins, ragged_ends, begins, ends, chars [, skips] of the n_first first rows followed by the second
        ones.  row_capacity: cells per row the outputs are allocated with."""
        if self.special is not None:
            self.special._ensure(special_pattern)
        self.split._ensure(split_pattern)
        self.bpe._ensure(list(ragged_inputs[:5]) + list(bpe_constant_inputs))
        return self._enqueue(self.bpe._lib, ragged_inputs, n_first, target_dim, row_capacity, stream, mask, type_ids)

    def _launch(self, lib, rs, pskips, n_first, p, outs, cap, st, pending):
        return lib.ovtk_encode_pair_dense_enqueue(self.special._h if self.special is not None else None, self.split._h, self.bpe._h, C.byref(rs),
                                                  pskips, n_first, C.byref(p), outs[0], outs[1], outs[2], cap, st, C.byref(pending))


class FusedPairWordpieceDense(_FusedPairDense):
    """RegexSplit(\\s+, remove) -> RegexSplit(BERT delimiters, isolate) -> WordpieceTokenizer on sentence pairs -> the paired tail, in
    one call (ovtk_wordpiece_encode_pair_dense_enqueue / ovtk_encode_pair_dense_finish)."""

    def __init__(self, whitespace, delimiters, wordpiece, **tail):
        super().__init__(**tail)
        self.whitespace, self.delimiters, self.wordpiece = whitespace, delimiters, wordpiece

    def enqueue(self, ragged_inputs, n_first, whitespace_pattern, delimiters_pattern, wordpiece_constant_inputs, target_dim=None,
                row_capacity=None, stream=None, mask=True, type_ids=True):
        """ragged_inputs: inputs 0-4 of the first RegexSplit, the n_first first rows followed by the second ones;
        wordpiece_constant_inputs: inputs 5-8 of WordpieceTokenizer."""
        self.whitespace._ensure(whitespace_pattern)
        self.delimiters._ensure(delimiters_pattern)
        self.wordpiece._ensure(list(ragged_inputs[:5]) + list(wordpiece_constant_inputs))
        self._unk = int(np.asarray(_host(wordpiece_constant_inputs[3], np.int32)).reshape(-1)[0])
        return self._enqueue(self.wordpiece._lib, ragged_inputs, n_first, target_dim, row_capacity, stream, mask, type_ids)

    def _launch(self, lib, rs, pskips, n_first, p, outs, cap, st, pending):
        return lib.ovtk_wordpiece_encode_pair_dense_enqueue(self.wordpiece._h, self.whitespace._h, self.delimiters._h, C.byref(rs),
                                                            C.c_int32(self._unk), n_first, C.byref(p), outs[0], outs[1], outs[2], cap, st,
                                                            C.byref(pending))
