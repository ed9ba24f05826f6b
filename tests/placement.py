"""Guarded arenas: the buffers an op sees carved out of ONE allocation, at chosen addresses modulo 16, between guard bands.

A caller of the C ABI hands it views (`t[1:]`) and regions of a pooled arena; the parity tests hand it torch / numpy allocations of
their own, which begin on a large power of two and have slack behind them.  `Arena` gives a test the first kind: every buffer
begins `shift` bytes (rounded down to what its element type needs) past a 16-byte boundary, is exactly as large as asked for, and
has GUARD bytes of a known `fill` in front and behind.  A kernel that reads one byte too far reads `fill` -- the tests run every
case under several fills, so a result that depends on it differs somewhere --, one that writes too far changes a guard byte, which
`check()` finds.  GUARD is two of the 2048-byte scan blocks: a stray access of that reach stays inside the allocation, so nothing
here can fault; bad reads and writes are found by value only.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from openvino_tokenizers_amd import _lib as L
from openvino_tokenizers_amd import ops

GUARD = 4096
_KINDS = {"i32": np.int32, "u8": np.uint8, "i64": np.int64, "bool": np.uint8}


def _dtype(kind):
    return np.dtype(_KINDS.get(kind, kind) if isinstance(kind, str) else kind)


class Arena:
    def __init__(self, backend, fill, size=6 << 20):
        self.backend, self.fill, self.size = backend, int(fill), int(size)
        self.device = backend.name == "hip-device"
        if self.device:
            import torch
            self.torch = torch
            self.mem = torch.full((self.size,), self.fill, dtype=torch.uint8, device="cuda")
            self.base = self.mem.data_ptr()
        else:
            self.mem = np.full(self.size, self.fill, np.uint8)
            self.base = self.mem.ctypes.data
        self.end = 0          # offset behind the last carved buffer
        self.bufs = []        # [name, offset, bytes, original bytes of a placed input or None]

    # -------------------------------------------------------------------------------------------- carving
    def carve(self, n_elems, kind, shift, min_align=None, name=None):
        """A typed view of n_elems elements whose address modulo 16 is shift - shift % max(element size, min_align or 1)."""
        dt = _dtype(kind)
        n_elems = int(n_elems)
        nbytes = n_elems * dt.itemsize
        mod = shift - shift % max(dt.itemsize, min_align or 1)
        off = self.end + GUARD
        off += (mod - (self.base + off)) % 16
        assert off + nbytes + GUARD <= self.size, f"arena of {self.size} bytes is too small for {name or kind}[{n_elems}]"
        assert (self.base + off) % 16 == mod and (self.base + off) % dt.itemsize == 0
        self.end = off + nbytes
        self.bufs.append([name or f"buffer {len(self.bufs)} ({dt.name}[{n_elems}])", off, nbytes, None])
        raw = self.mem[off:off + nbytes]
        if self.device:
            return raw.view(getattr(self.torch, dt.name))
        return raw.view(dt)

    def place(self, array, shift, min_align=None, name=None):
        """Carve a buffer for `array` (its dtype and shape; np.bool_ goes in as the bytes it is) and copy it in."""
        a = np.ascontiguousarray(array)
        if a.dtype == np.bool_:
            a = a.view(np.uint8)
        view = self.carve(a.size, a.dtype, shift, min_align, name or f"input {len(self.bufs)} ({a.dtype.name}{list(a.shape)})")
        self.bufs[-1][3] = a.tobytes()
        if self.device:
            if a.size:
                view.copy_(self.torch.from_numpy(a.reshape(-1).copy()))
            return view.reshape(a.shape)
        view[...] = a.reshape(-1)
        return view.reshape(a.shape)

    @staticmethod
    def pointer(view):
        return C.c_void_p(view.data_ptr() if hasattr(view, "data_ptr") else view.ctypes.data)

    # -------------------------------------------------------------------------------------------- outputs
    @contextlib.contextmanager
    def outputs(self, monkeypatch, shift, min_align=None):
        """While active, every output an op of ops.py allocates (ops._Mem.alloc) is carved from this arena: max(n, 1) elements and
        not one more, at `shift`; `min_align`: {kind: bytes} for the outputs that include/ovtk_amd.h gives an alignment rule.
        With the emulator build, device memory IS host memory: its calls go in as OVTK_MEM_DEVICE, so that the kernels get the carved
        addresses themselves and not the library's own staging copies of them."""
        arena, align = self, dict(min_align or {})
        emu = self.backend.name == "emu"
        init = ops._Mem.__init__

        def alloc(mem, n, kind):
            n = max(int(n), 1)
            view = arena.carve(n, kind, shift, align.get(kind), f"output {len(arena.bufs)} ({kind}[{n}])")
            return view, arena.pointer(view)

        def init_device(mem, sample):
            init(mem, sample)
            if not mem.torch:
                mem.mem = L.MEM_DEVICE

        with monkeypatch.context() as mp:
            mp.setattr(ops._Mem, "alloc", alloc)
            if emu:
                mp.setattr(ops._Mem, "__init__", init_device)
            yield self

    @property
    def mem_kind(self):
        """The `mem` argument of a direct C call on this arena's buffers."""
        return L.MEM_HOST if self.backend.name == "hip-host" else L.MEM_DEVICE

    @property
    def stream(self):
        if self.device:
            return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        return C.c_void_p(0)

    # -------------------------------------------------------------------------------------------- checking
    def check(self):
        """Every byte outside the carved buffers is still `fill`, every placed input still holds its bytes."""
        if self.device:
            self.torch.cuda.synchronize()
            host = self.mem.cpu().numpy()
        else:
            host = self.mem
        edges = [(None, 0, 0, None)] + [tuple(b) for b in self.bufs] + [(None, self.size, 0, None)]
        for (pname, poff, pbytes, _), (nname, noff, _, _) in zip(edges[:-1], edges[1:]):
            lo, hi = poff + pbytes, noff
            bad = np.flatnonzero(host[lo:hi] != self.fill)
            if len(bad):
                at = lo + int(bad[0])
                behind = nname is None or (pname is not None and at - lo < hi - at)
                who, rel = (pname, at - poff) if behind else (nname, at - noff)
                raise AssertionError(f"stray write: byte {rel:+d} relative to {who} (of {pbytes if behind else '?'} bytes) is "
                                     f"0x{int(host[at]):02X}, the guard fill is 0x{self.fill:02X}; {len(bad)} guard bytes between "
                                     f"{pname} and {nname} changed")
        for name, off, nbytes, orig in self.bufs:
            if orig is None:
                continue
            now = host[off:off + nbytes]
            bad = np.flatnonzero(now != np.frombuffer(orig, np.uint8))
            if len(bad):
                at = int(bad[0])
                raise AssertionError(f"input overwritten: byte +{at} of {name} is 0x{int(now[at]):02X}, was 0x{orig[at]:02X}")
