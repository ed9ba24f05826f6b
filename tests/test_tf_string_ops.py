"""StringToHashBucket (src/string_to_hash_bucket.cpp:10-220), EqualStr (src/equal_str.cpp:29-61) and RaggedToRagged
(src/ragged_to_ragged.cpp:43-98): the ops of the reference's TensorFlow front end, on every backend, against a plain-Python restatement
of the three evaluate() bodies written from the algorithm (Python ints masked to 64 bits for the hash, the sequential loop for the row
ids).  Every comparison is of whole arrays.

The restatement of the hash is pinned by two known answers that do not depend on it, and these are the ONLY independent pins:
TensorFlow's documented tf.strings.to_hash_bucket_fast(["Hello", "TensorFlow", "2.x"], 3) == [0, 2, 2], and FarmHash's
Fingerprint64("") == k2 == 0x9ae16a3b2f90404f.  Both are asserted on the restatement and on the library."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

from openvino_tokenizers_amd import _lib as L

M64 = (1 << 64) - 1
K0, K1, K2 = 0xc3a5c85c97cb3127, 0xb492b66fbe98f273, 0x9ae16a3b2f90404f


# ---------------------------------------------------------------------------------------------- the restatement
def _rot(v, s):
    return ((v >> s) | (v << (64 - s))) & M64


def _mix(v):
    return v ^ (v >> 47)


def _f64(s, at):
    return int.from_bytes(s[at:at + 8], "little")


def _f32(s, at):
    return int.from_bytes(s[at:at + 4], "little")


def _len16(u, v, mul):
    a = ((u ^ v) * mul) & M64
    a ^= a >> 47
    b = ((v ^ a) * mul) & M64
    b ^= b >> 47
    return (b * mul) & M64


def _weak(s, at, a, b):
    w, x, y, z = _f64(s, at), _f64(s, at + 8), _f64(s, at + 16), _f64(s, at + 24)
    a = (a + w) & M64
    b = _rot((b + a + z) & M64, 21)
    c = a
    a = (a + x + y) & M64
    b = (b + _rot(a, 44)) & M64
    return (a + z) & M64, (b + c) & M64


def fingerprint64(s):
    s = bytes(s)
    n = len(s)
    if n <= 16:
        mul = (K2 + 2 * n) & M64
        if n >= 8:
            a, b = (_f64(s, 0) + K2) & M64, _f64(s, n - 8)
            return _len16((_rot(b, 37) * mul + a) & M64, ((_rot(a, 25) + b) * mul) & M64, mul)
        if n >= 4:
            return _len16((n + (_f32(s, 0) << 3)) & M64, _f32(s, n - 4), mul)
        if n > 0:
            y = (s[0] + (s[n >> 1] << 8)) & 0xFFFFFFFF
            z = (n + (s[n - 1] << 2)) & 0xFFFFFFFF
            return (_mix(((y * K2) & M64) ^ ((z * K0) & M64)) * K2) & M64
        return K2
    mul = (K2 + 2 * n) & M64
    if n <= 32:
        a, b, c, d = (_f64(s, 0) * K1) & M64, _f64(s, 8), (_f64(s, n - 8) * mul) & M64, (_f64(s, n - 16) * K2) & M64
        return _len16((_rot((a + b) & M64, 43) + _rot(c, 30) + d) & M64, (a + _rot((b + K2) & M64, 18) + c) & M64, mul)
    if n <= 64:
        a, b, c, d = (_f64(s, 0) * K2) & M64, _f64(s, 8), (_f64(s, n - 8) * mul) & M64, (_f64(s, n - 16) * K2) & M64
        y = (_rot((a + b) & M64, 43) + _rot(c, 30) + d) & M64
        z = _len16(y, (a + _rot((b + K2) & M64, 18) + c) & M64, mul)
        e, f = (_f64(s, 16) * mul) & M64, _f64(s, 24)
        g, h = ((y + _f64(s, n - 32)) * mul) & M64, ((z + _f64(s, n - 24)) * mul) & M64
        return _len16((_rot((e + f) & M64, 43) + _rot(g, 30) + h) & M64, (e + _rot((f + a) & M64, 18) + g) & M64, mul)
    x = 81
    y = (81 * K1 + 113) & M64
    z = (_mix((y * K2 + 113) & M64) * K2) & M64
    v, w = (0, 0), (0, 0)
    x = (x * K2 + _f64(s, 0)) & M64

    def one_round(at, mul, times):
        nonlocal x, y, z, v, w
        x = (_rot((x + y + v[0] + _f64(s, at + 8)) & M64, 37) * mul) & M64
        y = (_rot((y + v[1] + _f64(s, at + 48)) & M64, 42) * mul) & M64
        x ^= (w[1] * times) & M64
        y = (y + v[0] * times + _f64(s, at + 40)) & M64
        z = (_rot((z + w[0]) & M64, 33) * mul) & M64
        v = _weak(s, at, (v[1] * mul) & M64, (x + w[0]) & M64)
        w = _weak(s, at + 32, (z + w[1]) & M64, (y + _f64(s, at + 16)) & M64)
        x, z = z, x
    for blk in range((n - 1) // 64):
        one_round(64 * blk, K1, 1)
    mul = (K1 + ((z & 0xFF) << 1)) & M64
    w = ((w[0] + ((n - 1) & 63)) & M64, w[1])
    v = ((v[0] + w[0]) & M64, v[1])
    w = ((w[0] + v[0]) & M64, w[1])
    one_round(n - 64, mul, 9)
    return _len16((_len16(v[0], w[0], mul) + ((_mix(y) * K0) & M64) + z) & M64, (_len16(v[1], w[1], mul) + x) & M64, mul)


def equal_ref(a, b):
    """equal_str.cpp:42-57 over two lists of bytes."""
    n = 0 if not a or not b else max(len(a), len(b))
    return np.array([a[i if i < len(a) else 0] == b[i if i < len(b) else 0] for i in range(n)], np.int32).reshape(n)


def ragged_ref(rowids, batch):
    """ragged_to_ragged.cpp:56-95, the sequential loop; -> begins, ends, the rows it writes."""
    begins, ends, written = np.zeros(batch, np.int32), np.zeros(batch, np.int32), np.zeros(batch, bool)

    def put(r, b, e):
        begins[r], ends[r], written[r] = b, e, True
    n = len(rowids)
    prev_idx, prev_row = 0, -1
    for i in range(n):
        cur = int(rowids[i])
        assert cur >= 0
        if cur >= batch:
            break
        if prev_row != cur:
            if prev_row != -1:
                put(prev_row, prev_idx, i)
            for r in range(prev_row + 1, cur):
                put(r, i, i)
            prev_idx, prev_row = i, cur
        if i + 1 == n:
            put(cur, prev_idx, n)
            prev_row, prev_idx = cur, n
    for r in range(0 if prev_row < 0 else prev_row + 1, batch):
        put(r, prev_idx, prev_idx)
    return begins, ends, written


# ---------------------------------------------------------------------------------------------- helpers
def pack(strings, lead=0):
    """Back-to-back strings behind `lead` bytes that belong to no string."""
    lens = np.array([len(s) for s in strings], np.int64)
    ends = (np.cumsum(lens) + lead).astype(np.int32)
    begins = (ends - lens).astype(np.int32)
    chars = np.frombuffer(b"\xa5" * lead + b"".join(strings), np.uint8).copy()
    return begins.reshape(len(strings)), ends.reshape(len(strings)), chars


def strings_of(b, e, c):
    raw = c.tobytes()
    return [raw[int(x):int(y)] for x, y in zip(b.reshape(-1), e.reshape(-1))]


def run(backend, op, arrays, **kw):
    """evaluate() on the backend's data; on hip-device the outputs must be CUDA tensors on the inputs' device."""
    data = backend.data(arrays)
    outs = op.evaluate(data, **kw)
    if backend.name == "hip-device":
        for o in outs:
            assert hasattr(o, "data_ptr") and o.device == data[0].device, "outputs belong on the inputs' device"
    else:
        assert all(isinstance(o, np.ndarray) for o in outs)
    return [backend.host(o) for o in outs]


def hash_op(backend, nb):
    from openvino_tokenizers_amd.ops import StringToHashBucket
    return StringToHashBucket(nb, lib=backend.lib)


def check_hash(backend, b, e, c, raw, nb=(1 << 63) - 1):
    (got,) = run(backend, hash_op(backend, nb), [b, e, c])
    want = np.array([h % nb for h in raw], np.int64).reshape(b.shape)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), f"first difference at {np.flatnonzero(got.reshape(-1) != want.reshape(-1))[:5]}"


@lru_cache(maxsize=None)
def every_length_batch():
    """Every length 0..200 at every begin offset mod 8: begins scattered over a buffer of random bytes (gaps, overlaps, no order), 16+
    junk bytes in front of the first begin, the last string flush with the end of chars."""
    rng = np.random.default_rng(11)
    size = 3001
    chars = rng.integers(0, 256, size, dtype=np.uint8)
    begins, ends = [], []
    for ln in range(201):
        for off in range(8):
            at = 8 * int(rng.integers(2, (size - ln - off) // 8)) + off
            begins.append(at)
            ends.append(at + ln)
    begins.append(size - 77)
    ends.append(size)
    order = rng.permutation(len(begins))
    b, e = np.array(begins, np.int32)[order], np.array(ends, np.int32)[order]
    assert b.min() >= 16 and e.max() == size and all(((b % 8 == o) & (e - b == 65)).any() for o in range(8))
    return b, e, chars, tuple(fingerprint64(s) for s in strings_of(b, e, chars))


@lru_cache(maxsize=None)
def short_batch():
    rng = np.random.default_rng(5)
    strings = [rng.integers(0, 256, int(ln), dtype=np.uint8).tobytes() for ln in rng.integers(0, 41, 4097)]
    return strings, tuple(fingerprint64(s) for s in strings)


# ---------------------------------------------------------------------------------------------- StringToHashBucket
def test_restatement_known_answers():
    assert fingerprint64(b"") == 0x9ae16a3b2f90404f
    assert [fingerprint64(s) % 3 for s in (b"Hello", b"TensorFlow", b"2.x")] == [0, 2, 2]


def test_hash_known_answers(backend):
    b, e, c = pack([b"Hello", b"TensorFlow", b"2.x"])
    (got,) = run(backend, hash_op(backend, 3), [b, e, c])
    assert got.tolist() == [0, 2, 2]
    # Fingerprint64("") == k2, seen through two moduli (a mask and a division)
    z = np.zeros(1, np.int32)
    for nb in (1 << 62, (1 << 63) - 1):
        (got,) = run(backend, hash_op(backend, nb), [z, z, np.zeros(4, np.uint8)])
        assert got.tolist() == [0x9ae16a3b2f90404f % nb]


def test_hash_every_length_and_alignment(backend):
    b, e, c, raw = every_length_batch()
    check_hash(backend, b, e, c, raw)


def test_hash_high_bytes_are_unsigned(backend):
    strings = [bytes([v]) * ln for v in (0xFF, 0x80) for ln in (1, 2, 3, 65)] + [b"\x80\xff\x80", b"\xff\x80"]
    b, e, c = pack(strings, lead=3)
    check_hash(backend, b, e, c, [fingerprint64(s) for s in strings])
    check_hash(backend, b, e, c, [fingerprint64(s) for s in strings], nb=1000)


def test_hash_long_strings_among_short_ones(backend):
    rng = np.random.default_rng(17)
    strings = [rng.integers(0, 256, int(ln), dtype=np.uint8).tobytes() for ln in rng.integers(0, 30, 70)]
    strings[5] = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()
    strings[40] = rng.integers(0, 256, 100001, dtype=np.uint8).tobytes()
    b, e, c = pack(strings, lead=1)
    check_hash(backend, b, e, c, [fingerprint64(s) for s in strings])


@pytest.mark.parametrize("nb", [1, 3, 1000, 1 << 31, (1 << 32) + 7, (1 << 63) - 1])
def test_hash_num_buckets(backend, nb):
    b, e, c, raw = every_length_batch()
    check_hash(backend, b[:300], e[:300], c, raw[:300], nb)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_hash_counts(backend, n):
    strings, raw = short_batch()
    b, e, c = pack(strings[:n], lead=2)
    check_hash(backend, b, e, c, raw[:n], nb=(1 << 32) + 7)


def test_hash_keeps_the_shape(backend):
    strings, raw = short_batch()
    b, e, c = pack(strings[:6])
    check_hash(backend, b.reshape(2, 3), e.reshape(2, 3), c, raw[:6], nb=1000)


def test_hash_error_codes(backend):
    strings, _ = short_batch()
    b, e, c = pack(strings[:101])
    for nb in (0, -1):
        with pytest.raises(L.OvtkError) as err:
            run(backend, hash_op(backend, nb), [b, e, c])
        assert err.value.code == L.E_ARG
    b = b.copy()
    b[57] = e[57] + 1
    with pytest.raises(L.OvtkError) as err:
        run(backend, hash_op(backend, 1000), [b, e, c])
    assert err.value.code == L.E_RANGE


# ---------------------------------------------------------------------------------------------- EqualStr
def equal_op(backend):
    from openvino_tokenizers_amd.ops import EqualStr
    return EqualStr(lib=backend.lib)


def check_equal(backend, a, b, lead_a=0, lead_b=5):
    (got,) = run(backend, equal_op(backend), list(pack(a, lead_a)) + list(pack(b, lead_b)))
    want = equal_ref(a, b)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), f"first difference at {np.flatnonzero(got != want)[:5]}"
    return got


def pairs(n):
    """n pairs over the kinds that matter; pair 0 (n > 1: pair 1) is 1 000 bytes long and differs at byte 999 only."""
    rng = np.random.default_rng(n)
    a, b = [], []
    for i in range(n):
        s = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
        kind = i % 7
        if kind == 0:
            t = s                                             # identical
        elif kind == 1:
            t = bytes([s[0] ^ 1]) + s[1:]                     # the first byte differs
        elif kind == 2:
            t = s[:-1] + bytes([s[-1] ^ 0x80])                # the last byte differs
        elif kind == 3:
            t = s + b"x"                                      # a is a proper prefix of b
        elif kind == 4:
            s, t = b"", b""                                   # empty against empty
        elif kind == 5:
            t = b""                                           # non-empty against empty
        else:
            s, t = s + b"tail", s                             # b is a proper prefix of a
        a.append(s)
        b.append(t)
    big = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
    a[min(1, n - 1)], b[min(1, n - 1)] = big, big[:999] + bytes([big[999] ^ 4])
    return a, b


@pytest.mark.parametrize("n", [1, 65, 4097])
def test_equal_pairwise(backend, n):
    a, b = pairs(n)
    got = check_equal(backend, a, b)
    if n > 1:
        assert got[0] == 1 and got[1] == 0 and got.sum() > n // 8


def test_equal_long_identical_pair(backend):
    rng = np.random.default_rng(2)
    big = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
    assert check_equal(backend, [big, big[:999]], [big, big]).tolist() == [1, 0]


def test_equal_broadcasts(backend):
    a, _ = pairs(130)
    const = a[7]
    a[64], a[129] = const, const
    got = check_equal(backend, a, [const], lead_b=9)        # n2 == 1, the constant in a buffer of its own at a non-zero begin
    assert got[7] == 1 and got[64] == 1 and got[129] == 1
    got = check_equal(backend, [const], a, lead_a=9, lead_b=0)   # n1 == 1
    assert got.sum() >= 3


@pytest.mark.parametrize("n1,n2", [(3, 2), (2, 5)])
def test_equal_quirk_sizes(backend, n1, n2):
    words = [b"aa", b"bb", b"aa", b"cc", b"aa"]
    got = check_equal(backend, words[:n1], words[:n2])
    assert len(got) == max(n1, n2)
    # (3, 2): element 2 is a[2] against b[0]; (2, 5): elements 2.. are a[0] against b[i]
    assert got.tolist() == ([1, 1, 1] if n1 == 3 else [1, 1, 1, 0, 1])


@pytest.mark.parametrize("n1,n2", [(0, 4), (4, 0), (0, 0)])
def test_equal_empty_side(backend, n1, n2):
    words = [b"aa", b"bb", b"aa", b"cc"]
    got = check_equal(backend, words[:n1], words[:n2])
    assert got.shape == (0,)


def test_equal_same_tensors(backend):
    a, _ = pairs(65)
    data = backend.data(list(pack(a, 3)))
    (got,) = equal_op(backend).evaluate(data + data)
    assert backend.host(got).tolist() == [1] * 65


def test_equal_capacity(backend):
    from openvino_tokenizers_amd.ops import _Mem
    a, b = pairs(65)
    data = backend.data(list(pack(a)) + list(pack(b, 5)))
    with pytest.raises(L.OvtkError) as err:
        equal_op(backend).evaluate(data, capacity=64)
    assert err.value.code == L.E_CAPACITY
    m = _Mem(data[2])
    ptr = [m.inp(x, "u8" if i % 3 == 2 else "i32") for i, x in enumerate(data)]
    sa = L.Strings(ptr[0][1], ptr[1][1], ptr[2][1], 65, len(ptr[2][0]))
    sb = L.Strings(ptr[3][1], ptr[4][1], ptr[5][1], 65, len(ptr[5][0]))
    out, pout = m.alloc(64, "i32")
    n = C.c_int64(-1)
    rc = backend.lib.ovtk_equal_str(C.byref(sa), C.byref(sb), pout, C.c_int64(64), C.byref(n), m.mem, 0, m.stream)
    assert rc == L.E_CAPACITY and n.value == 65


# ---------------------------------------------------------------------------------------------- RaggedToRagged
def ragged_op(backend):
    from openvino_tokenizers_amd.ops import RaggedToRagged
    return RaggedToRagged(lib=backend.lib)


def run_ragged(backend, rowids, batch):
    ob, oe = run(backend, ragged_op(backend), [np.array(rowids, np.int32).reshape(-1), np.array([batch], np.int32)])
    assert ob.dtype == np.int32 and oe.dtype == np.int32 and ob.shape == (batch,) and oe.shape == (batch,)
    return ob, oe


def check_ragged(backend, rowids, batch):
    ob, oe = run_ragged(backend, rowids, batch)
    wb, we, written = ragged_ref(rowids, batch)
    assert np.array_equal(ob[written], wb[written]) and np.array_equal(oe[written], we[written]), (ob.tolist()[:20], oe.tolist()[:20])
    return ob, oe, written


@pytest.mark.parametrize("batch", [0, 1, 5])
def test_ragged_empty_ids(backend, batch):
    ob, oe, written = check_ragged(backend, [], batch)
    assert written.all() and not ob.any() and not oe.any()


@pytest.mark.parametrize("rowids,batch,want", [
    ([2, 2, 3], 5, ([0, 0, 0, 2, 3], [0, 0, 2, 3, 3])),                       # leading empty rows
    ([0, 0, 3, 3, 3, 6], 7, ([0, 2, 2, 2, 5, 5, 5], [2, 2, 2, 5, 5, 5, 6])),  # gaps in the middle
    ([0, 1, 1], 6, ([0, 1, 3, 3, 3, 3], [1, 3, 3, 3, 3, 3])),                 # trailing empty rows
    ([2, 2, 2, 2], 3, ([0, 0, 0], [0, 0, 4])),                                # a single run
    ([0, 1, 2, 3], 4, ([0, 1, 2, 3], [1, 2, 3, 4])),                          # every row one element
    ([1], 3, ([0, 0, 1], [0, 1, 1])),                                         # n = 1
])
def test_ragged_hand_cases(backend, rowids, batch, want):
    ob, oe, written = check_ragged(backend, rowids, batch)
    assert written.all() and (ob.tolist(), oe.tolist()) == want


def test_ragged_random_sorted(backend):
    rng = np.random.default_rng(9)
    present = np.flatnonzero(rng.random(300) > 1 / 3)
    rowids = np.sort(rng.choice(present, 4097)).astype(np.int32)
    ob, oe, written = check_ragged(backend, rowids, 300)
    assert written.all() and 80 < int((ob == oe).sum()) < 130


def test_ragged_gap_longer_than_a_block(backend):
    ob, oe, written = check_ragged(backend, [0, 4999], 5000)
    assert written.all() and ob[1:4999].tolist() == [1] * 4998 and oe[4999] == 2


def test_ragged_long_stretches(backend):
    """Stretches beyond the length a wave fills itself (leading, middle, trailing) go through the list."""
    ob, oe, written = check_ragged(backend, [4500, 4500, 9500], 15000)
    assert written.all() and not ob[:4500].any() and ob[4501:9500].tolist() == [2] * 4999 and oe[9501:].tolist() == [3] * 5499


def test_ragged_out_of_range_tail(backend):
    ob, oe, written = check_ragged(backend, [0, 0, 1, 1, 1, 7, 9], 4)
    assert written.tolist() == [True, False, True, True]           # the reference leaves row 1 unwritten ...
    assert (ob.tolist(), oe.tolist()) == ([0, 2, 2, 2], [2, 5, 2, 2])   # ... here it is [s, j) = [2, 5); rows 2 and 3 are [s, s)
    ob, oe, written = check_ragged(backend, [5, 6], 4)                # the very first id is out of range
    assert written.all() and not ob.any() and not oe.any()
    ob, oe, _ = check_ragged(backend, [3, 3, 9000], 5000)                # the [s, s) rows as one long stretch
    assert (ob[3], oe[3]) == (0, 2) and ob[4:].tolist() == [0] * 4996 and oe[4:].tolist() == [0] * 4996


def test_ragged_error_codes(backend):
    for rowids, code in (([-1, 0, 1], L.E_RANGE), ([0, 2, 1], L.E_ARG)):
        with pytest.raises(L.OvtkError) as err:
            run_ragged(backend, rowids, 4)
        assert err.value.code == code
    with pytest.raises(L.OvtkError) as err:
        run_ragged(backend, [0], -1)
    assert err.value.code == L.E_ARG


# ---------------------------------------------------------------------------------------------- across backends
def test_host_and_device_give_identical_bytes(gpu_backend):
    import torch
    from openvino_tokenizers_amd.ops import EqualStr, RaggedToRagged, StringToHashBucket
    lib = gpu_backend.lib
    b, e, c, _ = every_length_batch()
    a1, a2 = pairs(4097)
    rng = np.random.default_rng(9)
    rowids = np.sort(rng.integers(0, 300, 4097)).astype(np.int32)
    cases = [(StringToHashBucket((1 << 32) + 7, lib=lib), [b, e, c]),
             (EqualStr(lib=lib), list(pack(a1)) + list(pack(a2, 5))),
             (RaggedToRagged(lib=lib), [rowids, np.array([300], np.int32)])]
    for op, arrays in cases:
        host = op.evaluate(list(arrays))
        dev = op.evaluate([torch.as_tensor(x, device="cuda") for x in arrays])
        assert len(host) == len(dev)
        for h, d in zip(host, dev):
            assert isinstance(h, np.ndarray) and d.is_cuda
            assert h.dtype == d.cpu().numpy().dtype and h.tobytes() == d.cpu().numpy().tobytes()
