"""NumericToString (src/numeric_to_string.cpp:18-92) on every backend against tests/golden/golden_numeric_to_string.npz: the texts a
C++ restatement of the op (std::to_string, std::ostringstream) gave for the recorded inputs, which the generator
(tests/gen_golden_numeric_to_string.py) also checked against Python's '%g' and str.  The float inputs hold the hard cases of %g with
precision 6: exact ties of the sixth digit, their neighbours one ulp away, every power of ten with its neighbours, denormals, the
999999.5 -> 1e+06 edge.  Every comparison is of whole begins, ends and chars arrays."""
import ctypes as C
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from openvino_tokenizers_amd import _lib as L

GOLDEN = Path(__file__).resolve().parent / "golden" / "golden_numeric_to_string.npz"
DTYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64", "bool"]
CODES = {"int8": L.NUM_I8, "int16": L.NUM_I16, "int32": L.NUM_I32, "int64": L.NUM_I64, "uint8": L.NUM_U8, "uint16": L.NUM_U16,
         "uint32": L.NUM_U32, "uint64": L.NUM_U64, "float32": L.NUM_F32, "float64": L.NUM_F64, "bool": L.NUM_BOOL}


@lru_cache(maxsize=None)
def golden(name):
    """-> (input array in its own dtype, the texts as a list of bytes); read once, never changed."""
    with np.load(GOLDEN) as z:
        arr, ends, chars = z[f"in_{name}"], z[f"ends_{name}"], z[f"chars_{name}"].tobytes()
    arr = arr.view({"float32": np.float32, "float64": np.float64, "bool": np.bool_}.get(name, arr.dtype))
    begins = np.concatenate([[0], ends[:-1]])
    texts = [chars[b:e] for b, e in zip(begins.tolist(), ends.tolist())]
    arr.setflags(write=False)
    return arr, texts


def expected(texts, shape=None):
    lens = np.array([len(t) for t in texts], np.int64)
    ends = np.cumsum(lens).astype(np.int32)
    begins = (ends - lens).astype(np.int32)
    shape = (len(texts),) if shape is None else shape
    return begins.reshape(shape), ends.reshape(shape), np.frombuffer(b"".join(texts), np.uint8)


def op_of(backend):
    from openvino_tokenizers_amd.ops import NumericToString
    return NumericToString(lib=backend.lib)


def run(backend, arr, **kw):
    op = op_of(backend)
    out = op.evaluate(backend.data([np.array(arr)]), **kw)
    return [backend.host(x) for x in out]


def check(backend, arr, texts):
    b, e, c = run(backend, arr)
    wb, we, wc = expected(texts, np.shape(arr))
    assert b.dtype == np.int32 and e.dtype == np.int32 and c.dtype == np.uint8
    assert b.shape == wb.shape and e.shape == we.shape
    if not (np.array_equal(b, wb) and np.array_equal(e, we) and np.array_equal(c, wc)):
        flat_b, flat_e, raw = b.reshape(-1), e.reshape(-1), c.tobytes()
        got = [raw[x:y] for x, y in zip(flat_b.tolist(), flat_e.tolist())]
        bad = [(i, np.asarray(arr).reshape(-1)[i], g, t) for i, (g, t) in enumerate(zip(got, texts)) if g != t][:8]
        raise AssertionError(f"{len(bad)}+ texts differ, the first (index, value, got, want): {bad}")


# ---------------------------------------------------------------------------------------------- the goldens
@pytest.mark.parametrize("name", DTYPES)
def test_matches_golden(backend, name):
    arr, texts = golden(name)
    check(backend, arr, texts)


def test_golden_holds_the_named_cases():
    """The file is the one the generator describes (a stale or hand-edited file would pass the parity tests on less)."""
    arr, texts = golden("float64")
    by_value = {float(v): t for v, t in zip(arr.tolist(), texts) if np.isfinite(v)}
    want = {999999.5: b"1e+06", 999999.4999999999: b"999999", 9.9999995e-05: b"0.0001", 9.99999949e-05: b"0.0001", 1234565.0: b"1.23456e+06",
            1234575.0: b"1.23458e+06", 0.0001: b"0.0001", 0.00001: b"1e-05", 100000.0: b"100000", 1000000.0: b"1e+06", 5e-324: b"4.94066e-324",
            1.7976931348623157e308: b"1.79769e+308", 0.5: b"0.5", 100000.5: b"100000", 2.0 ** -10: b"0.000976562"}
    for v, t in want.items():
        assert by_value[v] == t, (v, by_value[v], t)
    raw = arr.view(np.uint64)
    at = {int(r): t for r, t in zip(raw.tolist(), texts)}
    assert at[0x8000000000000000] == b"-0" and at[0] == b"0" and at[0x7FF8000000000000] == b"nan" and at[0xFFF8000000000000] == b"-nan"
    assert at[0x7FF0000000000000] == b"inf" and at[0xFFF0000000000000] == b"-inf" and at[0x7FF0000000012345] == b"nan"
    ints, itexts = golden("int64")
    assert dict(zip(ints.tolist(), itexts))[-2 ** 63] == b"-9223372036854775808"
    u, utexts = golden("uint64")
    assert dict(zip(u.tolist(), utexts))[2 ** 64 - 1] == b"18446744073709551615"
    assert golden("bool")[1] == [b"false", b"true", b"true", b"true"]


# ---------------------------------------------------------------------------------------------- sizes and shapes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_counts(backend, n):
    """The wave and block edges of the scan and of the staged write; 4097 crosses a scan tile."""
    for name in ("float64", "int64"):
        arr, texts = golden(name)
        pick = np.random.default_rng(n).integers(0, arr.size, n)
        check(backend, arr[pick], [texts[i] for i in pick.tolist()])


def test_mixed_lengths_across_a_wave(backend):
    """The staged write at its most uneven: 1-byte and 20-byte (13-byte) texts in turn, over two waves and a bit."""
    ints = np.array([7 if i % 2 == 0 else -2 ** 63 for i in range(130)], np.int64)
    check(backend, ints, [b"7" if i % 2 == 0 else b"-9223372036854775808" for i in range(130)])
    floats = np.array([0.0 if i % 2 == 0 else -np.finfo(np.float64).max for i in range(130)], np.float64)
    check(backend, floats, [b"0" if i % 2 == 0 else b"-1.79769e+308" for i in range(130)])


@pytest.mark.parametrize("shape", [(3, 0, 5), (2, 3, 7)])
def test_keeps_the_shape(backend, shape):
    n = int(np.prod(shape))
    for name in ("float32", "uint16"):
        arr, texts = golden(name)
        check(backend, arr[:n].reshape(shape), texts[:n])


def test_exact_path_agrees(backend, monkeypatch):
    """OVTK_NUM2STR_EXACT=1 (read by every call) sends every finite element through the big-integer comparison: the same bytes."""
    for name in ("float32", "float64"):
        arr, texts = golden(name)
        monkeypatch.setenv("OVTK_NUM2STR_EXACT", "1")
        check(backend, arr, texts)
        monkeypatch.delenv("OVTK_NUM2STR_EXACT")
        check(backend, arr, texts)


# ---------------------------------------------------------------------------------------------- the C ABI's edges
def raw_call(backend, arr, dtype, n, cap, in_ptr="own", mem=None):
    """-> (rc, n_chars the call reports, begins, ends, chars); buffers pre-filled with 0x55 so that a write shows."""
    from openvino_tokenizers_amd.ops import _Mem
    data = backend.data([np.array(arr)])[0]
    m = _Mem(data)
    if m.torch:
        ptr = data.data_ptr()
    else:
        ptr = data.ctypes.data
    rows = max(min(int(n), np.asarray(arr).size), 1)   # (a refused n is refused before anything is touched)
    ob, pob = m.alloc(rows, "i32")
    oe, poe = m.alloc(rows, "i32")
    oc, poc = m.alloc(max(cap, 1), "u8")
    for x in (ob, oe, oc):
        x[...] = 0x55 if x.dtype == np.uint8 or "uint8" in str(x.dtype) else 0x55555555
    out = L.StringsOut(pob, poe, poc, cap, -7)
    rc = backend.lib.ovtk_numeric_to_string(C.c_void_p(ptr if in_ptr == "own" else in_ptr), dtype, C.c_int64(n), C.byref(out),
                                            m.mem if mem is None else mem, 0, m.stream)
    return rc, int(out.n_chars), backend.host(ob), backend.host(oe), backend.host(oc)


def test_capacity(backend):
    arr, texts = golden("int64")
    arr, texts = arr[:500], texts[:500]
    wb, we, wc = expected(texts)
    need = len(wc)
    rc, n_chars, b, e, c = raw_call(backend, arr, L.NUM_I64, arr.size, need - 1)
    assert rc == L.E_CAPACITY and n_chars == need
    assert (c == 0x55).all() and (b == 0x55555555).all() and (e == 0x55555555).all()   # nothing written
    rc, n_chars, b, e, c = raw_call(backend, arr, L.NUM_I64, arr.size, need)
    assert rc == L.OVTK_OK and n_chars == need and np.array_equal(b, wb) and np.array_equal(e, we) and np.array_equal(c[:need], wc)
    for name in DTYPES:
        garr, gtexts = golden(name)
        bound = backend.lib.ovtk_numeric_to_string_bound(CODES[name], garr.size)
        longest = max(len(t) for t in gtexts)
        assert bound % garr.size == 0 and longest <= bound // garr.size, (name, longest, bound)
        assert sum(len(t) for t in gtexts) <= bound
    assert backend.lib.ovtk_numeric_to_string_bound(11, 5) == -1 and backend.lib.ovtk_numeric_to_string_bound(-1, 5) == -1
    assert backend.lib.ovtk_numeric_to_string_bound(L.NUM_F64, -1) == -1
    assert backend.lib.ovtk_numeric_to_string_bound(L.NUM_F64, 3) == 39 and backend.lib.ovtk_numeric_to_string_bound(L.NUM_I64, 0) == 0


def test_error_codes(backend):
    arr = np.arange(4, dtype=np.int32)
    assert raw_call(backend, arr, 11, 4, 64)[0] == L.E_ARG            # an unknown dtype
    assert raw_call(backend, arr, -1, 4, 64)[0] == L.E_ARG
    assert raw_call(backend, arr, L.NUM_I32, -1, 64)[0] == L.E_ARG    # a negative n
    assert raw_call(backend, arr, L.NUM_I32, 4, 64, in_ptr=None)[0] == L.E_ARG   # a null input with n > 0
    assert raw_call(backend, arr, L.NUM_I32, 4, 64, mem=2)[0] == L.E_ARG         # neither host nor device
    rc, n_chars, *_ = raw_call(backend, arr, L.NUM_I32, 0, 64)        # n == 0: nothing to do
    assert rc == L.OVTK_OK and n_chars == 0
    assert raw_call(backend, arr, L.NUM_U8, (1 << 31) // 3 + 1, 64)[0] == L.E_UNSUPPORTED   # the bound reaches 2^31: refused before anything is read
    from openvino_tokenizers_amd.ops import NumericToString
    with pytest.raises(L.OvtkError) as err:
        NumericToString(lib=backend.lib).evaluate([np.zeros(3, np.float16)])
    assert err.value.code == L.E_ARG
    with pytest.raises(L.OvtkError) as err:
        NumericToString(lib=backend.lib).evaluate([arr, arr])
    assert err.value.code == L.E_ARG


# ---------------------------------------------------------------------------------------------- a pin that is not the goldens
def test_live_against_python(emu_lib):
    """Fresh random bit patterns against CPython's own '%g' and str (NaNs skipped: Python writes them without the sign)."""
    from openvino_tokenizers_amd.ops import NumericToString
    op = NumericToString(lib=emu_lib)
    rng = np.random.default_rng()
    seed = int(rng.integers(0, 1 << 32))
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 1 << 64, 5000, dtype=np.uint64).view(np.float64)
    f = f[~np.isnan(f)]
    i = (rng.integers(0, 1 << 64, 5000, dtype=np.uint64) >> rng.integers(0, 64, 5000).astype(np.uint64)).view(np.int64) * rng.choice([-1, 1], 5000)
    for arr, want in ((f, [("%g" % v).encode() for v in f.tolist()]), (i, [str(v).encode() for v in i.tolist()])):
        b, e, c = op.evaluate([arr])
        wb, we, wc = expected(want)
        assert np.array_equal(b, wb) and np.array_equal(e, we) and np.array_equal(c, wc), f"seed {seed}"


# ---------------------------------------------------------------------------------------------- across backends
def test_host_and_device_give_identical_bytes(gpu_backend):
    import torch
    from openvino_tokenizers_amd.ops import NumericToString
    op = NumericToString(lib=gpu_backend.lib)
    for name in DTYPES:
        arr = np.array(golden(name)[0])
        host = op.evaluate([arr])
        dev = op.evaluate([torch.as_tensor(arr, device="cuda")])
        for h, d in zip(host, dev):
            assert isinstance(h, np.ndarray) and d.is_cuda
            assert np.array_equal(h, d.cpu().numpy()), name
