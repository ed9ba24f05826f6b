"""Writes tests/golden/golden_numeric_to_string.npz: per element type the inputs of tests/test_numeric_to_string.py and the texts
NumericToString (src/numeric_to_string.cpp:18-92) gives for them.

The texts come from a few-line C++ restatement of the op, written here from its description -- std::to_string per integer type (the
8- and 16-bit ones through int32 / uint32), std::ostringstream << x for float and double, "true" / "false" for a boolean byte --
compiled with g++ in a temporary directory and fed the inputs as raw bytes.  Nothing is downloaded.  Before it writes the file the
generator checks the restatement against Python: every finite float text is '%g' % float(v) (CPython formats with its own correctly
rounded conversion, not with the C library's), every integer text is str(int(v)); and it checks that the float inputs hold what they
are there for: at least 40 exact ties of the sixth digit, at least 40 values one ulp from a tie or from a power of ten, fixed and
exponent notation, two- and three-digit exponents.

    python tests/gen_golden_numeric_to_string.py
"""
import math
import subprocess
import sys
import tempfile
from fractions import Fraction
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent / "golden" / "golden_numeric_to_string.npz"
DTYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64", "bool"]

RESTATEMENT = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

template <class T, class F>
static void each(const std::vector<char>& raw, F text) {
    for (size_t i = 0; i + sizeof(T) <= raw.size(); i += sizeof(T)) {
        T v;
        std::memcpy(&v, raw.data() + i, sizeof(T));
        const std::string s = text(v);
        std::fwrite(s.data(), 1, s.size(), stdout);
        std::fputc('\n', stdout);
    }
}
template <class T>
static std::string streamed(T v) {
    std::ostringstream oss;
    oss << v;
    return oss.str();
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const std::string t = argv[1];
    std::ifstream f(argv[2], std::ios::binary);
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (t == "int64") each<int64_t>(raw, [](int64_t v) { return std::to_string(v); });
    else if (t == "int32") each<int32_t>(raw, [](int32_t v) { return std::to_string(v); });
    else if (t == "int16") each<int16_t>(raw, [](int16_t v) { return std::to_string(static_cast<int32_t>(v)); });
    else if (t == "int8") each<int8_t>(raw, [](int8_t v) { return std::to_string(static_cast<int32_t>(v)); });
    else if (t == "uint64") each<uint64_t>(raw, [](uint64_t v) { return std::to_string(v); });
    else if (t == "uint32") each<uint32_t>(raw, [](uint32_t v) { return std::to_string(v); });
    else if (t == "uint16") each<uint16_t>(raw, [](uint16_t v) { return std::to_string(static_cast<uint32_t>(v)); });
    else if (t == "uint8") each<uint8_t>(raw, [](uint8_t v) { return std::to_string(static_cast<uint32_t>(v)); });
    else if (t == "float32") each<float>(raw, [](float v) { return streamed(v); });
    else if (t == "float64") each<double>(raw, [](double v) { return streamed(v); });
    else if (t == "bool") each<uint8_t>(raw, [](uint8_t v) { return std::string(v ? "true" : "false"); });
    else return 2;
    return 0;
}
"""


# ------------------------------------------------------------------------------------------------------ inputs
def integer_inputs(name, rng):
    info = np.iinfo(name)
    vals = [0, 1, info.min, info.max] + ([-1] if info.min < 0 else [])
    k = 0
    while 10 ** k - 1 <= info.max:
        for v in (10 ** k - 1, 10 ** k, 10 ** k + 1):
            if v <= info.max:
                vals.append(v)
            if -v >= info.min:
                vals.append(-v)
        k += 1
    for _ in range(2000):   # a uniformly random bit length, then uniformly random bits of that length
        bits = int(rng.integers(0, info.bits + (0 if info.min < 0 else 1)))
        v = int(rng.integers(0, 1 << 62)) << 2 | int(rng.integers(0, 4))
        v &= (1 << bits) - 1
        if bits:
            v |= 1 << (bits - 1)
        if info.min < 0 and rng.integers(0, 2):
            v = -v
        vals.append(min(max(v, info.min), info.max))
    return np.array(vals, dtype=object).astype(name)


def exact_ties():
    """60 doubles whose exact value has seven significant digits, the seventh a 5: (N + 1/2) * 10^(X - 5) for X = -4 .. 19."""
    ties = []
    for x in range(-4, 20):
        # below X = 5 the value is (2N + 1) / (2 * 10^(5 - X)), a double only if 5^(5 - X) divides 2N + 1; above X = 5 it is the
        # integer (2N + 1) * 5^(X - 5) * 2^(X - 6), a double only while (2N + 1) * 5^(X - 5) fits 53 bits
        step = 5 ** max(5 - x, 0)
        k = -(-200001 // step) | 1
        want, found = (1 if x == -4 else 4 if 0 <= x < 5 else 3 if 5 <= x < 8 else 2), 0   # (X = -4 has one: 2^-10)
        while found < want and step * k < 2000000:
            v = Fraction(step * k, 2) * Fraction(10) ** (x - 5)   # step * k = 2N + 1
            if Fraction(float(v)) == v:
                ties.append(float(v))
                found += 1
                k += 2 * max(1, 150000 // step) + 2 * found   # (spread over N, both parities)
            else:
                k += 2
        assert found == want, (x, found)
    assert len(ties) == 60
    return ties


def is_tie(v):
    """True if the exact value of the finite non-zero double v lies half way between two six-digit decimals."""
    fr = abs(Fraction(v))
    x = int(math.floor(math.log10(fr)))
    while Fraction(10) ** x > fr:
        x -= 1
    while Fraction(10) ** (x + 1) <= fr:
        x += 1
    scaled = fr * Fraction(10) ** (5 - x)
    return scaled - scaled.numerator // scaled.denominator == Fraction(1, 2)


def float_inputs(name, rng):
    f64 = name == "float64"
    ft = np.float64 if f64 else np.float32
    ut = np.uint64 if f64 else np.uint32
    info = np.finfo(ft)
    hand = [0.0, -0.0, np.inf, -np.inf, float(info.smallest_subnormal), float(info.tiny) - float(info.smallest_subnormal), float(info.tiny), float(info.max),
            0.5, 1234565.0, 1234575.0, 0.1234565, 1.234565e10, 1.234565e22, 1234565.0 / 2 ** 20,
            999999.5, 999999.4999999999, 9.9999995e-05, 9.99999949e-05, 99999.95, 0.0001, 0.00001, 100000.0, 1000000.0]
    bits = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000012345] if f64 else [0x7FC00000, 0xFFC00000, 0x7F812345]   # NaN, -NaN, a payload
    ties = [t for t in exact_ties() if float(ft(t)) == t]
    near = []
    for t in ties:
        near += [np.nextafter(ft(t), ft(np.inf)), np.nextafter(ft(t), ft(-np.inf))]
    lo, hi = (-323, 308) if f64 else (-45, 38)
    for k in range(lo, hi + 1):
        p = ft("1e%d" % k)
        near += [p, np.nextafter(p, ft(np.inf)), np.nextafter(p, ft(-np.inf))]
    with np.errstate(over="ignore", under="ignore"):
        vals = np.concatenate([np.array(hand, dtype=np.float64).astype(ft), np.array(ties, dtype=np.float64).astype(ft), -np.array(ties[:8], dtype=np.float64).astype(ft),
                               np.array(near, dtype=ft)])
    rand = rng.integers(0, 1 << (64 if f64 else 32), size=20000, dtype=np.uint64).astype(ut)
    return np.concatenate([vals.view(ut), np.array(bits, dtype=ut), rand]).view(ft), len(ties)


# ------------------------------------------------------------------------------------------------------ the run
def texts_of(exe, name, arr, tmp):
    raw = Path(tmp) / f"{name}.bin"
    raw.write_bytes(arr.tobytes())
    out = subprocess.run([str(exe), name, str(raw)], check=True, capture_output=True).stdout
    texts = out.split(b"\n")[:-1]
    assert len(texts) == arr.size, (name, len(texts), arr.size)
    return texts


def main():
    np.seterr(all="ignore")   # (NaNs and infinities are among the inputs on purpose)
    rng = np.random.default_rng(20260519)
    store = {}
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "numeric_to_string_restated.cpp"
        src.write_text(RESTATEMENT)
        exe = Path(tmp) / "numeric_to_string_restated"
        subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), str(src)], check=True)
        for name in DTYPES:
            n_ties_in = 0
            if name == "bool":
                arr = np.array([0, 1, 2, 255], dtype=np.uint8)
            elif name.startswith("float"):
                arr, n_ties_in = float_inputs(name, rng)
            else:
                arr = integer_inputs(name, rng)
            texts = texts_of(exe, name, arr, tmp)
            if name.startswith("float"):
                ties = near = 0
                forms = set()
                as64 = arr.astype(np.float64)
                tie_at = np.zeros(arr.size, bool)
                for i, (v, t) in enumerate(zip(as64, texts)):
                    if not np.isfinite(v):
                        continue
                    assert t == ("%g" % float(v)).encode(), (name, float(v).hex(), t, "%g" % float(v))
                    if v != 0 and is_tie(float(v)):
                        ties += 1
                        tie_at[i] = True
                    if b"e" in t:
                        forms.add("e3" if len(t.split(b"e")[1]) == 4 else "e2")
                    elif v != 0:
                        forms.add("fixed")
                # one ulp from a tie or from a power of ten
                up, down = np.nextafter(arr, arr.dtype.type(np.inf)), np.nextafter(arr, arr.dtype.type(-np.inf))
                tie_values = set(arr[tie_at].tolist())
                pow10 = {float(arr.dtype.type("1e%d" % k)) for k in range(-330, 310)}
                for v, a, b in zip(arr.tolist(), up.tolist(), down.tolist()):
                    if np.isfinite(v) and (a in tie_values or b in tie_values or a in pow10 or b in pow10):
                        near += 1
                assert ties >= 40 and ties >= n_ties_in, (name, ties, n_ties_in)
                assert near >= 40, (name, near)
                assert forms == {"fixed", "e2"} | ({"e3"} if name == "float64" else set()), (name, forms)
                print(f"{name}: {arr.size} values, {ties} exact ties, {near} one ulp from a tie or a power of ten, forms {sorted(forms)}")
                arr = arr.view(np.uint64 if name == "float64" else np.uint32)   # (bit patterns: NaN payloads survive the file)
            elif name != "bool":
                for v, t in zip(arr.tolist(), texts):
                    assert t == str(int(v)).encode(), (name, v, t)
            else:
                assert texts == [b"false", b"true", b"true", b"true"]
            store[f"in_{name}"] = arr
            store[f"ends_{name}"] = np.cumsum([len(t) for t in texts]).astype(np.int32)
            store[f"chars_{name}"] = np.frombuffer(b"".join(texts), dtype=np.uint8)
    np.savez_compressed(OUT, **store)
    size = OUT.stat().st_size
    assert size < 1000000, size
    print(f"wrote {OUT} ({size} bytes)")


if __name__ == "__main__":
    sys.exit(main())
