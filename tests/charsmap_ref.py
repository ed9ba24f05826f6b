"""CharsMapNormalization in plain Python: the yardstick of tests/test_charsmap.py (the oracle directory holds no normalizer).

The rules, in this project's words (the reference's ops -- src/charsmap_normalization.cpp:34-69, src/normalize_unicode.cpp:32-62,
src/case_fold.cpp:34-73 -- all call sentencepiece's normalizer::Normalizer::Normalize per string, src/utils.cpp:178-234):
  * a blob is u32 trie_size | trie_size bytes of Darts double-array units (u32 each) | NUL-terminated replacement strings; an empty blob
    has no trie;
  * the trie is walked as Darts' commonPrefixSearch walks it: offset(u) = (u >> 10) << ((u & 0x200) >> 6), label(u) = u & 0x800000FF,
    has_leaf(u) = (u >> 8) & 1, value(u) = u & 0x7FFFFFFF; pos = offset(units[0]); per byte c: pos ^= c, stop unless label(units[pos]) ==
    c, pos ^= offset(units[pos]); with has_leaf the key of this length maps to the replacement at byte value(units[pos]); the first 32
    matches are looked at, the longest of them wins;
  * a prefix: the longest match's replacement and its length; no match: one well-formed UTF-8 character unchanged (right trail bytes,
    not overlong, no surrogate, at most U+10FFFF, not cut off by the string's end), else EF BF BD for ONE byte;
  * Normalize: empty in, empty out; with remove_extra_whitespaces leading prefixes that emit exactly " " are skipped (nothing left:
    empty out, no dummy prefix); add_dummy_prefix puts one space symbol in front; per prefix, while the previous one ended in a space
    (initially: remove_extra_whitespaces) leading spaces are dropped, what is left is appended with 0x20 -> E2 96 81 under
    escape_whitespaces, and "ended in a space" is updated only by a non-empty rest (and cleared after every prefix without
    remove_extra_whitespaces); with remove_extra_whitespaces the space symbol is stripped from the end for as long as it is there --
    under escape_whitespaces that eats a literal U+2581 of the input too;
  * the op: outputs back to back from offset 0 whatever the input offsets were; a row with skips[i] != 0 is copied unchanged.
"""
import struct

import numpy as np

SPACE_SYMBOL = b"\xe2\x96\x81"
REPLACEMENT = b"\xef\xbf\xbd"
MAX_TRIE_RESULTS = 32


def utf8_char_len(s, p):
    """Length of the well-formed UTF-8 character at s[p:], 0 if there is none."""
    c, n = s[p], len(s) - p
    if c < 0x80:
        return 1
    if 0xC2 <= c <= 0xDF:
        need, lo, hi = 2, 0x80, 0xBF
    elif 0xE0 <= c <= 0xEF:
        need, lo, hi = 3, (0xA0 if c == 0xE0 else 0x80), (0x9F if c == 0xED else 0xBF)
    elif 0xF0 <= c <= 0xF4:
        need, lo, hi = 4, (0x90 if c == 0xF0 else 0x80), (0x8F if c == 0xF4 else 0xBF)
    else:
        return 0
    if n < need or not lo <= s[p + 1] <= hi:
        return 0
    return need if all(0x80 <= s[p + k] <= 0xBF for k in range(2, need)) else 0


class CharsMapRef:
    def __init__(self, blob=b"", add_dummy_prefix=False, remove_extra_whitespaces=False, escape_whitespaces=False):
        blob = bytes(blob)
        self.add_dummy_prefix, self.remove_extra_whitespaces, self.escape_whitespaces = bool(add_dummy_prefix), bool(remove_extra_whitespaces), bool(escape_whitespaces)
        self.units, self.strings = None, b""
        if blob:
            (size,) = struct.unpack_from("<I", blob, 0)
            assert 4 + size <= len(blob) and size % 4 == 0, "malformed charsmap blob"
            self.units = np.frombuffer(blob, "<u4", size // 4, 4).tolist()
            self.strings = blob[4 + size:]

    def longest_match(self, s, p):
        """(key length, replacement) of the longest of the first 32 keys that are prefixes of s[p:]; (0, None) without one."""
        u = self.units
        if not u:
            return 0, None
        off = lambda x: (x >> 10) << ((x & 0x200) >> 6)   # noqa: E731
        pos, found, best, value = off(u[0]), 0, 0, 0
        for k in range(p, len(s)):
            pos ^= s[k]
            if pos >= len(u) or (u[pos] & 0x800000FF) != s[k]:
                break
            unit = u[pos]
            pos ^= off(unit)
            if (unit >> 8) & 1:
                if found < MAX_TRIE_RESULTS and k + 1 - p > best:
                    best, value = k + 1 - p, u[pos] & 0x7FFFFFFF
                found += 1
        if not best:
            return 0, None
        return best, self.strings[value:self.strings.index(b"\0", value)]

    def prefix(self, s, p):
        """(emitted bytes, bytes consumed) at position p."""
        n, rep = self.longest_match(s, p)
        if n:
            return rep, n
        n = utf8_char_len(s, p)
        return (s[p:p + n], n) if n else (REPLACEMENT, 1)

    def normalize(self, s):
        s = bytes(s)
        if not s:
            return b""
        p = 0
        if self.remove_extra_whitespaces:
            while p < len(s):
                sp, n = self.prefix(s, p)
                if sp != b" ":
                    break
                p += n
            if p == len(s):
                return b""
        out = bytearray()
        space = SPACE_SYMBOL if self.escape_whitespaces else b" "
        if self.add_dummy_prefix:
            out += space
        prev_space = self.remove_extra_whitespaces
        while p < len(s):
            sp, n = self.prefix(s, p)
            while prev_space and sp.startswith(b" "):
                sp = sp[1:]
            if sp:
                out += sp.replace(b" ", space)
                prev_space = sp.endswith(b" ")
            p += n
            if not self.remove_extra_whitespaces:
                prev_space = False
        if self.remove_extra_whitespaces:
            while out.endswith(space):
                del out[len(out) - len(space):]
        return bytes(out)

    def __call__(self, begins, ends, chars, skips=None):
        """The op: strings in, (begins, ends, chars) out, written back to back from 0."""
        data = bytes(np.asarray(chars, np.uint8))
        ob, oe, out = [], [], bytearray()
        for i, (b, e) in enumerate(zip(np.asarray(begins).tolist(), np.asarray(ends).tolist())):
            ob.append(len(out))
            out += data[b:e] if skips is not None and skips[i] else self.normalize(data[b:e])
            oe.append(len(out))
        return np.asarray(ob, np.int32), np.asarray(oe, np.int32), np.frombuffer(bytes(out), np.uint8)


def case_fold_ascii(data, lower=True):
    """CaseFold with encoding "": bytes 'A'..'Z' + 32 (lower) or 'a'..'z' - 32, every other byte unchanged (src/case_fold.hpp:21-23)."""
    lo, hi, delta = (0x41, 0x5A, 32) if lower else (0x61, 0x7A, -32)
    return bytes(c + delta if lo <= c <= hi else c for c in bytes(data))
