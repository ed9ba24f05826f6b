"""Plain-Python restatement of BytesToChars, CharsToBytes, ContribStringSplit and ContribStringJoin, written from the semantics
include/ovtk_amd.h states (not from the library's kernels): the comparison side of tests/test_string_ops.py, which also pins it
against tokenizers' ByteLevel, the GPT-2 fixture's vocabulary, bytes.split and bytes.join."""
import numpy as np


def bytes_to_unicode():
    """GPT-2's public rule: byte -> character."""
    keep = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
    table, extra = {}, 0
    for b in range(256):
        if b in keep:
            table[b] = chr(b)
        else:
            table[b] = chr(256 + extra)
            extra += 1
    return table


B2C = {b: ch.encode("utf-8") for b, ch in bytes_to_unicode().items()}
C2B = {v: k for k, v in B2C.items()}


def map_bytes(data: bytes) -> bytes:
    return b"".join(B2C[x] for x in data)


class OutOfDomain(ValueError):
    pass


def unmap_bytes(data: bytes) -> bytes:
    """The reference's left-to-right walk, with every read it leaves undefined turned into an error."""
    out, k = bytearray(), 0
    while k < len(data):
        c = data[k]
        if c < 128:
            out.append(c)
            k += 1
            continue
        pair = data[k:k + 2]
        if pair not in C2B:
            raise OutOfDomain(pair)
        out.append(C2B[pair])
        k += 2
    return bytes(out)


def element(begins, ends, chars, i):
    return bytes(bytearray(chars[begins[i]:ends[i]]))


def bytes_to_chars(rb, re_, begins, ends, chars, skips=None):
    """-> (begins, ends, chars): elements no row covers are [0, 0)."""
    ob, oe, out = np.zeros(len(begins), np.int32), np.zeros(len(begins), np.int32), bytearray()
    for j in range(len(rb)):
        for i in range(rb[j], re_[j]):
            ob[i] = len(out)
            text = element(begins, ends, chars, i)
            out += text if skips is not None and skips[i] else map_bytes(text)
            oe[i] = len(out)
    return ob, oe, np.frombuffer(bytes(out), np.uint8)


def chars_to_bytes(rb, re_, begins, ends, chars):
    ob, oe, out = np.zeros(len(rb), np.int32), np.zeros(len(rb), np.int32), bytearray()
    for j in range(len(rb)):
        ob[j] = len(out)
        for i in range(rb[j], re_[j]):
            out += unmap_bytes(element(begins, ends, chars, i))   # (element by element: a pair never spans two)
        oe[j] = len(out)
    return ob, oe, np.frombuffer(bytes(out), np.uint8)


def split_tokens(text: bytes, delim: bytes):
    if not delim:
        return [text[k:k + 1] for k in range(len(text))]
    tokens, pos = [], 0
    while True:
        found = text.find(delim, pos)
        if found < 0:
            tokens.append(text[pos:])
            return tokens
        tokens.append(text[pos:found])
        pos = found + len(delim)


def string_split(begins, ends, chars, delim: bytes, skip_empty: bool):
    """begins / ends of any shape -> (indices [N, rank + 1], begins [N], ends [N], chars, dense_shape)."""
    begins, ends = np.asarray(begins), np.asarray(ends)
    shape = begins.shape
    fb, fe = begins.reshape(-1), ends.reshape(-1)
    indices, vb, ve, out, most = [], [], [], bytearray(), 0
    for p in range(fb.size):
        coord = np.unravel_index(p, shape) if shape else ()
        tokens = split_tokens(element(fb, fe, chars, p), delim)
        most = max(most, len(tokens))
        for t, tok in enumerate(tokens):
            if skip_empty and not tok:
                continue
            indices.append([int(x) for x in coord] + [t])
            vb.append(len(out))
            out += tok
            ve.append(len(out))
    return (np.asarray(indices, np.int64).reshape(len(vb), len(shape) + 1), np.asarray(vb, np.int32), np.asarray(ve, np.int32),
            np.frombuffer(bytes(out), np.uint8), np.asarray(list(shape) + [most], np.int64))


def string_join(begins, ends, chars, sep: bytes, axis: int):
    """begins / ends of any shape -> (begins, ends with the axis removed, chars); numpy does the axis bookkeeping."""
    begins, ends = np.asarray(begins), np.asarray(ends)
    shape = begins.shape
    texts = np.empty(shape, dtype=object)
    fb, fe = begins.reshape(-1), ends.reshape(-1)
    flat = texts.reshape(-1)
    for p in range(fb.size):
        flat[p] = element(fb, fe, chars, p)
    if not shape:
        joined = np.empty((), dtype=object)
        joined[()] = flat[0]
    else:
        moved = np.moveaxis(texts, axis, -1)
        joined = np.empty(moved.shape[:-1], dtype=object)
        for idx in np.ndindex(*moved.shape[:-1]):
            joined[idx] = sep.join(moved[idx])
    ob, oe, out = [], [], bytearray()
    for text in joined.reshape(-1):
        ob.append(len(out))
        out += text
        oe.append(len(out))
    return (np.asarray(ob, np.int32).reshape(joined.shape), np.asarray(oe, np.int32).reshape(joined.shape), np.frombuffer(bytes(out), np.uint8))


def pack(texts):
    """list of bytes -> begins, ends, chars, back to back."""
    lens = np.asarray([len(t) for t in texts], np.int64)
    ends = np.cumsum(lens).astype(np.int32)
    return (ends - lens).astype(np.int32), ends, np.frombuffer(b"".join(texts), np.uint8)
