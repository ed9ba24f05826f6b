"""The yardstick of RegexNormalization: PCRE2Wrapper::substitute (src/utils.cpp:315-382) restated over the system's libpcre2-8 through
ctypes, with the reference's flags (PCRE2_UTF | PCRE2_UCP to compile, PCRE2_NO_UTF_CHECK to match), its first pcre2_match whose return
value sizes the buffer -- 4 * (len + rc * template_len) bytes --, and "any negative code gives the input back"; around it the op's two
rewrites of its inputs (src/regex_normalization.cpp:19-53) and evaluate_normalization_helper's layout (src/utils.cpp:178-234).
Test infrastructure: the product never runs PCRE2."""
import ctypes as C
import ctypes.util

import numpy as np

_lib = C.CDLL(ctypes.util.find_library("pcre2-8") or "libpcre2-8.so.0")
PCRE2_UTF, PCRE2_UCP, PCRE2_NO_UTF_CHECK, PCRE2_SUBSTITUTE_GLOBAL = 0x00080000, 0x00020000, 0x40000000, 0x00000100
_lib.pcre2_compile_8.restype = C.c_void_p
_lib.pcre2_compile_8.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.c_void_p]
_lib.pcre2_match_data_create_from_pattern_8.restype = C.c_void_p
_lib.pcre2_match_data_create_from_pattern_8.argtypes = [C.c_void_p, C.c_void_p]
_lib.pcre2_match_8.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p]
_lib.pcre2_substitute_8.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t,
                                    C.c_char_p, C.POINTER(C.c_size_t)]
_lib.pcre2_match_data_free_8.argtypes = [C.c_void_p]
_lib.pcre2_code_free_8.argtypes = [C.c_void_p]

SEARCH_PATTERN_REWRITES = {   # src/regex_normalization.cpp:32-36
    r" ([\\.\\?\\!,])| ('[ms])| (') | ('[rv]e)| (n't)": r"(?| ([\\.\\?\\!,])| ('[ms])| (') | ('[rv]e)| (n't))",
    r"(^)(.)": r"(^)([\s\S])",
    r"(^)(.+)": r"(^)([\s\S])",
}


def reformat_replace_pattern(replace: bytes) -> bytes:   # :19-30
    for i in b"123456789":
        replace = replace.replace(b"\\" + bytes([i]), b"$" + bytes([i]))
    return replace


class Substitute:
    """One RegexNormalization node: pattern and template as the op's constructor prepares them (:58-77)."""

    def __init__(self, pattern, replace, global_replace=True, fix_pattern=True):
        pattern = pattern if isinstance(pattern, str) else pattern.decode()
        replace = replace.encode() if isinstance(replace, str) else bytes(replace)
        if fix_pattern:
            pattern = SEARCH_PATTERN_REWRITES.get(pattern, pattern)
        self.replace = reformat_replace_pattern(replace)
        self.global_replace = bool(global_replace)
        pat = pattern.encode()
        err, off = C.c_int(0), C.c_size_t(0)
        self.code = _lib.pcre2_compile_8(pat, len(pat), PCRE2_UTF | PCRE2_UCP, C.byref(err), C.byref(off), None)   # utils.cpp:259-261

    def __del__(self):
        if getattr(self, "code", None):
            _lib.pcre2_code_free_8(self.code)

    GAVE_UP = (-47, -53, -63)   # PCRE2_ERROR_MATCHLIMIT / DEPTHLIMIT / HEAPLIMIT: the backtracker ran out of steps

    def __call__(self, subject: bytes) -> bytes:   # utils.cpp:315-382
        self.gave_up = False   # (a property of PCRE2's search order and limits, not of the pattern: fuzzers do not compare such subjects)
        if not self.code:
            return subject
        md = _lib.pcre2_match_data_create_from_pattern_8(self.code, None)
        try:
            n = _lib.pcre2_match_8(self.code, subject, len(subject), 0, PCRE2_NO_UTF_CHECK, md, None)
            if n < 0:
                self.gave_up = n in self.GAVE_UP
                return subject
            size = 4 * (len(subject) + n * len(self.replace))
            buf = C.create_string_buffer(max(size, 1))
            out_len = C.c_size_t(size)
            rc = _lib.pcre2_substitute_8(self.code, subject, len(subject), 0, (PCRE2_SUBSTITUTE_GLOBAL if self.global_replace else 0) | PCRE2_NO_UTF_CHECK,
                                         md, None, self.replace, len(self.replace), buf, C.byref(out_len))
            if rc < 0:
                self.gave_up = rc in self.GAVE_UP
                return subject
            return buf.raw[:out_len.value]
        finally:
            _lib.pcre2_match_data_free_8(md)


def normalize(strings, pattern, replace, global_replace=True, skips=None, fix_pattern=True):
    """evaluate_normalization_helper over a list of bytes -> (begins, ends, chars), written back to back from 0."""
    f = Substitute(pattern, replace, global_replace, fix_pattern)
    outs = [s if (skips is not None and skips[i]) else f(s) for i, s in enumerate(strings)]
    ends = np.cumsum([len(o) for o in outs], dtype=np.int64).astype(np.int32) if outs else np.zeros(0, np.int32)
    begins = np.concatenate([[0], ends[:-1]]).astype(np.int32) if outs else np.zeros(0, np.int32)
    return begins, ends, np.frombuffer(b"".join(outs), np.uint8)
