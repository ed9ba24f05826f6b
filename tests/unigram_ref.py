"""UnigramTokenizer in plain Python: the yardstick of tests/test_unigram.py (the oracle directory holds no Unigram op).

The rules, in this project's words (the reference's are src/unigram_tokenizer.cpp:147-224):
  1. a node per byte position 0..n: token_id = unk_token_id, best_score = float32(0), starts_at = -1;
  2. starts walk the string by characters whose length is read off the lead byte's high nibble alone (0x0-0xB: 1, 0xC-0xD: 2, 0xE: 3,
     0xF: 4), cut to the bytes that are left; nothing is validated;
  3. from each start every vocabulary token that is a prefix of the rest of the string, shortest first, is a candidate for the node at its
     end: candidate = float32(scores[id] + best_score[start]); it replaces the node's entry when the node is unset or candidate >
     best_score, strictly;
  4. no token of exactly the character's length at this start: the node one character on gets the unknown edge under the same rule, with
     unk_score = float32(float64(min(scores)) - 10.0);
  5. back-tracking from node n: an id equal to unk_token_id that directly follows another such id is dropped (whatever produced either);
     the list is reversed;
  6. byte_fallback and fuse_unk change nothing.
Two choices of this library: a vocabulary string that occurs more than once answers with its lowest id; an empty one never matches.
`acc` is the accumulator's type: numpy.float32 is the reference, numpy.float64 is what Hugging Face's Unigram model adds in.
"""
import numpy as np

CHAR_LEN = [1] * 12 + [2, 2, 3, 4]


def char_starts(s):
    out, p = [], 0
    while p < len(s):
        out.append(p)
        p += min(CHAR_LEN[s[p] >> 4], len(s) - p)
    return out


class UnigramRef:
    def __init__(self, vocab, scores, unk_token_id=0, byte_fallback=False, fuse_unk=True, acc=np.float32):
        self.acc = acc
        self.scores = [acc(np.float32(x)) for x in scores]
        self.unk_token_id = int(unk_token_id)
        self.table = {}
        for i, w in enumerate(vocab):
            w = bytes(w)
            if w and w not in self.table:
                self.table[w] = i
        self.longest = max(map(len, self.table), default=0)
        lowest = np.min(np.asarray(scores, np.float32)) if len(scores) else np.finfo(np.float32).max
        self.unk_score = acc(np.float32(np.float64(lowest) - np.float64(10.0)))

    def tokenize(self, s):
        s, n = bytes(s), len(s)
        if n == 0:
            return []
        best = [self.acc(0.0)] * (n + 1)
        starts_at = [-1] * (n + 1)
        token = [self.unk_token_id] * (n + 1)

        def push(end, cand, start, tok):
            if starts_at[end] == -1 or cand > best[end]:
                best[end], starts_at[end], token[end] = cand, start, tok

        for p in char_starts(s):
            clen = min(CHAR_LEN[s[p] >> 4], n - p)
            found = False
            for ln in range(1, min(self.longest, n - p) + 1):
                tok = self.table.get(s[p:p + ln])
                if tok is not None:
                    push(p + ln, self.acc(self.scores[tok] + best[p]), p, tok)
                    found = found or ln == clen
            if not found:
                push(p + clen, self.acc(self.unk_score + best[p]), p, self.unk_token_id)
        out, end, prev = [], n, -1
        while end > 0:
            tok, end = token[end], starts_at[end]
            if tok == self.unk_token_id and prev == self.unk_token_id:
                continue
            out.append(tok)
            prev = tok
        return out[::-1]

    def __call__(self, ragged_begins, ragged_ends, begins, ends, chars):
        """The op: ragged strings in, (begins, ends, ids) out; a row's ids are those of its strings one after the other."""
        data = bytes(np.asarray(chars, np.uint8))
        memo, ob, oe, ids = {}, [], [], []
        for rb, re_ in zip(np.asarray(ragged_begins).tolist(), np.asarray(ragged_ends).tolist()):
            ob.append(len(ids))
            for col in range(rb, re_):
                s = data[int(begins[col]):int(ends[col])]
                if s not in memo:
                    memo[s] = self.tokenize(s)
                ids += memo[s]
            oe.append(len(ids))
        return np.asarray(ob, np.int32), np.asarray(oe, np.int32), np.asarray(ids, np.int32)
