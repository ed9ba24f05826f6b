"""Differential fuzzer for RegexNormalization's plan on the host: random patterns from tools/fuzz_regex_host.py's grammar (with more capture
groups and top-level alternations) and random templates, every string over a small alphabet up to length 3 plus random longer ones,
the plan run by tools/regex_subst_host_check.cpp against pcre2_substitute as the reference calls it (tests/pcre2_substitute.py).  Build the
checker first (see its header), or let `build()` do it.
    python tools/fuzz_regex_subst_host.py SEED N_CASES"""
import itertools
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
CHECK = ROOT / "tools" / "build" / "regex_subst_host_check"
ATOMS = ["a", "b", "c", " ", r"\n", ".", r"\s", r"\S", r"\d", r"\w", r"\W", "[ab]", "[^a]", "[a-c]", r"[^\s]", r"\p{L}", r"\P{L}", r"\p{N}",
         "1", "é", "[é1]", r"[\s\d]", r"\b", r"\B", "^", "$", r"\z", r"\A"]
QUANT = ["", "", "", "", "*", "+", "?", "{1,2}", "{2}", "{0,2}", "*?", "+?", "??", "*+", "++", "?+"]
ALPHA = ["a", "b", "c", " ", "\n", "1", "é", "A"]
LITERALS = ["X", "-", " ", "", "é", "$$", "<", "XXXXXXXXXX", "YYYYYYYY"]
BROKEN = ["$", "${1", "$w", "$9", "${x}"]   # what PCRE2 answers with an error: the op is the identity


def build():
    src = [ROOT / "tools" / "regex_subst_host_check.cpp", ROOT / "openvino_tokenizers_amd" / "csrc" / "regex_subst.cpp",
           ROOT / "openvino_tokenizers_amd" / "csrc" / "regex_compile.cpp"]
    hdr = list((ROOT / "openvino_tokenizers_amd" / "csrc").glob("regex_*.hpp"))
    if CHECK.exists() and all(CHECK.stat().st_mtime >= p.stat().st_mtime for p in src + hdr):
        return CHECK
    CHECK.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + str(ROOT / "openvino_tokenizers_amd" / "csrc")] + [str(p) for p in src] + ["-o", str(CHECK)], check=True)
    return CHECK


def fixed(rng):
    return "".join(ATOMS[rng.integers(18)] for _ in range(int(rng.integers(1, 4))))


def gen(rng, depth=0):
    r = rng.random()
    if depth >= 3 or r < 0.36:
        a = ATOMS[rng.integers(len(ATOMS))]
        if a in (r"\b", r"\B", "^", "$", r"\z", r"\A"):
            return a
        return a + QUANT[rng.integers(len(QUANT))]
    if r < 0.54:
        return gen(rng, depth + 1) + gen(rng, depth + 1)
    if r < 0.62:
        return "(?:" + gen(rng, depth + 1) + "|" + gen(rng, depth + 1) + ")" + QUANT[rng.integers(len(QUANT))]
    if r < 0.80:   # capture groups, mostly unquantified: the ones a template can refer to
        return "(" + gen(rng, depth + 1) + ")" + (QUANT[rng.integers(len(QUANT))] if rng.random() < 0.3 else "")
    if r < 0.86:
        return ["(?=", "(?!"][rng.integers(2)] + gen(rng, depth + 1) + ")"
    if r < 0.91:
        return ["(?<=", "(?<!"][rng.integers(2)] + "|".join(fixed(rng) for _ in range(int(rng.integers(1, 3)))) + ")"
    if r < 0.97:
        return "(?>" + gen(rng, depth + 1) + ")" + QUANT[rng.integers(len(QUANT))]
    return "(?i:" + gen(rng, depth + 1) + ")"


def gen_case(rng):
    """(pattern, template, global_replace)"""
    r = rng.random()
    if r < 0.35:     # top-level alternatives, sometimes under one outer group or a branch reset
        alts = "|".join(gen(rng, 1) for _ in range(int(rng.integers(2, 4))))
        pattern = [alts, "(" + alts + ")", "(?|" + alts + ")", "(?:" + alts + ")"][rng.integers(4)]
    else:
        pattern = gen(rng)
    n_groups = sum(1 for k, ch in enumerate(pattern) if ch == "(" and pattern[k + 1:k + 2] not in ("?", "*") and pattern[k - 1:k] != "\\")
    parts = []
    for _ in range(int(rng.integers(0, 4))):
        r2 = rng.random()
        if r2 < 0.45:
            parts.append(LITERALS[rng.integers(len(LITERALS))])
        elif r2 < 0.93:   # a group the pattern has (mostly): $n, ${n} or the op's own \n
            g = int(rng.integers(0, n_groups + 1)) if rng.random() < 0.93 else n_groups + 1
            parts.append(["$%d", "${%d}", "\\%d"][rng.integers(3) if 0 < g < 10 else rng.integers(2)] % g)
        else:
            parts.append(BROKEN[rng.integers(len(BROKEN))])
    template = "".join(parts)
    return pattern, template, bool(rng.random() < 0.8)


def subjects(rng):
    strings = ["".join(t) for k in range(1, 4) for t in itertools.product(ALPHA, repeat=k)]
    return strings + ["".join(rng.choice(ALPHA, size=int(k))) for k in rng.integers(4, 14, size=200)] + ["", "a" * 40, "ab " * 9]


def run_case(pattern, template, global_replace, strings):
    """-> ("same" | "unsupported", info) or ("BAD", what).  Undecided strings (the buffer quirk with an open rc) and
    strings on which PCRE2's backtracker hits its match limit (the reference then returns the input) are not compared."""
    from tests.pcre2_substitute import Substitute
    r = subprocess.run([str(CHECK), pattern, template, "1" if global_replace else "0"] + strings, capture_output=True)
    if r.returncode == 2:
        return "unsupported", r.stdout.decode(errors="replace").strip()
    if r.returncode != 0:
        return "BAD", f"checker exit {r.returncode}: {r.stderr[-300:]!r}"
    lines = r.stdout.decode().split("\n")
    ref = Substitute(pattern, template, global_replace)
    undecided = 0
    for s, line in zip(strings, lines[1:]):
        if line == "UNDECIDED":
            undecided += 1
            continue
        got = b"" if line == "-" else bytes.fromhex(line)
        want = ref(s.encode())
        if got != want and not ref.gave_up:
            return "BAD", f"{lines[0]}: on {s!r} the plan gives {got!r}, PCRE2 {want!r}"
    return "same", f"{lines[0]} undecided={undecided}"


def main():
    seed, n = int(sys.argv[1]), int(sys.argv[2])
    build()
    rng = np.random.default_rng(seed)
    strings = subjects(rng)
    cnt, why = {}, {}
    for _ in range(n):
        case = gen_case(rng)
        verdict, info = run_case(*case, strings)
        cnt[verdict] = cnt.get(verdict, 0) + 1
        if verdict == "BAD":
            print("BAD", repr(case), info)
        elif verdict == "unsupported":
            k = info.split("(")[1].split(")")[0] if "pattern outside" in info else info[:70]
            why[k] = why.get(k, 0) + 1
        else:
            k = info.split(" undecided")[0]
            why[k] = why.get(k, 0) + 1
    print("seed", seed, cnt)
    for k, v in sorted(why.items(), key=lambda x: -x[1]):
        print("   ", v, k)


if __name__ == "__main__":
    main()
