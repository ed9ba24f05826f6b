"""Generates tests/golden/table_collisions.json: the inputs on which the device hash tables of csrc/tables.hpp collide, and the facts that make
each of them a case (slots, chain lengths, wraps, overflowing buckets, stored / refused) -- the fixture of tests/test_table_collisions.py.

Builds tests/emu/table_collisions.cpp (host code: the project's own hash functions and builders, tables.cpp linked) and writes what it
prints.  The searches are deterministic, the run takes about a second.  The file holds small inputs and recorded facts only; the large BPE
vocabularies are named by their size (base token i is four letters, i in base 26) and their merges by (left id, right id).

Run here; the .json is committed:    python -m tests.gen_golden_table_collisions
"""
import json
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
G = ROOT / "tests" / "golden"


def main():
    subprocess.run(["make", "-C", str(ROOT / "openvino_tokenizers_amd" / "csrc"), "-s", "collisions"], check=True)
    out = subprocess.run([str(ROOT / "tests" / "emu" / "build" / "table_collisions")], check=True, capture_output=True, text=True).stdout
    cases = json.loads(out)   # (it parses: nothing half-written is committed)
    (G / "table_collisions.json").write_text(out)
    for family, members in cases.items():
        print(f"{family}: {', '.join(members)}")
    print(f"{len(out)} bytes")


if __name__ == "__main__":
    main()
