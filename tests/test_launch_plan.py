"""Which kernels a fused encode launches (csrc/api_common.hpp EncodePlan, csrc/api_encode.cpp start_encode, csrc/api_ops.cpp
start_wordpiece_encode): the launch census of tests/gen_golden_launch_census.py replayed on the emulator build, tag -> launch count per
cell, compared exactly with tests/golden/launch_census.json.  A characterisation test: the fixture records what the host code launched
when it was generated, and a change of the host code that is meant to keep the launch sequence passes it without regenerating."""
import json

import pytest

from tests import gen_golden_launch_census as G

GROUPS = G.groups()


@pytest.fixture(scope="module")
def golden():
    return json.loads(G.FIXTURE.read_text())


def test_the_fixture_holds_the_matrix(golden):
    assert sorted(golden) == sorted(G.group_id(g) for g in GROUPS)
    for g in GROUPS:
        assert sorted(golden[G.group_id(g)]) == sorted(G.step_id(s) for s in g["steps"]), G.group_id(g)


def test_the_matrix_reaches_every_front_kernel(golden):
    """Every kind of first kernel turns up somewhere (the profiler's tags: bench.py's kernel_ms keys).  (Not bpe_exact: it takes more
    exact pieces than the folded tail holds, or 2^18 rows.)"""
    tags = {t for steps in golden.values() for cell in steps.values() for t, n in cell.items() if n}
    assert {"encode_small", "lookup_span", "lookup_rows", "lookup_fused", "lookup_pieces", "lookup_words", "bpe_merge",
            "wordpiece_deferred", "compact", "row_width", "special_split", "regex_split", "split_count", "split_write"} <= tags
    cells = [cell for steps in golden.values() for cell in steps.values()]
    assert any(c["short_path.tried"] > c["short_path.exact"] for c in cells), "no cell took the short path's second set of launches"
    assert any(c["short_path.exact"] for c in cells)


@pytest.mark.parametrize("group", GROUPS, ids=G.group_id)
def test_launch_census(emu_lib, golden, group):
    got = G.census(emu_lib, group)
    want = golden[G.group_id(group)]
    for step in group["steps"]:
        sid = G.step_id(step)
        assert got[sid] == want[sid], f"{G.group_id(group)} {sid}: launches per tag differ from the fixture"
