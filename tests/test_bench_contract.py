"""bench.py end to end on the GPU box: one JSON line with the fields the driver reads, for the plain run, for the run with
every leg (--full) and for the exchange loop (one-rank RCCL group), at a small row count so that all finish in seconds."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _run(*flags):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "6", "--warmup", "2", "--rows", "4096", *flags],
                       capture_output=True, text=True, timeout=600, env=env, cwd=str(ROOT))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run():
    """A plain run: the headline fields, none of the legs --full adds, and the outputs of its last timed step on request."""
    import tempfile
    with tempfile.TemporaryDirectory() as out:
        d = _run("--dump-outputs", out)
        files = {p.name: p for p in Path(out).iterdir()}
        assert sorted(files) == ["begins.npy", "ends.npy", "ids.npy"]
        got = {k[:-4]: np.load(v) for k, v in files.items()}
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype"):
        assert key in d, key
    assert d["steps"] == 6 and d["warmup"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0 and d["full"] is False
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["stress"] is None and d["steady"] is None and d["kernel_ms"] is None
    assert all(x.dtype in (np.float32, np.float64) for x in got.values())
    assert not any(f["sampled"] for f in d["dumped_outputs"]["files"].values())
    # the last timed step (index warmup + steps - 1 = 7) encoded batch 7 of the rotation: the oracle's ids for it, bit for bit
    from oracle import oracle as O
    from tools.harness import BpeTok
    from tools.workloads import TextModel, ragged_rows
    tok = BpeTok.load("gpt2")
    b, e, c = TextModel(1234, "zipf").batch(4096, 512, seed=1000 + 7 * 7)
    rb, re_ = ragged_rows(4096)
    rb_, re2, ids = tok.oracle()(*O.RegexSplit(tok.pattern, "isolate")(rb, re_, b, e, c)[:5])
    assert np.array_equal(got["begins"], rb_) and np.array_equal(got["ends"], re2) and np.array_equal(got["ids"], ids)


def test_dump_outputs_budget(tmp_path):
    """--dump-outputs' writer (CPU): exact float32 where it can be, float64 otherwise, and a fixed seeded sample under the budget."""
    sys.path.insert(0, str(ROOT))
    import bench
    small = np.arange(10, dtype=np.int32)
    wide = np.array([0, 1 << 24, -(1 << 30)], np.int64)
    big = np.arange(1000, dtype=np.int32).reshape(10, 100)
    w = bench.dump_outputs(tmp_path / "a", ["small", "wide", "big"], [small, wide, big], budget=2048)
    assert w["small"] == {"shape": [10], "dtype": "float32", "sampled": False}
    assert w["wide"] == {"shape": [3], "dtype": "float64", "sampled": False}
    assert w["big"]["sampled"] and w["big"]["dtype"] == "float32"
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in w}
    assert sum(x.nbytes for x in got.values()) <= 2048
    assert np.array_equal(got["small"], small) and np.array_equal(got["wide"], wide)
    assert np.all(np.diff(got["big"]) > 0) and set(got["big"].tolist()) <= set(range(1000))
    again = bench.dump_outputs(tmp_path / "b", ["small", "wide", "big"], [small, wide, big], budget=2048)
    assert again == w and np.array_equal(np.load(tmp_path / "b" / "big.npy"), got["big"])
    w = bench.dump_outputs(tmp_path / "c", ["big"], [big])
    assert w["big"] == {"shape": [10, 100], "dtype": "float32", "sampled": False}


@pytest.mark.gpu
def test_bench_json_line():
    d = _run("--full")
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["vs_baseline"] is None
    assert d["value"] > 0 and d["higher_is_better"] is True and "workload" in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and 0 < r["frac"] < 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4
    assert r["alone"]["kernel_ms"] > 0 and r["step"]["frac"] > 0
    assert r["kernel_ms"] == r["alone"]["kernel_ms"], "frac must come from the one-stream leg, not from overlapped launches"
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0
    assert d["cpu_baseline_all_cores"]["cores"] >= 1 and d["cpu_baseline_all_cores"]["value"] > 0
    assert d["stress"]["uniform_text"]["value"] > 0 and d["stress"]["no_memo"]["ms_per_step"] > 0
    assert d["stress"]["fixed_memo_only"]["ms_per_step"] > 0 and d["stress"]["mixed_script_text"]["value"] > 0
    memo = d["config"]["piece_memo"]
    # (memo_learn = 0, the library's default: the first level learns up to max(cache_capacity, the store's capacity) pieces)
    assert memo["fixed"] > 1000 and memo["cache_capacity"] == 20000 and memo["memo_learn"] == 0
    assert 0 < memo["learned"] <= max(memo["cache_capacity"], memo["store"]["capacity"])
    assert d["stress"]["reference_cache_count"]["value"] > 0
    assert d["end_to_end"]["value"] > 0 and "8 distinct batches" in d["config"]["workload"]
    assert d["parity_prefix_bit_exact"] is True


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["1", "5", "r2d", "vocab_encoder", "pipeline"])
def test_bench_other_configs(config):
    d = _run("--config", config, "--no-extras", "--full")
    assert d["value"] > 0 and d["parity_prefix_bit_exact"] is True and 0 < d["roofline"]["frac"] < 1


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["2", "3"])
def test_bench_exchange_loop(config):
    d = _run("--force-exchange", "--no-cpu-baseline", "--config", config, "--full")
    assert d["value"] > 0 and "all-gather" in d["config"]["exchange"] and "shard_unpack" in d["kernel_ms"]
    if config == "2":   # the fused BPE encode writes the send wire itself
        assert "shard_pack" not in d["kernel_ms"] and "written by the encode itself" in d["config"]["exchange"]
    else:
        assert "shard_pack" in d["kernel_ms"]


@pytest.mark.gpu
def test_bench_exchange_loop_packed():
    d = _run("--force-exchange", "--no-cpu-baseline", "--wire", "0", "--exchange", "p2p", "--full")
    assert d["value"] > 0 and "shard_pack" in d["kernel_ms"] and "grouped direct" in d["config"]["exchange"]


def test_relaunch_argv():
    """`python bench.py --gpus N` without WORLD_SIZE runs N ranks under torch.distributed.run in a child process (CPU: the
    command only)."""
    sys.path.insert(0, str(ROOT))
    import bench
    argv = bench.relaunch_argv(8, ["--gpus", "8", "--steps", "20", "--warmup", "5"], port=29611)
    assert argv[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in argv and "--nproc-per-node=8" in argv
    assert argv[argv.index("--master-addr") + 1] == "127.0.0.1" and argv[argv.index("--master-port") + 1] == "29611"
    k = argv.index(str(ROOT / "bench.py"))
    assert argv[k + 1:] == ["--gpus", "8", "--steps", "20", "--warmup", "5"]


def test_gpus_must_match_world_size():
    """Launched as 2 ranks but told --gpus 1 (or the reverse): refuse before touching a GPU."""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1"], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode != 0 and "must agree" in p.stderr


@pytest.mark.gpu
def test_bench_through_the_relaunch():
    """--spawn: the path `--gpus N` takes (a child process under torch.distributed.run), with one rank and its RCCL group."""
    d = _run("--spawn", "--force-exchange", "--no-cpu-baseline", "--no-extras")
    assert d["n_gpus"] == 1 and d["value"] > 0 and "all-gather" in d["config"]["exchange"]
    assert d["config"]["world"] == {"ranks": 1, "launched_by": "torch.distributed.run"}
