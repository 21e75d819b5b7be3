"""bench.py's options around the headline figure: a plain run times the select and nothing else, `--full`
adds the legs that take runs of their own, and `--dump-outputs DIR` writes what the last timed step computed
(the decoded per-pod top-k keys) so that two builds can be compared on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA_LEGS = ("cycle", "replay", "replay_100k")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_options_default_off(monkeypatch):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_decodes_keys_exactly(tmp_path):
    """Totals and node indices are 32-bit fields of the key, so float64 holds them exactly; key 0 (no feasible
    node) is -1 in both arrays."""
    import bench
    from koordinator_amd import abi

    total = np.array([[0xFFFFFFFF, 7], [300, 0]], np.uint64)
    node = np.array([[0, 0xFFFFFFFE], [99_999, 0]], np.uint64)
    keys = (total << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - node)
    keys[1, 1] = 0
    out = tmp_path / "nested" / "dir"
    bench.dump_outputs(str(out), keys)
    assert sorted(os.listdir(out)) == ["select_node.npy", "select_total.npy"]
    t, n = np.load(out / "select_total.npy"), np.load(out / "select_node.npy")
    assert t.dtype == np.float64 and n.dtype == np.float64 and t.shape == n.shape == (2, 2)
    assert np.array_equal(t, [[0xFFFFFFFF, 7], [300, -1]])
    assert np.array_equal(n, [[0, 0xFFFFFFFE], [99_999, -1]])
    assert np.array_equal(t, abi.key_total(keys)) and np.array_equal(n, abi.key_node(keys))


@pytest.mark.gpu
def test_plain_run_times_only_the_select_and_dumps_its_result(tmp_path):
    """Config 1 (1k nodes x 500 pods): the line carries the headline figure over exactly --steps steps and none of
    the extra legs; the dumped arrays are the oracle's selectHost of the same seeded inputs."""
    import oracle_lib
    from koordinator_amd import abi, synth

    out = _bench("--config", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(500 * 1000 / (out["ms_per_step"] * 1e-3))
    assert out["unit"] == "evals/s" and out["higher_is_better"] is True and out["dtype"] == "int64"
    assert out["cpu_baseline"] is None and not any(leg in out for leg in EXTRA_LEGS)
    cfg, nodes, pods = synth.cluster(1)
    want = oracle_lib.select(cfg.kg_config(), nodes, pods, 1)
    t, n = np.load(tmp_path / "select_total.npy"), np.load(tmp_path / "select_node.npy")
    assert t.dtype == np.float64 and n.dtype == np.float64
    assert np.array_equal(t, abi.key_total(want)) and np.array_equal(n, abi.key_node(want))


@pytest.mark.gpu
def test_full_run_adds_the_extra_legs():
    """--full brings the cycle and the CPU baseline back (the replays, minutes of work at their sizes, are switched
    off here with their own option), next to the same headline keys."""
    out = _bench("--config", "1", "--steps", "3", "--warmup", "1", "--full", "--no-replay", "--cpu-seconds", "0.2")
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert out["cycle"]["ms_per_cycle"] > 0 and (out["cycle"]["pods"], out["cycle"]["nodes"]) == (500, 1000)
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["unit"] == "evals/s"
    assert "replay" not in out
