"""`bench.py --dump-outputs DIR`: what the last timed step computed, as DIR/<name>.npy - bounded in size, f32 / f64 only,
a function of the arguments alone (the untimed steps, whose number follows the clock, must not show in it) and of
`--steps` in particular."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench():
    spec = importlib.util.spec_from_file_location("nk_bench", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_sample_index_is_fixed_sorted_and_in_range():
    b = _bench()
    size = 3 * b.DUMP_SAMPLE + 5
    i0, i1 = b.dump_sample_index(size), b.dump_sample_index(size)
    assert np.array_equal(i0, i1)
    assert i0.shape == (b.DUMP_SAMPLE,) and i0.min() >= 0 and i0.max() < size
    assert np.all(np.diff(i0) > 0)                              # ascending, no element twice
    assert not np.array_equal(i0, np.arange(b.DUMP_SAMPLE))     # a sample of the whole array, not its head


def test_dump_outputs_writes_float_arrays_whole_or_sampled(tmp_path):
    b = _bench()
    rng = np.random.default_rng(0)
    big = rng.random((2, b.DUMP_SAMPLE + 7), dtype=np.float32)
    arrays = {"small": rng.random((3, 5), dtype=np.float32), "double": rng.random(4), "count": np.arange(6).reshape(2, 3),
              "big": big, "big_t": np.asfortranarray(big)}
    d = b.dump_outputs(str(tmp_path / "out"), arrays)
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == sorted(n + ".npy" for n in arrays)
    got = {n: np.load(tmp_path / "out" / (n + ".npy")) for n in arrays}
    assert all(g.dtype in (np.float32, np.float64) for g in got.values())
    assert np.array_equal(got["small"], arrays["small"]) and got["small"].dtype == np.float32
    assert np.array_equal(got["double"], arrays["double"]) and got["double"].dtype == np.float64
    assert np.array_equal(got["count"], arrays["count"].astype(np.float64))
    idx = b.dump_sample_index(big.size)
    assert np.array_equal(got["big"], big.reshape(-1)[idx])
    assert np.array_equal(got["big_t"], got["big"])            # the sample is of the C-order flattening, whatever the layout
    assert d["bytes"] == sum(g.nbytes for g in got.values()) <= b.DUMP_MAX_BYTES
    assert d["arrays"]["big"] == {"shape": [2, b.DUMP_SAMPLE + 7], "dtype": "float32", "sampled": True, "elements_written": b.DUMP_SAMPLE}
    assert d["arrays"]["small"]["sampled"] is False and d["arrays"]["small"]["elements_written"] == 15
    json.dumps(d)                                               # goes into the result line


def test_dump_outputs_refuses_to_pass_its_bound(tmp_path):
    b = _bench()
    b.DUMP_MAX_BYTES = 100
    with pytest.raises(SystemExit):
        b.dump_outputs(str(tmp_path), {"a": np.zeros(20, np.float32), "b": np.zeros(20, np.float32)})


def test_the_default_workload_budget_holds():
    """What run_mlp dumps at ANY --hidden / --batch: seven matrices (output, three intermediate gradients, three weights),
    three bias vectors and the loss, none stored with more than DUMP_SAMPLE f32 elements - inside the bound by construction."""
    b = _bench()
    assert 7 * 4 * b.DUMP_SAMPLE + 4 * (3 * b.DUMP_SAMPLE + 1) <= b.DUMP_MAX_BYTES


@pytest.mark.parametrize("argv", [["--workload", "conv"], ["--workload", "matmul"], ["--workload", "mha"], ["--steps", "0"]])
def test_dump_outputs_is_refused_where_it_is_not_defined(tmp_path, argv):
    r = subprocess.run([sys.executable, BENCH, "--dump-outputs", str(tmp_path / "d"), *argv], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr
    assert not (tmp_path / "d").exists()


def _run(tmp_path, name, steps, warmup):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / name
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--hidden", "512",
                        "--batch", "384", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return line, {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}


@pytest.mark.gpu
def test_dump_is_a_function_of_the_arguments_and_follows_steps(tmp_path):
    line, a = _run(tmp_path, "a", 3, 2)
    assert line["steps"] == 3 and line["dumped_outputs"]["of_timed_step"] == 3
    assert sorted(a) == sorted(line["dumped_outputs"]["arrays"])
    assert {"loss", "output", "output_grad", "hidden1_grad", "hidden2_grad", "linear0_weight", "linear2_bias"} <= set(a)
    for name, v in a.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), name
        assert np.count_nonzero(v) > 0, name                   # every array carries what the step computed, none is a blank buffer
    assert a["output"].size == 384 * 512 and a["linear1_weight"].size == 512 * 512      # under DUMP_SAMPLE elements: whole
    assert float(a["loss"][0]) == pytest.approx(line["loss"], rel=1e-6)
    _, b = _run(tmp_path, "b", 3, 2)                            # the same arguments: the same bits
    assert all(np.array_equal(a[k], b[k]) for k in a)
    _, c = _run(tmp_path, "c", 3, 7)                            # more untimed steps: still the same bits
    assert all(np.array_equal(a[k], c[k]) for k in a)
    _, d = _run(tmp_path, "d", 4, 2)                            # one more TIMED step: one more SGD update behind the last step
    assert not np.array_equal(a["linear2_weight"], d["linear2_weight"])
    assert not np.array_equal(a["output"], d["output"])
