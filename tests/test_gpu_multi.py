"""Multi-GPU execution of the PRODUCT path (one process per GPU, RCCL over xGMI), skipped on a box with fewer than
two GPUs: `bench.py --gpus 2` self-spawned, and the data-parallel algebra of SURVEY.md section 8e with the tape,
`dp::GradientSync` and RCCL doing the work - per-rank `backward(1/p)` on a batch shard + overlapped sum all-reduce
== the full-batch gradient of a single rank (what tests/test_dp_cpu.py checks with the oracle over gloo).

Insertion point in the reference: between `VarDiff::backward` (neuronika-variable/src/vardiff.rs:125-141) and
`Optimizer::step` (neuronika-optim/src/optimizer.rs:81-86)."""
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ngpu():
    from neuronika_amd import capi
    return capi.device_count()


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def test_bench_refuses_more_ranks_than_gpus():
    """`--gpus N` on a node with fewer GPUs must fail, never report a smaller job under the requested label."""
    n = _ngpu() + 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "refusing" in r.stderr and r.stdout.strip() == ""


@pytest.mark.skipif(_ngpu() < 2, reason="needs two GPUs")
def test_bench_self_spawns_two_ranks():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1",
                        "--hidden", "1024", "--batch", "512", "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["n_gpus"] == 2 and res["rccl_ranks"] == 2
    assert res["config"]["global_batch"] == 1024
    assert res["allreduce_bytes_per_step"] == 3 * (1024 * 1024 + 1024) * 4
    assert np.isfinite(res["loss"]) and res["value"] > 0


_WORKER = r"""
import os, sys
import numpy as np
sys.path.insert(0, {root!r})
import neuronika_amd
from neuronika_amd.rendezvous import Rendezvous
t = neuronika_amd.tape
rv = Rendezvous()
rank, world = rv.rank, rv.world
dev = t.Device(rv.local)
H, B = {hidden}, {batch}                       # B rows per rank
rng = np.random.default_rng(7)
x = rng.random((B * world, H), dtype=np.float32)
tg = rng.random((B * world, H), dtype=np.float32)

def build(xs, ts):
    lins = [t.nn.Linear(dev, H, H, s) for s in (1, 3, 5)]          # identical weights on every rank
    out = lins[2].forward(lins[1].forward(lins[0].forward(t.from_ndarray(dev, xs)).relu()).relu())
    loss = out.mse(t.from_ndarray(dev, ts), t.Reduction.Mean)
    return loss, [p for l in lins for p in (l.weight, l.bias)]

uid = rv.broadcast(t.dp.Communicator.unique_id() if rank == 0 else None)
comm = t.dp.Communicator(dev, world, rank, uid)
assert comm.size == world
sl = slice(rank * B, (rank + 1) * B)
loss, params = build(x[sl], tg[sl])
sync = t.dp.GradientSync(comm, params)
worst = 0.0
for rep in range(2):                                  # second pass: re-armed events, recycled buffers
    for p in params: p.zero_grad()
    loss.forward(); loss.no_grad(); loss.with_grad()
    loss.backward_sync(1.0 / world, sync); sync.join()
    got = [p.grad().copy() for p in params]
    full, fparams = build(x, tg)                      # single-rank full-batch reference on this GPU
    full.forward(); full.backward(1.0)
    for g, fp in zip(got, fparams):
        w = fp.grad()
        err = float(np.abs(g - w).max() / (np.abs(w).max() + 1e-30))
        worst = max(worst, err)
assert sync.elements_exchanged() == 2 * sum(int(np.prod(p.shape)) for p in params)
mx = rv.max(worst)
rv.barrier()
dev.sync()
if rank == 0:
    print("WORST", mx, flush=True)
rv.close()
"""


@pytest.mark.skipif(_ngpu() < 2, reason="needs two GPUs")
@pytest.mark.parametrize("hidden,batch", [(4096, 256), (640, 96)])   # piecewise weight gradients / small unsplit ones
def test_two_rank_gradient_sync_equals_full_batch(tmp_path, hidden, batch):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, hidden=hidden, batch=batch))
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), NK_RV_SECRET="t",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=600) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-1500:] for o in outs]
    worst = float([l for l in outs[0][0].splitlines() if l.startswith("WORST")][-1].split()[1])
    assert worst < 2e-5, worst       # f32 sums in a different order (two shards of B rows vs one pass over 2B rows)


def _bench_line(args, env_extra=None, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "NCCL_DEBUG")}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]), r.stderr


def test_bench_plain_run_does_only_what_its_headline_needs():
    """`bench.py --gpus 1 --steps K --warmup W` with nothing else: set-up, warm-up, the K timed steps, the line - the headline
    fields and the roofline the timed steps leave behind, none of the records that take runs of their own (`--full`), and
    at most 30 s of the whole run, process start to exit, outside its steps."""
    steps, warmup = 3, 1
    t0 = time.perf_counter()
    res, _ = _bench_line(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)])
    outside = time.perf_counter() - t0 - (steps + warmup) * res["ms_per_step"] * 1e-3
    assert res["metric"] == "training-step samples/sec (fwd+bwd+allreduce)" and res["unit"] == "samples/s"
    assert res["higher_is_better"] is True and res["dtype"] == "f32" and res["n_gpus"] == 1 and res["steps"] == steps
    assert res["ms_per_step"] > 0 and res["value"] == pytest.approx(4096 * 1e3 / res["ms_per_step"], rel=1e-3)
    assert res["roofline"]["frac"] > 0 and res["roofline"]["launches"] > 0 and np.isfinite(res["loss"])
    moved = [k for k in res if k.startswith("matmul_") or k in ("conv_c3", "mha_c5", "hbm_kernels", "cpu_baseline", "allreduce_alone",
                                                                "gemm_contention", "rccl")]
    assert moved == []
    assert outside < 30.0, outside


def test_bench_default_line_carries_every_baseline_config():
    """The ONE `--full` record holds all headline numbers: C4 at the top level, C2 at 1024 / 2048 / 4096 / 8192,
    C3 and C5 as sub-records of the same shape (value, ms_per_step, roofline{achieved, frac, launches, avg_launch_ms})."""
    res, _ = _bench_line(["--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline"])
    assert res["n_gpus"] == 1 and res["roofline"]["frac"] > 0 and res["roofline"]["traffic_measured_at_commit"]
    for key, unit in [("matmul_1024", "TFLOP/s"), ("matmul_2048", "TFLOP/s"), ("matmul_4096", "TFLOP/s"), ("matmul_8192", "TFLOP/s"),
                      ("conv_c3", "samples/s"), ("mha_c5", "sequences/s")]:
        rec = res[key]
        assert rec["unit"] == unit and rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["steps"] == 20, key
        roof = rec["roofline"]
        # every `frac` of the line is a fraction of a roofline: below 1.  (C3 with the Winograd kernels: on the MFMA flops the launches
        # EXECUTE; the rate on the direct algorithmic flops - SURVEY.md 8d - stands beside it with the ratio as `algorithmic_speedup`)
        assert 0 < roof["frac"] < 1 and roof["launches"] > 0 and roof["avg_launch_ms"] > 0 and roof["achieved"] > 0, key
        if roof.get("winograd"):
            assert abs(roof["algorithmic_speedup"] - 2.25) < 1e-3 and roof["direct_equivalent_frac_of_peak"] > roof["frac"]
    assert res["matmul_4096"]["roofline"]["launches"] == 6 * 20       # K = 4096: every product as two chained launches
    hb = res["hbm_kernels"]
    assert hb["tensor_bytes"] == 1 << 30 and all(0 < k["frac"] < 1 for k in hb["kernels"].values())
    assert all(0 < c["frac_of_peak"] < 1 for c in hb["ceilings"].values())      # at 1 GiB per tensor nothing runs at or above the HBM peak
    assert res["conv_c3"]["roofline"]["launches"] == 3 * 20           # one launch record per conv pass
    att = res["mha_c5"]["attention_core"]
    assert att["launches"] == 2 * 20 and 0 < att["frac"] < 1


def test_bench_multi_rank_record_is_self_diagnosing():
    """Every line of bench.py's N > 1 path on ONE GPU: a one-rank RCCL communicator with the exchange forced on
    (NK_BENCH_FORCE_RCCL=1).  The record must carry the diagnostics the first real multi-GPU run will be tuned from and
    must not be readable as a measurement."""
    res, err = _bench_line(["--steps", "3", "--warmup", "1", "--hidden", "1024", "--batch", "512", "--full", "--no-cpu-baseline"],
                           {"NK_BENCH_FORCE_RCCL": "1", "NK_BENCH_VERBOSE": "1"})
    assert res["rccl_single_rank_debug"] is True and res["metric"].startswith("DEBUG RUN")
    assert res["rccl_ranks"] == 1 and res["allreduce_bytes_per_step"] == 3 * (1024 * 1024 + 1024) * 4
    assert res["allreduce_launches_per_step"] >= 4
    assert len(res["per_rank_device_ms_per_step"]) == 1 and res["per_rank_device_ms_min_max"][0] > 0
    alone = res["allreduce_alone"]
    assert alone["bytes"] == res["allreduce_bytes_per_step"] and alone["ms"] > 0 and len(alone["by_size"]) == 3
    g = res["gemm_contention"]
    # (3 steps of a 1024-wide model: 0.16 - 0.35 ms of GEMMs per step, the ratio of two such figures swings by a factor of two
    # between boxes - the record's SHAPE is what this test pins, tools/first_multi_gpu.sh measures)
    assert g["gemm_ms_per_step_overlapped"] > 0 and g["gemm_ms_per_step_no_exchange"] > 0 and 0.1 < g["slowdown"] < 10.0
    assert isinstance(res["exposed_comm_ms"], float)
    rccl = res["rccl"]
    assert "excerpt" in rccl, rccl                 # the NCCL_DEBUG=INFO log of rank 0 was found and parsed
    assert rccl["version"] or rccl["excerpt"], rccl
    assert "communicator up" in err and "timed loop done" in err      # progress markers


def test_replica_debug_run_is_not_readable_as_a_measurement():
    res, _ = _bench_line(["--steps", "2", "--warmup", "1", "--hidden", "1024", "--batch", "512", "--full", "--no-cpu-baseline"],
                         {"NK_BENCH_REPLICAS": "4"})
    assert res["metric"].startswith("DEBUG RUN") and res["exposed_comm_ms"] is None and res["replica_ranks_debug"] == 4


_THREAD_WORKER = """
def run(idx, out):
    # one host thread per GPU, each with its own device handle (the shape a Rust host takes: the graph is !Send,
    # neuronika-variable/src/utils.rs:9, so one thread owns one device's tape)
    import numpy as np
    from neuronika_amd import capi
    dev = capi.Device(idx)
    rng = np.random.default_rng(idx)
    a, b = rng.random((384, 256), dtype=np.float32), rng.random((256, 320), dtype=np.float32)
    A, B, Cm = dev.array(a), dev.array(b), dev.zeros((384, 320))
    for _ in range(50):
        capi.mm_fwd(dev, A, B, Cm)
    x = rng.random((64, 512), dtype=np.float32)
    Y = dev.zeros(x.shape)
    capi.softmax_fwd(dev, dev.array(x), Y, 1)
    try:                                          # an error on this thread's device must not show up on the other thread
        capi.softmax_fwd(dev, dev.array(x), Y, 7)
        out[idx] = "no error raised"
        return
    except capi.NeuronikaHipError as e:
        msg = str(e)
    out[idx] = (Cm.numpy(), a @ b, Y.numpy(), x, msg)
"""


@pytest.mark.skipif(_ngpu() < 2, reason="needs two GPUs")
def test_two_threads_drive_two_devices():
    """Thread-per-GPU use of the C ABI (thread-safe ACROSS devices): two host threads, one device handle
    each, concurrently; results per device are right and the thread-local error state does not leak."""
    import threading
    ns = {}
    exec(_THREAD_WORKER, ns)
    out = {}
    ths = [threading.Thread(target=ns["run"], args=(i, out)) for i in range(2)]
    [t.start() for t in ths]
    [t.join(300) for t in ths]
    for i in range(2):
        assert not isinstance(out.get(i), str), out.get(i)
        c, ref, y, x, msg = out[i]
        np.testing.assert_allclose(c, ref, rtol=2e-5)
        e = np.exp(x - x.max(1, keepdims=True))
        np.testing.assert_allclose(y, e / e.sum(1, keepdims=True), rtol=1e-5)
        assert "axis" in msg.lower() or msg


@pytest.mark.skipif(_ngpu() < 2, reason="needs two GPUs")
def test_comm_init_all_two_threads_all_reduce():
    """nk_comm_init_all (ncclCommInitAll): the communicators of both GPUs of one process, each driven by its own host thread;
    the sum all-reduce of rank-dependent data is the same on both and equals the host sum."""
    import threading
    from neuronika_amd import capi
    devs = [capi.Device(0), capi.Device(1)]
    comms = capi.Comm.init_all(devs)
    assert [c.size for c in comms] == [2, 2] and [c.rank for c in comms] == [0, 1]
    xs = [np.random.default_rng(40 + r).random(1 << 20, dtype=np.float32) for r in range(2)]
    out = {}

    def run(r):
        try:
            buf = devs[r].array(xs[r])
            comms[r].allreduce_sum_async(buf)
            comms[r].join()
            out[r] = buf.numpy()
        except Exception as e:                      # noqa: BLE001 - reported by the asserting thread
            out[r] = repr(e)
    ths = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in ths]
    [t.join(300) for t in ths]
    for r in range(2):
        assert not isinstance(out.get(r), str), out.get(r)
        assert np.array_equal(out[r], xs[0] + xs[1])
    [c.close() for c in comms]


def test_comm_init_all_single_device():
    """The same entry point with one device handle (runs on a 1-GPU box): a one-rank RCCL communicator, whose sum all-reduce is
    the identity; a device named twice is refused."""
    from neuronika_amd import capi
    dev = capi.Device(0)
    (comm,) = capi.Comm.init_all([dev])
    assert comm.size == 1 and comm.rank == 0
    x = np.random.default_rng(3).random(100003, dtype=np.float32)
    buf = dev.array(x)
    comm.allreduce_sum_async(buf); comm.join()
    assert np.array_equal(buf.numpy(), x)
    comm.close()
    with pytest.raises(capi.NeuronikaHipError, match="named twice"):
        capi.Comm.init_all([dev, capi.Device(0)])


def test_two_threads_share_one_gpu_through_two_handles():
    """The same thread-per-handle shape on a 1-GPU box: two handles (own streams, own workspace) of device 0 driven from
    two threads at once."""
    import threading
    ns = {}
    exec(_THREAD_WORKER.replace("capi.Device(idx)", "capi.Device(0)"), ns)
    out = {}
    ths = [threading.Thread(target=ns["run"], args=(i, out)) for i in range(2)]
    [t.start() for t in ths]
    [t.join(300) for t in ths]
    for i in range(2):
        assert not isinstance(out.get(i), str), out.get(i)
        c, ref, y, x, msg = out[i]
        np.testing.assert_allclose(c, ref, rtol=2e-5)
