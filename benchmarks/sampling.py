"""Token sampling on the device (warm-up, windows of at least `min_ms`, the best of three; the sampler and baseline (a) timed in
alternation in one process, baseline (b) in a child process of its own, before the parent opens the device):

  shapes    (rows, V) in (1, 32000), (8, 32000), (64, 32000) - staged in LDS - and (8, 128256) - re-read from memory; rows at stride V
  modes     greedy; top-k 50; top-p 0.9; both (temperature 1 for the three drawing modes)
  sampler   `nk_sample_fwd` through the C ABI: `device_ms` by HIP events on the compute stream (the call as a generation loop issues
            it: nothing waits for it), and `device_read_ms`, the wall time of the call plus the read of the `rows` ids by the host -
            the form that compares with baseline (a), which cannot avoid the host
  (a)       what the generation loop did before: a device-to-host copy of the (rows, V) logits and NumPy `argmax(axis=1)`; wall time.
            It is greedy whatever the mode.
  (b)       the torch-ROCm composition on the same device (`topk` and a mask, `softmax`, `sort` + `cumsum` for top-p, `multinomial`;
            `argmax` for greedy), by torch's events on its stream; null when torch does not see the device.  The child process
            (`--torch-worker`) imports torch and nothing of this project: the torch wheel carries its own HIP and HSA runtime next to the
            one the library links, and a process that has loaded both aborts in the C runtime's exit handlers (double free)

    python benchmarks/sampling.py [--min-ms 25] [--out profiles/r18_sampling.jsonl]
One JSON line per (shape, mode), printed and written to `--out`.  There is no pass / fail threshold."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1, 32000), (8, 32000), (64, 32000), (8, 128256))
MODES = (("greedy", 0.0, 0, 1.0), ("top_k_50", 1.0, 50, 1.0), ("top_p_0.9", 1.0, 0, 0.9), ("top_k_50_top_p_0.9", 1.0, 50, 0.9))


def logits_of(rng, rows, V):
    return (rng.standard_normal((rows, V)) * 3).astype(np.float32)      # the spread of a language model's logits


def window(timer, fn, min_ms):
    calls, ms = 2, timer(fn, 2)                                          # warm-up and a first estimate
    while ms * calls < min_ms and calls < (1 << 20):
        calls *= 2
        ms = timer(fn, calls)
    return timer(fn, max(4, int(min_ms / max(ms, 1e-4)) + 1))


def torch_worker(min_ms):
    """baseline (b): prints one JSON object, "rows,V,mode" -> the best of three windows in ms, or {} when torch sees no device"""
    try:
        import torch
    except ImportError:
        print(json.dumps({}))
        return
    if not torch.cuda.is_available():
        print(json.dumps({}))
        return

    def torch_events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / iters

    def sampler(x, temperature, k, p):
        if temperature == 0:
            return lambda: x.argmax(dim=-1)

        def draw():
            z = x / temperature
            if k:
                z = z.masked_fill(z < torch.topk(z, k, dim=-1).values[:, -1:], float("-inf"))
            probs = torch.softmax(z, dim=-1)
            if p < 1:
                sp, si = torch.sort(probs, dim=-1, descending=True)
                sp = sp.masked_fill(sp.cumsum(dim=-1) - sp >= p, 0.0)    # keep the smallest prefix whose mass reaches p
                probs = torch.zeros_like(probs).scatter(-1, si, sp)
            return torch.multinomial(probs, 1)
        return draw

    rng = np.random.default_rng(0)
    out = {}
    for rows, V in SHAPES:
        x = torch.from_numpy(logits_of(rng, rows, V)).cuda()
        for name, temperature, k, p in MODES:
            fn = sampler(x, temperature, k, p)
            out["%d,%d,%s" % (rows, V, name)] = round(min(window(torch_events, fn, min_ms) for _ in range(3)), 5)
    torch.cuda.synchronize()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-ms", type=float, default=25.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_sampling.jsonl"))
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--torch-worker", action="store_true", help="internal: run baseline (b) alone and print its times")
    args = ap.parse_args()
    if args.torch_worker:
        return torch_worker(args.min_ms)

    torch_ms = {}
    if not args.skip_torch:                                              # a fresh process, finished before this one opens the device
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-worker", "--min-ms", str(args.min_ms)], capture_output=True,
                           text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("the torch baseline failed:\n" + r.stderr[-2000:])
        torch_ms = json.loads(r.stdout.strip().splitlines()[-1])

    from neuronika_amd import capi as c
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/sampling.py needs a GPU")
    dev = c.Device(0)
    rows_out = []

    def emit(row):
        rows_out.append(row)
        print(json.dumps(row), flush=True)

    def events(fn, iters):
        e0, e1 = dev.event(), dev.event()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record(); e1.sync()
        return e0.elapsed_ms(e1) / iters

    def wall(fn, iters):                                                 # fn ends with the host holding its result
        dev.sync()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        return (time.perf_counter() - t0) * 1e3 / iters

    rng = np.random.default_rng(0)
    for rows, V in SHAPES:
        host = logits_of(rng, rows, V)
        X, IDS = dev.array(host), dev.zeros((rows,))
        d2h = lambda: X.numpy().argmax(axis=1)
        for name, temperature, k, p in MODES:
            offset = [0]

            def sample():
                c.sample_fwd(dev, X, V, rows, V, IDS, temperature, k, p, 1, offset[0])
                offset[0] += 1

            def sample_read():
                sample()
                return IDS.numpy()
            tb = torch_ms.get("%d,%d,%s" % (rows, V, name))
            ms_s, ms_r, ms_a = [], [], []
            for _ in range(3):
                ms_s.append(window(events, sample, args.min_ms)); ms_r.append(window(wall, sample_read, args.min_ms))
                ms_a.append(window(wall, d2h, args.min_ms))
            emit({"bench": "sampling", "rows": rows, "V": V, "staged": V <= c.sample_stage_limit(), "mode": name, "temperature": temperature,
                  "top_k": k, "top_p": p, "device_ms": round(min(ms_s), 5), "device_windows": [round(v, 5) for v in ms_s],
                  "device_read_ms": round(min(ms_r), 5), "d2h_argmax_ms": round(min(ms_a), 5), "d2h_argmax_windows": [round(v, 5) for v in ms_a],
                  "torch_ms": tb, "logit_bytes": rows * V * 4,
                  "device_read_over_d2h_argmax": round(min(ms_r) / min(ms_a), 3),
                  "device_over_torch": round(min(ms_s) / tb, 3) if tb else None})
        del X, IDS
    dev.sync()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows_out:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
