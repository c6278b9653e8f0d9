"""Sliding-window decode, HIP events on the compute stream (warm-up, windows of at least `min_ms`), all in ONE process on one device;
written after benchmarks/attention_decode_gqa.py.  The claim under test: the time of a windowed step is a function of min(n, W), not
of the length n of the generation or of the capacity of the cache.

  kernels (through the C ABI), T = 1, W = 4096, dh in {64, 128}, B*H in {64, 512} with H = 16 query heads and G = H / Hkv in
  {1, 4, 8}.  Per point, timed in alternation, `repeats` windows each:
    comparator  nk_attention_decode_gqa_fwd at n = W on a cache of capacity W: the parent's code on the same bytes.  Its own
                run-to-run spread s = max - min over its windows is measured first-hand, by repeating it.
    window      nk_attention_decode_window_fwd at n in {W, 4W, 16W}, on a LINEAR cache of capacity 16W and on a RING of capacity W
                (the comparator's buffers).  `within_2s` = median(window) <= median(comparator) + 2 s at all six.  `tight`: the
                same call at n = W on the comparator's buffers as a linear cache of capacity W (reported, not judged).
    unwindowed  nk_attention_decode_gqa_fwd at n = 16W on the linear cache: what a layer without a window pays at that length;
                `headline_ratio` = unwindowed_ms / window_ms at n = 16W on the ring.
    launch      the comparator with every start at -1: the same launches and grids, every block returns at once.  A point is
                `launch_bound` when comparator_ms <= 1.5 * launch_ms; such points are reported, not judged.
    GB/s        from the bytes the window needs: 2 * min(n, W) * dh * 4 per kv head and row.

    python benchmarks/attention_decode_window.py [--min-ms 25] [--out profiles/r22_attention_decode_window.jsonl]
One JSON line per point, printed and written to `--out`."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-ms", type=float, default=25.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_attention_decode_window.jsonl"))
    ap.add_argument("--problems", type=int, nargs="*", default=[64, 512], help="B*H values")
    ap.add_argument("--groups", type=int, nargs="*", default=[1, 4, 8], help="H / Hkv values")
    ap.add_argument("--head-sizes", type=int, nargs="*", default=[64, 128])
    args = ap.parse_args()

    from neuronika_amd import capi as c
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/attention_decode_window.py needs a GPU")
    dev = c.Device(0)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def timed(fn, iters):
        e0, e1 = dev.event(), dev.event()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record(); e1.sync()
        return e0.elapsed_ms(e1) / iters

    def window(fn):
        calls, ms = 2, timed(fn, 2)                                      # warm-up and a first estimate
        while ms * calls < args.min_ms and calls < (1 << 20):
            calls *= 2
            ms = timed(fn, calls)
        return timed(fn, max(4, int(args.min_ms / max(ms, 1e-4)) + 1))

    W, H, T = args.window, 16, 1
    lengths = [W, 4 * W, 16 * W]
    long_cap = lengths[-1]
    for dh in args.head_sizes:
        scale = float(np.float32(1.0 / np.sqrt(dh)))
        chunk = c.attention_decode_chunk(dh)
        for bh in args.problems:
            for G in args.groups:
                B, Hkv, d = bh // H, H // G, H * dh
                nbytes = 2 * B * Hkv * W * dh * 4
                Kl, Vl = dev.full((B, Hkv, long_cap, dh), 0.01), dev.full((B, Hkv, long_cap, dh), 0.02)      # linear, capacity 16W
                Kr, Vr = dev.full((B, Hkv, W, dh), 0.01), dev.full((B, Hkv, W, dh), 0.02)                    # capacity W: comparator and ring
                q = dev.array(np.random.default_rng(0).random((B, d), dtype=np.float32) - np.float32(0.5))
                out = dev.zeros((B, d))
                ws = dev.zeros((max(c.attention_decode_workspace(B, T, H, dh, long_cap), c.attention_decode_window_workspace(B, T, H, dh, W)),))
                starts = {n: dev.int_array(np.full(B, n - 1, dtype=np.int32)) for n in lengths}
                none = dev.int_array(np.full(B, -1, dtype=np.int32))
                calls = {"comparator": lambda: c.attention_decode_gqa_fwd(dev, q, d, Kr, Vr, starts[W], out, ws, B, T, H, Hkv, dh, W, scale),
                         "launch": lambda: c.attention_decode_gqa_fwd(dev, q, d, Kr, Vr, none, out, ws, B, T, H, Hkv, dh, W, scale),
                         "unwindowed": lambda: c.attention_decode_gqa_fwd(dev, q, d, Kl, Vl, starts[long_cap], out, ws, B, T, H, Hkv, dh, long_cap, scale)}
                for n in lengths:
                    calls["linear n=%d" % n] = (lambda n=n: c.attention_decode_window_fwd(dev, q, d, Kl, Vl, starts[n], out, ws, B, T, H, Hkv, dh,
                                                                                         long_cap, W, 0, scale))
                    calls["ring n=%d" % n] = (lambda n=n: c.attention_decode_window_fwd(dev, q, d, Kr, Vr, starts[n], out, ws, B, T, H, Hkv, dh,
                                                                                       W, W, 1, scale))
                # the window kernel on the comparator's own buffers as a LINEAR cache of capacity W: the kernel alone, without the
                # sixteen times larger address range of the long cache
                calls["tight n=%d" % W] = lambda: c.attention_decode_window_fwd(dev, q, d, Kr, Vr, starts[W], out, ws, B, T, H, Hkv, dh, W, W, 0, scale)
                ms = {name: [] for name in calls}
                for _ in range(args.repeats):                            # the comparator between every two windowed calls
                    for name, fn in calls.items():
                        if name != "comparator":
                            ms["comparator"].append(window(calls["comparator"]))
                            ms[name].append(window(fn))
                med = {name: statistics.median(v) for name, v in ms.items()}
                comp, s = med["comparator"], max(ms["comparator"]) - min(ms["comparator"])
                launch_bound = bool(comp <= 1.5 * med["launch"])
                row = {"bench": "attention_decode_window", "BH": bh, "B": B, "H": H, "Hkv": Hkv, "G": G, "dh": dh, "T": T, "W": W, "chunk": chunk,
                       "bytes": nbytes, "comparator_ms": round(comp, 5), "comparator_spread_ms": round(s, 5),
                       "comparator_windows": len(ms["comparator"]), "comparator_min_ms": round(min(ms["comparator"]), 5),
                       "comparator_max_ms": round(max(ms["comparator"]), 5), "comparator_GBps": round(nbytes / (comp * 1e-3) / 1e9, 1),
                       "launch_ms": round(med["launch"], 5), "launch_bound": launch_bound, "unwindowed_16W_ms": round(med["unwindowed"], 5),
                       "headline_ratio": round(med["unwindowed"] / med["ring n=%d" % long_cap], 2)}
                row["tight_1W_ms"] = round(med["tight n=%d" % W], 5)
                worst = 0.0
                for n in lengths:
                    for kind in ("linear", "ring"):
                        v = med["%s n=%d" % (kind, n)]
                        row["%s_%dW_ms" % (kind, n // W)] = round(v, 5)
                        row["%s_%dW_GBps" % (kind, n // W)] = round(nbytes / (v * 1e-3) / 1e9, 1)
                        worst = max(worst, v - comp)
                row["worst_excess_ms"] = round(worst, 5)
                row["within_2s"] = None if launch_bound else bool(worst <= 2 * s)    # launch-bound points are reported, not judged
                emit(row)
                del Kl, Vl, Kr, Vr, q, out, ws, starts, none, calls
    dev.sync()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
