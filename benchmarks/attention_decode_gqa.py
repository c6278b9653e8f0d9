"""Grouped-query decode, HIP events on the compute stream (warm-up, windows of at least `min_ms`, the best of three), all in ONE process
on one device; written after benchmarks/attention_decode.py.

  kernels (through the C ABI), T = 1, cap = n, dh in {64, 128}, n in {128, 1024, 4096, 16384} cached keys, B*H in {64, 512} with H = 16
  query heads and G = H / Hkv in {1, 2, 4, 8}, plus one multi-query point H = 32, Hkv = 1.  Timed in alternation per point:
    gqa        nk_attention_decode_gqa_fwd on the (B, Hkv, n, dh) caches: the query heads of a group share one read of their chunk
    ungrouped  nk_attention_decode_fwd with the same B, H on a (B, H, n, dh) cache - what a layer without kv_heads runs, and what the
               grouped call must beat: G times the bytes
    copy       nk_copy of the bytes the grouped call has to read, 2 * B * Hkv * n * dh * 4 (half read, half written)
    launch     the ungrouped call with every start at -1: the same launches and grids, every block returns at once.  A point is
               `launch_bound` when ungrouped_ms <= 1.5 * launch_ms.
    `speedup` = ungrouped_ms / gqa_ms (G at best); `fraction_of_copy_rate` = (bytes / gqa_ms) over (bytes / copy_ms).
  module (through the tape), d_model = 1024, H = 16, B = 8, prefilled 1024: the forward() of one forward_step node, replayed, at
  Hkv = 16, 4 and 1, with the bytes of the layer's caches.

    python benchmarks/attention_decode_gqa.py [--min-ms 25] [--out profiles/r21_attention_decode_gqa.jsonl]
One JSON line per measurement, printed and written to `--out`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-ms", type=float, default=25.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_attention_decode_gqa.jsonl"))
    ap.add_argument("--problems", type=int, nargs="*", default=[64, 512], help="B*H values")
    ap.add_argument("--lengths", type=int, nargs="*", default=[128, 1024, 4096, 16384])
    ap.add_argument("--head-sizes", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--skip-module", action="store_true")
    args = ap.parse_args()

    import neuronika_amd
    from neuronika_amd import capi as c
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/attention_decode_gqa.py needs a GPU")
    t = neuronika_amd.tape
    tdev = t.Device(0)
    dev = c.Device(handle=tdev.raw())
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

    # ---- kernels ------------------------------------------------------------------------------------------------------------------
    for dh in args.head_sizes:
        scale = float(np.float32(1.0 / np.sqrt(dh)))
        chunk = c.attention_decode_chunk(dh)
        for bh in args.problems:
            for n in args.lengths:
                # one allocation per (dh, B*H, n): the ungrouped cache; a grouped cache is its first B * Hkv * n * dh floats
                Kc, Vc = dev.full((bh, n, dh), 0.01), dev.full((bh, n, dh), 0.02)
                for H, Hkv in ((16, 16), (16, 8), (16, 4), (16, 2), (32, 1)):
                    B, G, d, cap = bh // H, H // Hkv, H * dh, n
                    nbytes = 2 * B * Hkv * n * dh * 4
                    q = dev.array(np.random.default_rng(0).random((B, d), dtype=np.float32) - np.float32(0.5))
                    start, none = dev.int_array(np.full(B, n - 1, dtype=np.int32)), dev.int_array(np.full(B, -1, dtype=np.int32))
                    out = dev.zeros((B, d))
                    ws = dev.zeros((c.attention_decode_workspace(B, 1, H, dh, cap),))
                    SRC, DST = dev.zeros((nbytes // 8,)), dev.zeros((nbytes // 8,))
                    copy = lambda: c.check(c.lib.nk_copy(dev.h, DST.p, SRC.p, nbytes // 8))
                    gqa = lambda: c.attention_decode_gqa_fwd(dev, q, d, Kc, Vc, start, out, ws, B, 1, H, Hkv, dh, cap, scale)
                    ungrouped = lambda: c.attention_decode_fwd(dev, q, d, Kc, Vc, start, out, ws, B, 1, H, dh, cap, scale)
                    launch = lambda: c.attention_decode_fwd(dev, q, d, Kc, Vc, none, out, ws, B, 1, H, dh, cap, scale)
                    ms = {"gqa": [], "ungrouped": [], "copy": [], "launch": []}
                    for _ in range(3):
                        for name, fn in (("gqa", gqa), ("ungrouped", ungrouped), ("copy", copy), ("launch", launch)):
                            ms[name].append(window(fn))
                    g, u, cp, la = (min(ms[k]) for k in ("gqa", "ungrouped", "copy", "launch"))
                    emit({"bench": "attention_decode_gqa", "part": "kernels", "BH": bh, "B": B, "H": H, "Hkv": Hkv, "G": G, "n": n, "dh": dh,
                          "T": 1, "chunk": chunk, "blocks_gqa": B * Hkv * ((G + 7) // 8) * ((n + chunk - 1) // chunk),
                          "blocks_ungrouped": bh * ((n + chunk - 1) // chunk), "bytes_gqa": nbytes, "bytes_ungrouped": nbytes * G,
                          "gqa_ms": round(g, 5), "gqa_windows": [round(v, 5) for v in ms["gqa"]], "ungrouped_ms": round(u, 5),
                          "ungrouped_windows": [round(v, 5) for v in ms["ungrouped"]], "copy_ms": round(cp, 5), "launch_ms": round(la, 5),
                          "launch_bound": bool(u <= 1.5 * la), "speedup": round(u / g, 3), "gqa_GBps": round(nbytes / (g * 1e-3) / 1e9, 1),
                          "copy_GBps": round(nbytes / (cp * 1e-3) / 1e9, 1), "fraction_of_copy_rate": round(cp / g, 3)})
                    del q, start, none, out, ws, SRC, DST
                del Kc, Vc

    # ---- module -------------------------------------------------------------------------------------------------------------------
    if not args.skip_module:
        d, Hm, Bm, n0 = 1024, 16, 8, 1024
        rng = np.random.default_rng(1)
        prefix = (rng.random((Bm * (n0 + 1), d), dtype=np.float32) - np.float32(0.5))
        rows_of = lambda lo, hi: np.ascontiguousarray(np.concatenate([prefix[b * (n0 + 1) + lo:b * (n0 + 1) + hi] for b in range(Bm)]))
        nodes = {}
        for Hkv in (16, 4, 1):
            mha = t.nn.MultiheadAttention(tdev, d, Hm, 0.0, 3, kv_heads=Hkv)
            mha.causal = True
            mha.drop.eval()
            cache = t.nn.KvCache(tdev, Bm, Hkv, d // Hm, n0 + 8)
            y = mha.forward_step(t.from_ndarray(tdev, rows_of(0, n0)), Bm, cache)
            y.forward()
            nodes[Hkv] = (mha, cache, mha.forward_step(t.from_ndarray(tdev, rows_of(n0, n0 + 1)), Bm, cache))   # the node of token 1025
        ms = {Hkv: [] for Hkv in nodes}
        for _ in range(3):
            for Hkv, (_, _, step) in nodes.items():
                ms[Hkv].append(window(step.forward))
        for Hkv, (_, cache, _) in nodes.items():
            emit({"bench": "attention_decode_gqa", "part": "module", "d_model": d, "heads": Hm, "kv_heads": Hkv, "batch": Bm, "prefilled": n0,
                  "forward_step_ms": round(min(ms[Hkv]), 4), "forward_step_windows": [round(v, 4) for v in ms[Hkv]],
                  "tokens_per_s": round(Bm / (min(ms[Hkv]) * 1e-3), 1),
                  "cache_bytes": 2 * cache.batch * cache.heads * cache.capacity * cache.head_dim * 4,
                  "projection_rows": d + 2 * (d // Hm) * Hkv})
    dev.sync()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
