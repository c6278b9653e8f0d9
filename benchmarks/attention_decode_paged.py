"""Paged decode against its contiguous twin, HIP events on the compute stream (warm-up, windows of at least `min_ms`, three windows
per contender, interleaved), all in ONE process on one device; written after benchmarks/attention_decode_gqa.py.

  kernels (through the C ABI), T = 1, dh = 128 (chunk C = 128), H = 32 query heads over Hkv = 8:
    B = 32 at n = 1024 and n = 8192 cached keys per sample; B = 1 at n = 32768.
  Per point and page size in {16, 64, 128, 1024}, timed in alternation:
    twin      nk_attention_decode_gqa_fwd on the (B, Hkv, n, dh) cache - the kernel whose body the paged one shares, and the yardstick:
              its machine code is the parent's (profiles/attention_decode_paged_isa.md)
    ordered   nk_attention_decode_paged_fwd, table[b][i] = b * max_pages + i: the pool is the contiguous cache, page by page
    shuffled  the same with the pool's pages in a random permutation
  `twin_spread` = (max - min) / min over the twin's three windows: a paged time inside it is not distinguishable from the twin.
  `ratio_*` = paged_ms / twin_ms at the best window of each.

    python benchmarks/attention_decode_paged.py [--min-ms 25] [--out profiles/attention_decode_paged.jsonl]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_decode_paged.jsonl"))
    ap.add_argument("--pages", type=int, nargs="*", default=[16, 64, 128, 1024])
    args = ap.parse_args()

    from neuronika_amd import capi as c
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/attention_decode_paged.py needs a GPU")
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

    H, Hkv, dh = 32, 8, 128
    d, scale, chunk = H * dh, float(np.float32(1.0 / np.sqrt(dh))), c.attention_decode_chunk(dh)
    for B, n in ((32, 1024), (32, 8192), (1, 32768)):
        nbytes = 2 * B * Hkv * n * dh * 4
        Kc, Vc = dev.full((B, Hkv, n, dh), 0.01), dev.full((B, Hkv, n, dh), 0.02)      # the cache, and the pool of every page size
        q = dev.array(np.random.default_rng(0).random((B, d), dtype=np.float32) - np.float32(0.5))
        start = dev.int_array(np.full(B, n - 1, dtype=np.int32))
        out = dev.zeros((B, d))
        ws = dev.zeros((c.attention_decode_workspace(B, 1, H, dh, n),))
        twin = lambda: c.attention_decode_gqa_fwd(dev, q, d, Kc, Vc, start, out, ws, B, 1, H, Hkv, dh, n, scale)
        for page in args.pages:
            max_pages = n // page
            num_pages = B * max_pages
            ordered = np.arange(num_pages, dtype=np.int32).reshape(B, max_pages)
            shuffled = np.random.default_rng(1).permutation(num_pages).astype(np.int32).reshape(B, max_pages)
            tabs = {"ordered": dev.int_array(ordered), "shuffled": dev.int_array(shuffled)}
            assert c.attention_decode_paged_workspace(B, 1, H, dh, max_pages, page, 0) == ws.size
            fns = {"twin": twin}
            for name, tab in tabs.items():
                fns[name] = (lambda tab: lambda: c.attention_decode_paged_fwd(dev, q, d, Kc, Vc, start, tab, max_pages, out, ws, B, 1, H, Hkv, dh,
                                                                              page, num_pages, 0, scale))(tab)
            ms = {k: [] for k in fns}
            for _ in range(3):
                for name, fn in fns.items():
                    ms[name].append(window(fn))
            t, o, s = (min(ms[k]) for k in ("twin", "ordered", "shuffled"))
            emit({"bench": "attention_decode_paged", "B": B, "H": H, "Hkv": Hkv, "dh": dh, "n": n, "T": 1, "chunk": chunk, "page": page,
                  "pages_per_chunk": max(1, chunk // page), "bytes": nbytes, "twin_ms": round(t, 5), "twin_windows": [round(v, 5) for v in ms["twin"]],
                  "twin_spread": round((max(ms["twin"]) - t) / t, 4), "ordered_ms": round(o, 5),
                  "ordered_windows": [round(v, 5) for v in ms["ordered"]], "shuffled_ms": round(s, 5),
                  "shuffled_windows": [round(v, 5) for v in ms["shuffled"]], "ratio_ordered": round(o / t, 4), "ratio_shuffled": round(s / t, 4),
                  "twin_GBps": round(nbytes / (t * 1e-3) / 1e9, 1), "ordered_GBps": round(nbytes / (o * 1e-3) / 1e9, 1),
                  "shuffled_GBps": round(nbytes / (s * 1e-3) / 1e9, 1)})
            del tabs, fns
        del Kc, Vc, q, start, out, ws
    dev.sync()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
