"""Packed sequences in the fused core (nk_attention_seg_fwd + _bwd), HIP events on the compute stream (warm-up, windows of at least
`min_ms`), all in ONE process on one device; written after benchmarks/attention_band.py.  Nobody had measured this: the expectation
to confirm or refute is that seg is about the band core at W = L, or faster - documents stop at their boundary instead of sliding, so
on average a row keeps about half the band's keys - and far below the causal core at the same S.

  core (through the C ABI), forward + backward, uniform documents of length L, dh in {64, 128}, S in {2048, 4096, 8192},
  L in {256, 512, 1024}, p in `--probs` (training), B * S = `tokens` rows of H heads.  Per point, timed in alternation, `repeats`
  windows each:
    causal    nk_attention_causal_fwd + _bwd at the same S: one document per sample; the kernels every one of these was copied
              from, unchanged.  Its own run-to-run spread max - min over its windows is reported next to every ratio.
    band      nk_attention_band_fwd + _bwd at W = L: the same scratch geometry, the same staged tiles, edges that slide.
    seg       nk_attention_seg_fwd + _bwd with lo[r] = L * (r // L), span = L.
    `seg_over_causal`, `seg_over_band` = ratios of the medians; `pairs_seg_over_band` = the (query, key) pairs each keeps.
    split     one profiled seg backward per class (nk_profile_*): the fused kernel against the per-strip dK / dV products.

    python benchmarks/attention_segments.py [--min-ms 100] [--out profiles/r24_attention_segments.jsonl]
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
    ap.add_argument("--min-ms", type=float, default=100.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=16384, help="B * S")
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--lengths", type=int, nargs="*", default=[2048, 4096, 8192])
    ap.add_argument("--documents", type=int, nargs="*", default=[256, 512, 1024])
    ap.add_argument("--head-sizes", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--probs", type=float, nargs="*", default=[0.0, 0.1])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_attention_segments.jsonl"))
    args = ap.parse_args()

    from neuronika_amd import capi as c
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/attention_segments.py needs a GPU")
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
        return timed(fn, max(2, int(args.min_ms / max(ms, 1e-4)) + 1))

    H = args.heads
    for dh in args.head_sizes:
        scale = float(np.float32(1.0 / np.sqrt(dh)))
        d = H * dh
        for S in args.lengths:
            B = max(1, args.tokens // S)
            BH, SP = B * H, c.attention_padded(S)
            rng = np.random.default_rng(0)
            Q, K, V, G = (dev.array(rng.random((B * S, d), dtype=np.float32) - np.float32(0.5)) for _ in range(4))
            out, stats = dev.zeros((B * S, d)), dev.zeros((BH, SP, 2))
            dQ, dK, dV = dev.zeros((B * S, d)), dev.zeros((B * S, d)), dev.zeros((B * S, d))
            cs, cds, cpd, cbits = dev.zeros((BH, SP, SP)), dev.zeros((BH, SP, SP)), dev.zeros((BH, SP, SP)), dev.zeros((BH, SP, SP // 32))
            for L in [n for n in args.documents if n < S]:
                ext, words = c.attention_band_scratch(S, L), c.attention_band_mask_words(S, L)
                bs, bds, bpd, bbits = dev.zeros((BH, ext)), dev.zeros((BH, ext)), dev.zeros((BH, ext)), dev.zeros((BH, words))
                lo = dev.int_array(np.tile((np.arange(S) // L * L).astype(np.int32), (B, 1)))
                for p in args.probs:
                    def causal_fwd():
                        c.attention_fwd(dev, Q, K, V, cs, stats, cbits, out, B, S, H, dh, scale, p, True, 1, 0, causal=True)

                    def causal_bwd():
                        c.attention_bwd(dev, dQ, dK, dV, cds, cpd, G, out, cs, stats, cbits, Q, K, V, B, S, H, dh, scale, p, True,
                                        assign=(True, True, True), causal=True)

                    def band_fwd():
                        c.attention_band_fwd(dev, Q, K, V, bs, stats, bbits, out, B, S, H, dh, scale, p, True, 1, 0, window=L)

                    def band_bwd():
                        c.attention_band_bwd(dev, dQ, dK, dV, bds, bpd, G, out, bs, stats, bbits, Q, K, V, B, S, H, dh, scale, p, True,
                                             assign=(True, True, True), window=L)

                    def seg_fwd():
                        c.attention_seg_fwd(dev, Q, K, V, lo, bs, stats, bbits, out, B, S, H, dh, scale, p, True, 1, 0, span=L)

                    def seg_bwd():
                        c.attention_seg_bwd(dev, dQ, dK, dV, bds, bpd, G, out, bs, stats, bbits, Q, K, V, lo, B, S, H, dh, scale, p, True,
                                            assign=(True, True, True), span=L)

                    # every class runs its own forward in front of its backward: the scratch the three share is always its own
                    calls = {"causal": lambda: (causal_fwd(), causal_bwd()), "band": lambda: (band_fwd(), band_bwd()),
                             "seg": lambda: (seg_fwd(), seg_bwd()), "band_fwd": band_fwd, "seg_fwd": seg_fwd}
                    ms = {name: [] for name in calls}
                    for _ in range(args.repeats):                        # interleaved: every window of one next to a window of the others
                        for name, fn in calls.items():
                            ms[name].append(window(fn))
                    med = {name: statistics.median(v) for name, v in ms.items()}
                    seg_fwd()                                            # the backward below reads the seg forward's state
                    split = {}
                    for klass, name in ((c.KERNEL_ATTENTION, "kernel"), (c.KERNEL_SGEMM, "strips")):
                        dev.profile_begin()
                        seg_bwd()
                        n, t, _ = dev.profile_end(klass)
                        split[name] = (n, t)
                    pairs_band = sum(min(r + 1, L) for r in range(S))
                    pairs_seg = sum(r % L + 1 for r in range(S))
                    spread = lambda name: round(max(ms[name]) - min(ms[name]), 4)
                    emit({"bench": "attention_segments", "dh": dh, "B": B, "H": H, "S": S, "L": L, "p": p,
                          "causal_ms": round(med["causal"], 4), "causal_spread_ms": spread("causal"),
                          "band_ms": round(med["band"], 4), "band_spread_ms": spread("band"),
                          "seg_ms": round(med["seg"], 4), "seg_spread_ms": spread("seg"),
                          "seg_over_causal": round(med["seg"] / med["causal"], 4), "seg_over_band": round(med["seg"] / med["band"], 4),
                          "band_fwd_ms": round(med["band_fwd"], 4), "seg_fwd_ms": round(med["seg_fwd"], 4),
                          "seg_fwd_over_band_fwd": round(med["seg_fwd"] / med["band_fwd"], 4),
                          "pairs_seg_over_band": round(pairs_seg / pairs_band, 4),
                          "bwd_kernel_ms": round(split["kernel"][1], 4), "bwd_strips_ms": round(split["strips"][1], 4),
                          "strip_share": round(split["strips"][1] / max(split["strips"][1] + split["kernel"][1], 1e-9), 4),
                          "seg_tflops": round(3 * 4.0 * BH * dh * pairs_seg / (med["seg"] * 1e-3) / 1e12, 2)})   # forward 2 products, backward 4
                del bs, bds, bpd, bbits, lo
            del Q, K, V, G, out, stats, dQ, dK, dV, cs, cds, cpd, cbits
    dev.sync()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
