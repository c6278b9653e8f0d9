"""The sliding-window fused core (nk_attention_band_fwd + _bwd), HIP events on the compute stream (warm-up, windows of at least
`min_ms`), all in ONE process on one device; written after benchmarks/attention_decode_window.py.  The claims under test: the band
core beats the causal core wherever S >= 4 W, its time grows about linearly in S at fixed W, and it beats the composed banded path.

  core (through the C ABI), forward + backward, dh in {64, 128}, S in {2048, 4096, 8192}, W in {256, 1024, 4096} with W < S,
  p in {0, 0.1} (training), B * S = `tokens` rows of H heads.  Per point, timed in alternation, `repeats` windows each:
    causal    nk_attention_causal_fwd + _bwd at the same S: the kernels the band kernels were copied from, unchanged.  Its own
              run-to-run spread max - min over its windows is reported next to every ratio.
    band      nk_attention_band_fwd + _bwd.  `band_over_causal` = median(band) / median(causal).
    split     one profiled backward per class (nk_profile_*): the fused kernel against the per-strip dK / dV products;
              `strip_share` = products / (kernel + products).
    scratch   bytes of scores + dS + Pd + mask words in the banded layout and in the (SP, SP) layout.
  module (through the tape), forward + backward of nn::MultiheadAttention at the same (S, W, dh), p = 0: `fused_core = true` (the
  band core) against `fused_core = false` (the composed path with the banded constant: what forward() ran before the core took a
  window), host clock around a device synchronise.  Skipped where one (B*H, S, S) temporary exceeds `--composed-limit-gb`.

    python benchmarks/attention_band.py [--min-ms 25] [--out profiles/r23_attention_band.jsonl]
One JSON line per point, printed and written to `--out`; `t(2S) / t(S)` per sequence at fixed W is computed from those lines at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-ms", type=float, default=25.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=16384, help="B * S")
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--lengths", type=int, nargs="*", default=[2048, 4096, 8192])
    ap.add_argument("--windows", type=int, nargs="*", default=[256, 1024, 4096])
    ap.add_argument("--head-sizes", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--probs", type=float, nargs="*", default=[0.0, 0.1])
    ap.add_argument("--composed-limit-gb", type=float, default=6.0)
    ap.add_argument("--no-module", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_attention_band.jsonl"))
    args = ap.parse_args()

    from neuronika_amd import capi as c
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/attention_band.py needs a GPU")
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
            for W in [w for w in args.windows if w < S]:
                ext, words, ld = c.attention_band_scratch(S, W), c.attention_band_mask_words(S, W), c.attention_band_ld(S, W)
                bs, bds, bpd, bbits = dev.zeros((BH, ext)), dev.zeros((BH, ext)), dev.zeros((BH, ext)), dev.zeros((BH, words))
                for p in args.probs:
                    def causal_fwd():
                        c.attention_fwd(dev, Q, K, V, cs, stats, cbits, out, B, S, H, dh, scale, p, True, 1, 0, causal=True)

                    def causal_bwd():
                        c.attention_bwd(dev, dQ, dK, dV, cds, cpd, G, out, cs, stats, cbits, Q, K, V, B, S, H, dh, scale, p, True,
                                        assign=(True, True, True), causal=True)

                    def band_fwd():
                        c.attention_band_fwd(dev, Q, K, V, bs, stats, bbits, out, B, S, H, dh, scale, p, True, 1, 0, window=W)

                    def band_bwd():
                        c.attention_band_bwd(dev, dQ, dK, dV, bds, bpd, G, out, bs, stats, bbits, Q, K, V, B, S, H, dh, scale, p, True,
                                             assign=(True, True, True), window=W)

                    calls = {"causal": lambda: (causal_fwd(), causal_bwd()), "band": lambda: (band_fwd(), band_bwd()),
                             "causal_fwd": causal_fwd, "band_fwd": band_fwd}
                    ms = {name: [] for name in calls}
                    for _ in range(args.repeats):                        # interleaved: every window of one next to a window of the other
                        for name, fn in calls.items():
                            ms[name].append(window(fn))
                    med = {name: statistics.median(v) for name, v in ms.items()}
                    band_fwd()                                           # the backward below reads the band forward's state
                    split = {}
                    for klass, name in ((c.KERNEL_ATTENTION, "kernel"), (c.KERNEL_SGEMM, "strips")):
                        dev.profile_begin()
                        band_bwd()
                        n, t, _ = dev.profile_end(klass)
                        split[name] = (n, t)
                    pairs = sum(min(r + 1, W) for r in range(S))
                    emit({"bench": "attention_band", "dh": dh, "B": B, "H": H, "S": S, "W": W, "p": p, "ld": ld,
                          "causal_ms": round(med["causal"], 4), "causal_spread_ms": round(max(ms["causal"]) - min(ms["causal"]), 4),
                          "band_ms": round(med["band"], 4), "band_spread_ms": round(max(ms["band"]) - min(ms["band"]), 4),
                          "band_over_causal": round(med["band"] / med["causal"], 4),
                          "causal_fwd_ms": round(med["causal_fwd"], 4), "band_fwd_ms": round(med["band_fwd"], 4),
                          "bwd_kernel_ms": round(split["kernel"][1], 4), "bwd_strips_ms": round(split["strips"][1], 4),
                          "bwd_strip_launches": split["strips"][0],
                          "strip_share": round(split["strips"][1] / max(split["strips"][1] + split["kernel"][1], 1e-9), 4),
                          "band_tflops": round(3 * 4.0 * BH * dh * pairs / (med["band"] * 1e-3) / 1e12, 2),   # forward 2 products, backward 4 (dK, dV included)
                          "scratch_band_bytes": 4 * BH * (3 * ext + words), "scratch_square_bytes": 4 * BH * (3 * SP * SP + SP * SP // 32)})
                del bs, bds, bpd, bbits
            del Q, K, V, G, out, stats, dQ, dK, dV, cs, cds, cpd, cbits
    dev.sync()

    if not args.no_module:
        import neuronika_amd
        nk = neuronika_amd.tape
        tdev = nk.Device(0)
        for dh in args.head_sizes:
            d = H * dh
            for S in args.lengths:
                B = max(1, args.tokens // S)
                if 4.0 * B * H * S * S / 2 ** 30 > args.composed_limit_gb:
                    emit({"bench": "attention_band_module", "dh": dh, "B": B, "H": H, "S": S, "skipped": "one (B*H, S, S) temporary exceeds the limit"})
                    continue
                x = (np.random.default_rng(1).random((B * S, d), dtype=np.float32) - np.float32(0.5))
                for W in [w for w in args.windows if w < S]:
                    res = {}
                    for core in (True, False):
                        mha = nk.nn.MultiheadAttention(tdev, d, H, 0.0, 3)
                        mha.causal, mha.window, mha.fused_core = True, W, core
                        X = nk.from_ndarray(tdev, x).requires_grad()
                        y = mha.forward(X, B)
                        g = nk.from_ndarray(tdev, x)

                        def step():
                            y.forward(); y.backward_from(g)

                        step(); tdev.sync()
                        ts = []
                        for _ in range(args.repeats):
                            n, t0 = 0, time.perf_counter()
                            while True:
                                step(); n += 1
                                if n >= 2 and (time.perf_counter() - t0) * 1e3 >= args.min_ms:
                                    break
                            tdev.sync()
                            ts.append((time.perf_counter() - t0) * 1e3 / n)
                        res[core] = (statistics.median(ts), y.history_len())
                        del mha, X, y, g
                    emit({"bench": "attention_band_module", "dh": dh, "B": B, "H": H, "S": S, "W": W, "p": 0.0,
                          "core_ms": round(res[True][0], 4), "composed_ms": round(res[False][0], 4), "core_nodes": res[True][1],
                          "composed_nodes": res[False][1], "composed_over_core": round(res[False][0] / res[True][0], 3)})

    # t(2S) / t(S) at fixed W, per sequence (the points hold B * S fixed, so the batch halves as S doubles)
    for kind in ("band", "causal"):
        core = {(r["dh"], r["W"], r["p"], r["S"]): r[kind + "_ms"] / r["B"] for r in rows if r["bench"] == "attention_band"}
        for (dh, W, p, S), t in sorted(core.items()):
            if (dh, W, p, 2 * S) in core:
                emit({"bench": "attention_band_scaling", "kernels": kind, "dh": dh, "W": W, "p": p, "S": S,
                      "t2S_over_tS_per_sequence": round(core[(dh, W, p, 2 * S)] / t, 3)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
