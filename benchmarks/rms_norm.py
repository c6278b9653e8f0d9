"""RMS normalisation kernels against their two yardsticks, HIP events on the compute stream (warm-up, windows of at least 25 ms):
forward (with statistics), dx (assign form) and dgamma (assign form) at
    (262144, 1024)  (65536, 4096)  (32768, 8192)   1 GiB per tensor: the judged rows (wave kernels, block kernels V = 4 and 8)
    (8192, 1024)    C5-sized, 32 MB per tensor: cache-assisted (the 256 MB Infinity Cache holds all of it)
    (8, 4096)       decode-sized, 128 KB: a launch, not a stream
    python benchmarks/rms_norm.py [min_ms]          # writes profiles/r19_rms_norm.jsonl as well
One JSON line per (shape, kernel): the RMSNorm kernel, `nk_copy` of the SAME byte count and the `nk_layer_norm_*` entry of the same
shape, timed in the same process in alternation (copy, layer norm, rms norm, copy, ...: the best window of each, every window
listed, so the spread of the alternation is in the line).  Algorithmic bytes (4 B x elements read + written; gamma, stats and the
partial sums are left out, under 1 %): forward 8 n, dx in the assign form 12 n, dgamma 8 n (g, x read).  LayerNorm's parameter pass
moves the same 8 n and writes two partial rows per split where dgamma writes one."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuronika_amd import capi as c  # noqa: E402

SHAPES = [(262144, 1024, "1 GiB per tensor"), (65536, 4096, "1 GiB per tensor"), (32768, 8192, "1 GiB per tensor"),
          (8192, 1024, "cache-assisted (32 MB per tensor)"), (8, 4096, "decode-sized (128 KB per tensor)")]
OUT = os.path.join(ROOT, "profiles", "r19_rms_norm.jsonl")


def main():
    min_ms = float(sys.argv[1]) if len(sys.argv) > 1 else 25.0
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/rms_norm.py needs a GPU")
    dev = c.Device(0)

    def window(fn):
        e0, e1 = dev.event(), dev.event()
        e0.record(); calls = 0
        while True:
            fn(); fn(); calls += 2
            e1.record(); e1.sync()
            if e0.elapsed_ms(e1) >= min_ms:
                break
        iters = max(4, int(min_ms / max(e0.elapsed_ms(e1) / calls, 1e-3)) + 1)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record(); e1.sync()
        return e0.elapsed_ms(e1) / iters

    lines = []
    for rows, D, label in SHAPES:
        n = rows * D
        rng = np.random.default_rng(0)
        X = dev.array(rng.standard_normal((rows, D), dtype=np.float32))
        G = dev.array(rng.standard_normal((rows, D), dtype=np.float32))
        W, B = dev.array(rng.standard_normal(D, dtype=np.float32)), dev.array(rng.standard_normal(D, dtype=np.float32))
        Y, S, S2, DG, DB = dev.zeros((rows, D)), dev.zeros((rows,)), dev.zeros((rows, 2)), dev.zeros((D,)), dev.zeros((D,))
        c.rms_norm_fwd(dev, X, W, Y, S, rows, D, 1e-6)
        c.layer_norm_fwd(dev, X, W, B, Y, S2, rows, D, 1e-5)
        cases = [("rms_norm_fwd", lambda: c.rms_norm_fwd(dev, X, W, Y, S, rows, D, 1e-6),
                  "layer_norm_fwd", lambda: c.layer_norm_fwd(dev, X, W, B, Y, S2, rows, D, 1e-5), 8 * n),
                 ("rms_norm_bwd_assign (dx)", lambda: c.rms_norm_bwd(dev, Y, G, X, W, S, rows, D, assign=True),
                  "layer_norm_bwd_assign (dx)", lambda: c.layer_norm_bwd(dev, Y, G, X, W, S2, rows, D, assign=True), 12 * n),
                 ("rms_norm_bwd_gamma_assign (dgamma)", lambda: c.rms_norm_bwd_gamma(dev, DG, G, X, S, rows, D, assign=True),
                  "layer_norm_bwd_params_assign (dgamma, dbeta)", lambda: c.layer_norm_bwd_params(dev, DG, DB, G, X, S2, rows, D, assign=True), 8 * n)]
        for name, fn, ln_name, ln_fn, nbytes in cases:
            # 12 n bytes as a copy need 1.5 n floats of source and destination: the copy of the dx row moves n floats and its RATE
            # stands in (a copy's rate does not depend on the count at this size)
            m = min(nbytes // 8, n)
            copy = lambda: c.check(c.lib.nk_copy(dev.h, Y.p, X.p, m))
            ms_k, ms_l, ms_c = [], [], []
            for _ in range(3):
                ms_c.append(window(copy))
                ms_l.append(window(ln_fn))
                ms_k.append(window(fn))
            k, ln, cp = min(ms_k), min(ms_l), min(ms_c)
            rate, copy_rate = nbytes / (k * 1e-3), 8 * m / (cp * 1e-3)
            line = json.dumps({"bench": "rms_norm", "shape": [rows, D], "size": label, "kernel": name, "algorithmic_bytes": nbytes,
                               "ms": round(k, 5), "ms_windows": [round(v, 5) for v in ms_k], "TBps": round(rate / 1e12, 3),
                               "layer_norm_kernel": ln_name, "layer_norm_ms": round(ln, 5), "layer_norm_ms_windows": [round(v, 5) for v in ms_l],
                               "ratio_to_layer_norm_time": round(k / ln, 3),
                               "copy_bytes": 8 * m, "copy_ms": round(cp, 5), "copy_ms_windows": [round(v, 5) for v in ms_c],
                               "copy_TBps": round(copy_rate / 1e12, 3), "ratio_to_copy": round(rate / copy_rate, 3)})
            print(line, flush=True)
            lines.append(line)
        del X, G, Y
    dev.sync()
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
