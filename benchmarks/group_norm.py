"""Group normalisation kernels against their three yardsticks, HIP events on the compute stream (warm-up, windows of at least
25 ms): forward (with statistics), dx (assign form) and the parameter pass (assign form) at
    (512, 512, 1024, 32)    D = 16 * 1024 = 16384: the row in registers (a block per row), 1 GiB per tensor
    (51, 1280, 4096, 32)    D = 40 * 4096 = 163840: the chunked class (the first U-Net stage at 64 x 64), 1.0 GiB per tensor
    (128, 64, 3136, 32)     D = 2 * 3136 = 6272: C3-sized, 98 MB per tensor (cache-assisted)
    python benchmarks/group_norm.py [min_ms]          # appends to profiles/r25_group_norm.jsonl as well
One JSON line per (shape, kernel): the GroupNorm entry, `nk_copy`, the `nk_layer_norm_*` entry at the same (rows, D) - the same
traffic; GroupNorm's extra work is the channel index and the gamma gather - and the composed path the tape would otherwise take
(layer norm without affine, then a broadcasting multiply and add; backward: the multiply's input gradient, then layer norm's dx;
parameters: the multiply's right gradient and an unbroadcast sum), timed in the same process in alternation (copy, layer norm,
composed, group norm, copy, ...: the best window of each, every window listed, so the spread of the alternation is in the line).
Algorithmic bytes (4 B x elements read + written; parameters, statistics and partial sums left out, under 1 %): forward 8 n, dx in
the assign form 12 n, the parameter pass 8 n.  The chunked class reads x twice forward (12 n moved) and g and x twice in dx (20 n
moved); its rates are still quoted over the algorithmic bytes, and `moved_bytes` is in the line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuronika_amd import capi as c  # noqa: E402

SHAPES = [(512, 512, 1024, 32, "1 GiB per tensor, registers"), (51, 1280, 4096, 32, "1.0 GiB per tensor, chunked"),
          (128, 64, 3136, 32, "C3-sized (98 MB per tensor), registers")]
OUT = os.path.join(ROOT, "profiles", "r25_group_norm.jsonl")


def main():
    min_ms = float(sys.argv[1]) if len(sys.argv) > 1 else 25.0
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/group_norm.py needs a GPU")
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
    for N, C, L, G, label in SHAPES:
        n, rows, D = N * C * L, N * G, (C // G) * L
        chunked = D > 16384
        rng = np.random.default_rng(0)
        X = dev.array(rng.standard_normal((N, C, L), dtype=np.float32))
        GR = dev.array(rng.standard_normal((N, C, L), dtype=np.float32))
        W, B = dev.array(rng.standard_normal(C, dtype=np.float32)), dev.array(rng.standard_normal(C, dtype=np.float32))
        WD, BD = dev.array(rng.standard_normal(D, dtype=np.float32)), dev.array(rng.standard_normal(D, dtype=np.float32))
        W3, B3 = dev.array(rng.standard_normal((C, 1), dtype=np.float32)), dev.array(rng.standard_normal((C, 1), dtype=np.float32))
        Y, T = dev.zeros((N, C, L)), dev.zeros((N, C, L))
        S, DG, DB, DGD, DBD = dev.zeros((rows, 2)), dev.zeros((C,)), dev.zeros((C,)), dev.zeros((D,)), dev.zeros((D,))
        DW3, DB3 = dev.zeros((C, 1)), dev.zeros((C, 1))
        c.group_norm_fwd(dev, X, W, B, Y, S, N, C, L, G, 1e-5)

        def composed_fwd():
            c.layer_norm_fwd(dev, X, None, None, T, S, rows, D, 1e-5)
            c.binary_fwd(dev, "mul", Y, T, W3)
            c.binary_fwd(dev, "add", Y, Y, B3)

        def composed_dx():
            c.binary_bwd_left(dev, "mul", T, GR, W3, assign=True)
            c.layer_norm_bwd(dev, Y, T, X, None, S, rows, D, assign=True)

        def composed_params():                                                     # T holds xhat after composed_fwd
            c.binary_bwd_right(dev, "mul", DW3, GR, l=T, r=W3, assign=True)
            c.unbroadcast_add(dev, DB3, GR, assign=True)

        cases = [("group_norm_fwd", lambda: c.group_norm_fwd(dev, X, W, B, Y, S, N, C, L, G, 1e-5),
                  "layer_norm_fwd", lambda: c.layer_norm_fwd(dev, X, WD, BD, Y, S, rows, D, 1e-5), composed_fwd, 8 * n, 12 * n if chunked else 8 * n),
                 ("group_norm_bwd_assign (dx)", lambda: c.group_norm_bwd(dev, Y, GR, X, W, S, N, C, L, G, assign=True),
                  "layer_norm_bwd_assign (dx)", lambda: c.layer_norm_bwd(dev, Y, GR, X, WD, S, rows, D, assign=True), composed_dx, 12 * n,
                  20 * n if chunked else 12 * n),
                 ("group_norm_bwd_params_assign (dgamma, dbeta)", lambda: c.group_norm_bwd_params(dev, DG, DB, GR, X, S, N, C, L, G, assign=True),
                  "layer_norm_bwd_params_assign (dgamma, dbeta)", lambda: c.layer_norm_bwd_params(dev, DGD, DBD, GR, X, S, rows, D, assign=True),
                  composed_params, 8 * n, 8 * n)]
        for name, fn, ln_name, ln_fn, comp_fn, nbytes, moved in cases:
            if comp_fn is composed_params:
                c.layer_norm_fwd(dev, X, None, None, T, S, rows, D, 1e-5)            # xhat for the multiply's right gradient
            m = min(nbytes // 8, n)                                                # a copy's rate does not depend on the count at this size
            copy = lambda: c.check(c.lib.nk_copy(dev.h, Y.p, X.p, m))
            ms_k, ms_l, ms_c, ms_p = [], [], [], []
            for _ in range(3):
                ms_c.append(window(copy))
                ms_l.append(window(ln_fn))
                ms_p.append(window(comp_fn))
                ms_k.append(window(fn))
            k, ln, cp, co = min(ms_k), min(ms_l), min(ms_c), min(ms_p)
            rate, copy_rate = nbytes / (k * 1e-3), 8 * m / (cp * 1e-3)
            line = json.dumps({"bench": "group_norm", "shape": [N, C, L, G], "rows_D": [rows, D], "size": label, "kernel": name,
                               "algorithmic_bytes": nbytes, "moved_bytes": moved, "ms": round(k, 5), "ms_windows": [round(v, 5) for v in ms_k],
                               "TBps": round(rate / 1e12, 3), "moved_TBps": round(moved / (k * 1e-3) / 1e12, 3),
                               "layer_norm_kernel": ln_name, "layer_norm_ms": round(ln, 5), "layer_norm_ms_windows": [round(v, 5) for v in ms_l],
                               "ratio_to_layer_norm_time": round(k / ln, 3),
                               "composed_ms": round(co, 5), "composed_ms_windows": [round(v, 5) for v in ms_p], "ratio_to_composed_time": round(k / co, 3),
                               "copy_bytes": 8 * m, "copy_ms": round(cp, 5), "copy_ms_windows": [round(v, 5) for v in ms_c],
                               "copy_TBps": round(copy_rate / 1e12, 3), "ratio_to_copy": round(rate / copy_rate, 3)})
            print(line, flush=True)
            lines.append(line)
        del X, GR, Y, T
    dev.sync()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
