"""AdamW and global-norm clipping, HIP events on the compute stream (warm-up, windows of at least `min_ms`, the best of three), all in
ONE process on one device:

  streaming, 1 GiB per tensor (through the C ABI)
    adamw / adamw_amsgrad   nk_adamw_step: 28 / 36 bytes per element (g read; w, m, v[, vmax] read and written)
    clip_measure_only       nk_clip_grad_norm_multi, max_norm = +inf: the norm pass and the one-block finalize, 4 bytes per element
    clip_unclipped          a finite max_norm above the norm: the same plus the scale launch, whose blocks return at coef == 1
    clip_clipped            max_norm below the norm at every call (it shrinks by 0.1 % a call): norm pass + scale pass, 12 bytes per
                            element; `scale_pass_derived_ms` = clip_clipped - clip_measure_only (8 bytes per element), a difference
                            of two measurements, not a measurement
    each with the time of `nk_copy` between two 1 GiB buffers timed in alternation, and `per_byte_ratio_to_copy` = (ms / bytes) of
    the kernel over (ms / bytes) of the copy (above 1: slower per byte moved than the copy)
  launch-bound (through the tape)
    the parameter list of a 12-layer, d = 768, vocabulary 50257 decoder (148 tensors, 124 M elements), and the same list without
    its three largest tensors: `optim::AdamW.step()` (one nk_adamw_step_multi call: ceil(148 / 32) launches) against
    `optim::Adam.step()` (one launch per parameter), alternating, both warmed.  Launch counts are computed from the list.

    python benchmarks/adamw.py [--min-ms 25] [--out profiles/r15_adamw.jsonl]
One JSON line per measurement, printed and written to `--out`."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLE = 32          # OPT_MULTI_MAX of neuronika_amd/csrc/nk_optim_multi.h


def decoder_shapes(layers=12, d=768, vocab=50257, positions=1024):
    shapes = [(vocab, d), (positions, d)]
    for _ in range(layers):
        shapes += [(d,), (d,), (3 * d, d), (3 * d,), (d, d), (d,), (d,), (d,), (4 * d, d), (4 * d,), (d, 4 * d), (d,)]
    return shapes + [(d,), (d,)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-ms", type=float, default=25.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_adamw.jsonl"))
    ap.add_argument("--elems", type=int, default=1 << 28, help="elements per tensor of the streaming part (1 GiB)")
    args = ap.parse_args()

    import neuronika_amd
    from neuronika_amd import capi as c
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/adamw.py needs a GPU")
    t = neuronika_amd.tape
    tdev = t.Device(0)
    dev = c.Device(handle=tdev.raw())
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def window(fn):
        e0, e1 = dev.event(), dev.event()
        e0.record(); calls = 0
        while True:
            fn(); fn(); calls += 2
            e1.record(); e1.sync()
            if e0.elapsed_ms(e1) >= args.min_ms:
                break
        iters = max(4, int(args.min_ms / max(e0.elapsed_ms(e1) / calls, 1e-3)) + 1)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record(); e1.sync()
        return e0.elapsed_ms(e1) / iters

    # ---- streaming --------------------------------------------------------------------------------------------------------------
    n = args.elems
    rng = np.random.default_rng(0)
    host = rng.standard_normal(n, dtype=np.float32)
    W, G = dev.array(host), dev.array(host[::-1])
    del host
    M, V, VM = dev.zeros(n), dev.zeros(n), dev.zeros(n)
    SRC, DST = dev.zeros(n), dev.zeros(n)
    OUT = dev.zeros(2)
    copy = lambda: c.check(c.lib.nk_copy(dev.h, DST.p, SRC.p, n))
    max_norm = [float(np.sqrt(n))]                      # about the norm of the N(0, 1) gradient

    def clipped():
        max_norm[0] *= 0.999
        c.clip_grad_norm_multi(dev, [G], max_norm[0], OUT)

    cases = [
        ("adamw", lambda: c.adamw_step(dev, W, G, M, V, None, lr=1e-9, step=1000, weight_decay=0.1), 28 * n),
        ("adamw_amsgrad", lambda: c.adamw_step(dev, W, G, M, V, VM, lr=1e-9, step=1000, weight_decay=0.1), 36 * n),
        ("clip_measure_only", lambda: c.clip_grad_norm_multi(dev, [G], float("inf"), OUT), 4 * n),
        ("clip_unclipped", lambda: c.clip_grad_norm_multi(dev, [G], 1e30, OUT), 4 * n),
        ("clip_clipped", clipped, 12 * n),
    ]
    measured = {}
    for name, fn, nbytes in cases:
        ms_k, ms_c = [], []
        for _ in range(3):
            ms_c.append(window(copy))
            ms_k.append(window(fn))
        k, cp = min(ms_k), min(ms_c)
        measured[name] = k
        emit({"bench": "adamw", "part": "streaming", "kernel": name, "elements": n, "algorithmic_bytes": nbytes, "ms": round(k, 4),
              "ms_windows": [round(v, 4) for v in ms_k], "GBps": round(nbytes / (k * 1e-3) / 1e9, 1), "copy_ms": round(cp, 4),
              "copy_GBps": round(8 * n / (cp * 1e-3) / 1e9, 1), "per_byte_ratio_to_copy": round((k / nbytes) / (cp / (8 * n)), 3)})
    coef = float(OUT.numpy()[1])
    derived = measured["clip_clipped"] - measured["clip_measure_only"]
    emit({"bench": "adamw", "part": "streaming", "kernel": "clip_summary", "clipped_ms": round(measured["clip_clipped"], 4),
          "unclipped_ms": round(measured["clip_unclipped"], 4), "measure_only_ms": round(measured["clip_measure_only"], 4),
          "unclipped_over_clipped": round(measured["clip_unclipped"] / measured["clip_clipped"], 3),
          "scale_pass_derived_ms": round(derived, 4), "scale_pass_derived_GBps": round(8 * n / (derived * 1e-3) / 1e9, 1),
          "last_coef_of_the_clipped_run": coef})
    del W, G, M, V, VM, SRC, DST

    # ---- launch-bound -------------------------------------------------------------------------------------------------------------
    full = decoder_shapes()
    largest = sorted(range(len(full)), key=lambda i: -math.prod(full[i]))[:3]
    lists = [("decoder_12x768", full), ("decoder_12x768_without_3_largest", [s for i, s in enumerate(full) if i not in largest])]
    for label, shapes in lists:
        params = [t.from_ndarray(tdev, np.full(s, 0.01, np.float32)).requires_grad() for s in shapes]
        adamw, adam = t.optim.AdamW(1e-9, weight_decay=0.1), t.optim.Adam(1e-9)
        for p in params:
            adamw.register(p); adam.register(p)
            p.set_grad(np.full(p.shape, 1e-3, np.float32))
        for _ in range(3):
            adamw.step(); adam.step()
        a, b = [], []
        for _ in range(3):
            b.append(window(adam.step))
            a.append(window(adamw.step))
        elems = sum(math.prod(s) for s in shapes)
        emit({"bench": "adamw", "part": "launch_bound", "list": label, "tensors": len(shapes), "elements": elems,
              "adamw_step_ms": round(min(a), 4), "adam_step_ms": round(min(b), 4), "adamw_windows": [round(v, 4) for v in a],
              "adam_windows": [round(v, 4) for v in b], "adam_over_adamw": round(min(b) / min(a), 2),
              "adamw_launches_computed": math.ceil(len(shapes) / TABLE), "adam_launches_computed": len(shapes),
              "adamw_GBps": round(28 * elems / (min(a) * 1e-3) / 1e9, 1), "adam_GBps": round(28 * elems / (min(b) * 1e-3) / 1e9, 1)})
        del params, adamw, adam
    dev.sync()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
