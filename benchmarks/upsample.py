"""Upsampling kernels against a copy of the same number of bytes, HIP events on the compute stream (warm-up, windows of at least
25 ms), at
    (8, 256, 64, 64)    -> 128 x 128     the first up-block of a U-Net, 134 MB out (cache-assisted)
    (8, 128, 128, 128)  -> 256 x 256     268 MB out
    (16, 256, 128, 128) -> 256 x 256     a 1 GiB output
    python benchmarks/upsample.py [min_ms]          # appends to profiles/r26_upsample.jsonl as well
One JSON line per (shape, mode, pass): forward and dx in the assign form, nearest (the x2 class) and bilinear (the vector class),
each timed in the same process in alternation with `nk_copy` of the same bytes and with the GENERIC class of the same call - the
same buffers entered one float past a 16-byte boundary, which is how the library itself falls back to it (copy, generic, class,
copy, ...: the best window of each, every window listed, so the spread of the alternation is in the line).  Algorithmic bytes:
(in + out) * 4 per plane for the forward, and the same for the backward in the assign form."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuronika_amd import capi as c  # noqa: E402

SHAPES = [((8, 256, 64, 64), (128, 128), "134 MB out"), ((8, 128, 128, 128), (256, 256), "268 MB out"),
          ((16, 256, 128, 128), (256, 256), "1 GiB out")]
OUT = os.path.join(ROOT, "profiles", "r26_upsample.jsonl")


def main():
    min_ms = float(sys.argv[1]) if len(sys.argv) > 1 else 25.0
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/upsample.py needs a GPU")
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
    for shape, size, label in SHAPES:
        n_in, n_out = int(np.prod(shape)), int(np.prod(shape[:2] + size))
        rng = np.random.default_rng(0)
        # four floats of slack: the same storage serves the aligned call and the one a float further on
        XB, YB = dev.zeros((n_in + 4,)), dev.zeros((n_out + 4,))
        chunk = 1 << 24
        for buf, n in ((XB, n_in), (YB, n_out)):                                   # random contents without a host array of the full size
            piece = dev.array(rng.standard_normal(min(chunk, n), dtype=np.float32))
            for at in range(0, n, chunk):
                m = min(chunk, n - at)
                c.check(c.lib.nk_copy(dev.h, buf.view_offset(at).p, piece.p, m))
        X, Y, X1, Y1 = XB.view_offset(0), YB.view_offset(0), XB.view_offset(1), YB.view_offset(1)
        nbytes = 4 * (n_in + n_out)
        m = nbytes // 8
        SRC, DST = dev.zeros((m,)), dev.zeros((m,))
        copy = lambda: c.check(c.lib.nk_copy(dev.h, DST.p, SRC.p, m))
        for mode in ("nearest", "linear"):
            cases = [("upsample_fwd", lambda: c.upsample_fwd(dev, X, shape, Y, size, mode), lambda: c.upsample_fwd(dev, X1, shape, Y1, size, mode)),
                     ("upsample_bwd_assign (dx)", lambda: c.upsample_bwd(dev, X, shape, Y, size, mode, assign=True),
                      lambda: c.upsample_bwd(dev, X1, shape, Y1, size, mode, assign=True))]
            for name, fn, generic in cases:
                ms_k, ms_g, ms_c = [], [], []
                for _ in range(3):
                    ms_c.append(window(copy))
                    ms_g.append(window(generic))
                    ms_k.append(window(fn))
                k, gms, cp = min(ms_k), min(ms_g), min(ms_c)
                rate, copy_rate = nbytes / (k * 1e-3), 8 * m / (cp * 1e-3)
                line = json.dumps({"bench": "upsample", "shape": list(shape), "out_size": list(size), "size": label, "mode": mode, "kernel": name,
                                   "class": "nearest x2" if mode == "nearest" else "vector", "algorithmic_bytes": nbytes, "ms": round(k, 5),
                                   "ms_windows": [round(v, 5) for v in ms_k], "TBps": round(rate / 1e12, 3),
                                   "generic_ms": round(gms, 5), "generic_ms_windows": [round(v, 5) for v in ms_g], "ratio_to_generic_time": round(k / gms, 3),
                                   "copy_bytes": 8 * m, "copy_ms": round(cp, 5), "copy_ms_windows": [round(v, 5) for v in ms_c],
                                   "copy_TBps": round(copy_rate / 1e12, 3), "ratio_to_copy": round(rate / copy_rate, 3)})
                print(line, flush=True)
                lines.append(line)
        del XB, YB, X, Y, X1, Y1, SRC, DST
    dev.sync()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
