"""nk_quant_linear_fwd against the f32 nk_linear_fwd it replaces in decoding, HIP events on the compute stream, at the projection shapes
of a 7B-class model:
    (N, K) = (8192, 8192)  and  (28672, 8192),   M in {1, 2, 4, 8, 16, 32, 64, 128},   bits in {8, 4},   group in {128, 0}
    python benchmarks/quant_linear.py [min_ms]          # appends to profiles/r27_quant_linear.jsonl as well
Every timed loop ROTATES over enough distinct weight buffers that the working set exceeds twice the 256 MiB last-level cache (the
67 MB int8 image of the small shape would otherwise be served from it): call i reads buffer i % n.  Per (shape, M) the f32 product and,
per variant, the rows path (NK_TUNE_QUANT_ROWS forced high: ceil(M / 8) passes) and the many-row path (forced 0: unpack + GEMM) are
timed in alternation in one process, two rounds, the best window of each; `nk_copy` of 512 MiB is timed in the same session.
One JSON line per (shape, M, bits, group): ms of each path, the weight bytes per second of the rows path, the copy rate, the f32
time.  The last lines give, per bits, L = the largest M up to which the rows path beats unpack + GEMM at every smaller-or-equal M on
both shapes and both groups - the number QL_RULE_* in csrc/nk_quant_linear.h is set from."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuronika_amd import capi as c  # noqa: E402

SHAPES = [(8192, 8192), (28672, 8192)]
MS = [1, 2, 4, 8, 16, 32, 64, 128]
VARIANTS = [(8, 128), (8, 0), (4, 128), (4, 0)]
WORKING_SET = 2 * (256 << 20)
OUT = os.path.join(ROOT, "profiles", "r27_quant_linear.jsonl")


def main():
    min_ms = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/quant_linear.py needs a GPU")
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

    def rotating(call, bufs):
        state = [0]

        def fn():
            call(bufs[state[0] % len(bufs)])
            state[0] += 1
        return fn

    m_copy = WORKING_SET // 8
    SRC, DST = dev.zeros((m_copy,)), dev.zeros((m_copy,))
    copy = lambda: c.check(c.lib.nk_copy(dev.h, DST.p, SRC.p, m_copy))
    lines, faster = [], {}
    rng = np.random.default_rng(0)
    for N, K in SHAPES:
        piece = dev.array(rng.standard_normal(1 << 24, dtype=np.float32) * np.float32(0.02))

        def f32_weight():
            W = dev.zeros((N, K))
            for at in range(0, N * K, 1 << 24):
                c.check(c.lib.nk_copy(dev.h, W.view_offset(at).p, piece.p, min(1 << 24, N * K - at)))
            return W

        Wf = [f32_weight() for _ in range(WORKING_SET // (4 * N * K) + 1)]
        bias = dev.array(rng.standard_normal(N, dtype=np.float32))
        images = {}
        for bits, group in VARIANTS:
            n = WORKING_SET // (N * K * bits // 8) + 1
            imgs = []
            for i in range(n):
                qw, sc = dev.zeros((c.quant_linear_words(N, K, bits),)), dev.zeros((c.quant_linear_scales(N, K, group),))
                c.quant_linear_pack(dev, Wf[i % len(Wf)], K, qw, sc, N, K, bits, group)
                imgs.append((qw, sc))
            images[(bits, group)] = imgs
        copy_ms = min(window(copy) for _ in range(3))
        for M in MS:
            X, Y = dev.array(rng.standard_normal((M, K), dtype=np.float32)), dev.zeros((M, N))
            f32 = rotating(lambda W: c.linear_fwd(dev, X, W, bias, Y), Wf)
            best = {}
            for _ in range(2):
                for bits, group in VARIANTS:
                    q = rotating(lambda img: c.quant_linear_fwd(dev, X, K, img[0], img[1], bias, Y, N, M, N, K, bits, group), images[(bits, group)])
                    best["f32"] = min(best.get("f32", 1e9), window(f32))
                    dev.quant_rows(1 << 20)
                    best[(bits, group, "rows")] = min(best.get((bits, group, "rows"), 1e9), window(q))
                    dev.quant_rows(0)
                    best[(bits, group, "many")] = min(best.get((bits, group, "many"), 1e9), window(q))
                    dev.quant_rows(None)
            for bits, group in VARIANTS:
                rows_ms, many_ms = best[(bits, group, "rows")], best[(bits, group, "many")]
                wbytes = N * K * bits // 8
                faster.setdefault(bits, {}).setdefault(M, []).append(rows_ms < many_ms)
                line = json.dumps({"bench": "quant_linear", "N": N, "K": K, "M": M, "bits": bits, "group": group,
                                   "weight_buffers": len(images[(bits, group)]), "rows_passes": (M + 7) // 8, "rows_ms": round(rows_ms, 5),
                                   "rows_weight_TBps": round(((M + 7) // 8) * wbytes / (rows_ms * 1e-3) / 1e12, 3), "many_ms": round(many_ms, 5),
                                   "f32_linear_ms": round(best["f32"], 5), "f32_weight_TBps": round(4 * N * K / (best["f32"] * 1e-3) / 1e12, 3),
                                   "rows_over_f32": round(rows_ms / best["f32"], 3), "copy_ms": round(copy_ms, 5),
                                   "copy_TBps": round(8 * m_copy / (copy_ms * 1e-3) / 1e12, 3)})
                print(line, flush=True)
                lines.append(line)
            del X, Y
        del Wf, images
    for bits, by_m in faster.items():
        L = 0
        for M in MS:
            if not all(by_m[M]):
                break
            L = M
        line = json.dumps({"bench": "quant_linear", "bits": bits, "L": L, "rule": c.quant_linear_rows_rule(bits),
                           "rows_faster_at": {str(M): all(v) for M, v in by_m.items()}})
        print(line, flush=True)
        lines.append(line)
    dev.sync()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
