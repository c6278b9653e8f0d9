"""nk_quant_mx_linear_fwd (MXFP4 weights x MXFP8 rows on v_mfma_scale_f32_16x16x128_f8f6f4) against nk_quant_a8_linear_fwd (int4 weights,
group 64, int8 activations) and, at M <= 8, nk_quant_linear_fwd (int4, the decode rows kernels), HIP events on the compute stream:
    (N, K) = (4096, 4096)  and  (14336, 4096),   M in {1, 8, 16, 64, 512, 2048, 8192}
    python benchmarks/quant_linear_mx.py [min_ms]          # appends to profiles/quant_linear_mx.jsonl as well
Every timed loop ROTATES over enough distinct weight buffers that the working set exceeds twice the 256 MiB last-level cache, as
benchmarks/quant_linear_a8.py does.  Per (shape, M), in alternation in one process, every call warmed, two rounds, the best window of each:
    mx_ms        the whole new entry (row quantiser + GEMM kernel)
    mx_gemm_ms   its GEMM kernel alone: the mean of the event pairs that nk_profile_begin / nk_profile_end put around that launch
                 (class KERNEL_QUANT_MX), taken in a separate instrumented pass
    mx_quant_ms  mx_ms - mx_gemm_ms: the row quantiser and the gap between the two launches
    a8_ms, a8_gemm_ms   the same two figures of nk_quant_a8_linear_fwd;  w4_ms  nk_quant_linear_fwd (M <= 8 only)
    mx_gemm_TOPs 2 M N K / mx_gemm_ms;  mx_weight_GBs (M <= 16) the bytes of codes and scales, N K (1 / 2 + 1 / 32), over mx_gemm_ms
    bound        which of the two floors of the GEMM kernel is the higher one at this shape: "weights" (those bytes at 8 TB/s) or "mfma"
                 (2 M N K at the 5 PFLOP/s dense fp8 rate of the data sheet; the mixed fp8 x fp4 rate of the instruction is what
                 mx_gemm_TOPs measures)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuronika_amd import capi as c  # noqa: E402

SHAPES = [(4096, 4096), (14336, 4096)]
MS = [1, 8, 16, 64, 512, 2048, 8192]
WORKING_SET = 2 * (256 << 20)
HBM_BYTES_PER_S, MFMA_OPS_PER_S = 8.0e12, 5.0e15
OUT = os.path.join(ROOT, "profiles", "quant_linear_mx.jsonl")


def main():
    min_ms = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/quant_linear_mx.py needs a GPU")
    dev = c.Device(0)

    def window(fn):
        fn(); fn()
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

    def kernel_ms(fn, klass, iters=8):
        dev.profile_begin()
        for _ in range(iters):
            fn()
        n, ms, _ = dev.profile_end(klass)
        assert n == iters, (n, iters)
        return ms / n

    def rotating(call, bufs):
        state = [0]

        def fn():
            call(bufs[state[0] % len(bufs)])
            state[0] += 1
        return fn

    lines = []
    rng = np.random.default_rng(0)
    for N, K in SHAPES:
        W = dev.array(rng.standard_normal(N * K, dtype=np.float32) * np.float32(0.02))
        bias = dev.array(rng.standard_normal(N, dtype=np.float32))
        mx_imgs, i4_imgs = [], []
        for _ in range(WORKING_SET // (N * K // 2) + 1):
            qw, sw = dev.zeros((c.quant_mx_words(N, K),)), dev.zeros((c.quant_mx_scales(N, K),))
            c.quant_mx_pack(dev, W, K, qw, sw, N, K)
            mx_imgs.append((qw, sw))
            q4, s4 = dev.zeros((c.quant_linear_words(N, K, 4),)), dev.zeros((c.quant_linear_scales(N, K, 64),))
            c.quant_linear_pack(dev, W, K, q4, s4, N, K, 4, 64)
            i4_imgs.append((q4, s4))
        del W
        for M in MS:
            X, Y = dev.array(rng.standard_normal((M, K), dtype=np.float32)), dev.zeros((M, N))
            mx = rotating(lambda img: c.quant_mx_linear_fwd(dev, X, K, img[0], img[1], bias, Y, N, M, N, K), mx_imgs)
            a8 = rotating(lambda img: c.quant_a8_linear_fwd(dev, X, K, img[0], img[1], bias, Y, N, M, N, K, 4, 64), i4_imgs)
            w4 = rotating(lambda img: c.quant_linear_fwd(dev, X, K, img[0], img[1], bias, Y, N, M, N, K, 4, 64), i4_imgs)
            best = {}
            for _ in range(2):
                runs = [("mx", lambda: window(mx)), ("mx_gemm", lambda: kernel_ms(mx, c.KERNEL_QUANT_MX)), ("a8", lambda: window(a8)),
                        ("a8_gemm", lambda: kernel_ms(a8, c.KERNEL_QUANT_A8))] + ([("w4", lambda: window(w4))] if M <= 8 else [])
                for key, run in runs:
                    best[key] = min(best.get(key, 1e9), run())
            ops, wbytes = 2.0 * M * N * K, N * K * (0.5 + 1.0 / 32)
            rec = {"bench": "quant_linear_mx", "N": N, "K": K, "M": M, "weight_buffers": len(mx_imgs), "mx_ms": round(best["mx"], 5),
                   "mx_gemm_ms": round(best["mx_gemm"], 5), "mx_quant_ms": round(best["mx"] - best["mx_gemm"], 5),
                   "mx_gemm_TOPs": round(ops / (best["mx_gemm"] * 1e-3) / 1e12, 3), "a8_ms": round(best["a8"], 5),
                   "a8_gemm_ms": round(best["a8_gemm"], 5), "a8_over_mx": round(best["a8"] / best["mx"], 3),
                   "bound": "weights" if wbytes / HBM_BYTES_PER_S > ops / MFMA_OPS_PER_S else "mfma"}
            if M <= 16:
                rec["mx_weight_GBs"] = round(wbytes / (best["mx_gemm"] * 1e-3) / 1e9, 1)
            if M <= 8:
                rec.update(w4_ms=round(best["w4"], 5), w4_over_mx=round(best["w4"] / best["mx"], 3))
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            del X, Y
        del mx_imgs, i4_imgs
    dev.sync()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
