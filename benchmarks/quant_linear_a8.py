"""nk_quant_a8_linear_fwd (int8 activations on v_mfma_i32_16x16x64_i8) against nk_quant_linear_fwd by rule and the f32 nk_linear_fwd, HIP
events on the compute stream, at the projection shapes of a 7B-class model:
    (N, K) = (4096, 4096)  and  (11008, 4096),   M in {16, 128, 512, 2048, 8192},   bits in {8, 4},   group 128
    python benchmarks/quant_linear_a8.py [min_ms]          # appends to profiles/quant_linear_a8.jsonl as well
Every timed loop ROTATES over enough distinct weight buffers that the working set exceeds twice the 256 MiB last-level cache, as
benchmarks/quant_linear.py does.  Per (shape, M, format), in alternation in one process, two rounds, the best window of each:
    a8_ms        the whole new entry (row quantiser + GEMM kernel)
    a8_gemm_ms   its GEMM kernel alone: the mean of the event pairs that nk_profile_begin / nk_profile_end put around that launch
                 (class KERNEL_QUANT_A8), taken in a separate instrumented pass so that the pairs do not sit in a8_ms
    a8_quant_ms  a8_ms - a8_gemm_ms: the row quantiser and the gap between the two launches
    rule_ms      nk_quant_linear_fwd by rule (rows / fused-dequant MFMA / unpack + f32 GEMM, whatever (M, bits) selects)
    f32_ms       nk_linear_fwd over f32 weights
    a8_gemm_TOPs 2 M N K / a8_gemm_ms: achieved int8 operations per second of the GEMM kernel."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuronika_amd import capi as c  # noqa: E402

SHAPES = [(4096, 4096), (11008, 4096)]
MS = [16, 128, 512, 2048, 8192]
VARIANTS = [(8, 128), (4, 128)]
WORKING_SET = 2 * (256 << 20)
OUT = os.path.join(ROOT, "profiles", "quant_linear_a8.jsonl")


def main():
    min_ms = float(sys.argv[1]) if len(sys.argv) > 1 else 10.0
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/quant_linear_a8.py needs a GPU")
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

    def kernel_ms(fn, iters=8):
        dev.profile_begin()
        for _ in range(iters):
            fn()
        n, ms, _ = dev.profile_end(c.KERNEL_QUANT_A8)
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
            imgs = []
            for i in range(WORKING_SET // (N * K * bits // 8) + 1):
                qw, sc = dev.zeros((c.quant_linear_words(N, K, bits),)), dev.zeros((c.quant_linear_scales(N, K, group),))
                c.quant_linear_pack(dev, Wf[i % len(Wf)], K, qw, sc, N, K, bits, group)
                imgs.append((qw, sc))
            images[(bits, group)] = imgs
        for M in MS:
            X, Y = dev.array(rng.standard_normal((M, K), dtype=np.float32)), dev.zeros((M, N))
            f32 = rotating(lambda W: c.linear_fwd(dev, X, W, bias, Y), Wf)
            best = {}
            for _ in range(2):
                for bits, group in VARIANTS:
                    imgs = images[(bits, group)]
                    a8 = rotating(lambda img: c.quant_a8_linear_fwd(dev, X, K, img[0], img[1], bias, Y, N, M, N, K, bits, group), imgs)
                    rule = rotating(lambda img: c.quant_linear_fwd(dev, X, K, img[0], img[1], bias, Y, N, M, N, K, bits, group), imgs)
                    for key, ms in (("f32",  window(f32)), ((bits, "a8"), window(a8)), ((bits, "gemm"), kernel_ms(a8)), ((bits, "rule"), window(rule))):
                        best[key] = min(best.get(key, 1e9), ms)
            for bits, group in VARIANTS:
                a8_ms, gemm_ms, rule_ms = best[(bits, "a8")], best[(bits, "gemm")], best[(bits, "rule")]
                line = json.dumps({"bench": "quant_linear_a8", "N": N, "K": K, "M": M, "bits": bits, "group": group, "weight_buffers": len(images[(bits, group)]),
                                   "a8_ms": round(a8_ms, 5), "a8_gemm_ms": round(gemm_ms, 5), "a8_quant_ms": round(a8_ms - gemm_ms, 5),
                                   "a8_gemm_TOPs": round(2.0 * M * N * K / (gemm_ms * 1e-3) / 1e12, 2), "rule_ms": round(rule_ms, 5),
                                   "f32_ms": round(best["f32"], 5), "rule_over_a8": round(rule_ms / a8_ms, 3), "f32_over_a8": round(best["f32"] / a8_ms, 3)})
                print(line, flush=True)
                lines.append(line)
            del X, Y
        del Wf, images
    dev.sync()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
