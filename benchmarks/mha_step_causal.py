"""The C5 module step (MultiheadAttention d=1024 h=16 S=1024 B=32, dropout 0.1, fwd + bwd) with `mha.causal` off and on, alternating
in one process: ms per step, sequences/s and TFLOP/s of both, and the causal / full ratio of the best times.
    python benchmarks/mha_step_causal.py [steps] [rounds]
The step is bench.py's `--workload mha` step (same module, seeds, inputs, loop body); bench.py has no switch for the causal form,
so its headline line stays what it was and this script gives the pair.  Flops: 1.237e12 per full step (412.3 GFLOP
forward, twice that backward), of which the attention core is a third, 12*B*H*S*S*dh; the causal form needs the S*(S+1)/2
(query, key) pairs on and below the diagonal of those."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import neuronika_amd  # noqa: E402


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    t = neuronika_amd.tape
    dev = t.Device(0)
    B, S, d, H = 32, 1024, 1024, 16
    X = t.from_ndarray(dev, np.random.default_rng(0).random((B * S, d), dtype=np.float32)).requires_grad()
    G = t.from_ndarray(dev, np.random.default_rng(5).random((B * S, d), dtype=np.float32))
    full_flop = 1.237e12
    flop = {False: full_flop, True: full_flop - 12.0 * B * H * S * S * (d // H) * (1.0 - (S + 1) / (2.0 * S))}

    def build(causal):
        t.manual_seed(7)
        mha = t.nn.MultiheadAttention(dev, d, H, 0.1, 1)
        mha.causal = causal
        y = mha.forward(X, B)
        leaves = [X] + [getattr(getattr(mha, n), w) for n in "qkvo" for w in ("weight", "bias")]

        def step():
            y.forward()
            y.no_grad(); y.with_grad()
            y.backward_from(G)
            for p in leaves:
                p.zero_grad()
        return step

    variants = {False: build(False), True: build(True)}
    best = {}
    for _ in range(rounds):
        for causal in (False, True):
            step = variants[causal]
            for _ in range(3):
                step()
            dev.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            dev.sync()
            ms = (time.perf_counter() - t0) / steps * 1e3
            best[causal] = min(best.get(causal, ms), ms)
            print(json.dumps({"workload": "C5: MHA d_model=1024 heads=16 seq=1024 batch=32 dropout=0.1" + (", causal" if causal else ""),
                              "steps": steps, "ms_per_step": round(ms, 4), "sequences_per_s": round(B / ms * 1e3, 1),
                              "step_tflops": round(flop[causal] / ms / 1e9, 2)}), flush=True)
    print(json.dumps({"best_ms_full": round(best[False], 4), "best_ms_causal": round(best[True], 4),
                      "causal_over_full_step": round(best[True] / best[False], 3)}), flush=True)


if __name__ == "__main__":
    main()
