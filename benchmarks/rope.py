"""Rotary position embedding, HIP events on the compute stream (warm-up, windows of at least `min_ms`, the best of three), all in ONE
process on one device:

  kernels (through the C ABI), in place over the Q|K blocks of a packed (rows, 3 d) projection output, H = 16, dh = 64:
    sizes     1 GiB of Q|K (rows = 2^17, d = 1024), the C5 module's own shape (B*S = 32 * 1024 rows, d = 1024), and a decode step
              (T = 1, B*H in {16, 64, 512}: rows = B, with a start array)
    families  both pairings; the vector family (16-byte accesses) and the scalar family (the same buffer entered one float off a
              16-byte boundary)
    copy      nk_copy of the same number of bytes, timed in alternation: `per_byte_ratio_to_copy` = ms of the rotation over ms of the
              copy.  Bytes counted: read + write of the rotated block, 2 * rows * 2 d * 4 (the copy moves that many: half read, half
              written).  The table row of a position (rot floats) is shared by all heads of the row and is not counted.
  module (through the tape), the C5 shape d_model = 1024, H = 16, S = 1024, B = 32, packed causal, p = 0.1:
    forward + backward of one step with `rope` set and unset, alternating; forward_step of one token (B = 8, 1024 positions
    prefilled) as the forward() of a node built once, with `rope` set and unset, alternating.

    python benchmarks/rope.py [--min-ms 25] [--out profiles/r17_rope.jsonl]
One JSON line per measurement, printed and written to `--out`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-ms", type=float, default=25.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_rope.jsonl"))
    ap.add_argument("--skip-module", action="store_true")
    ap.add_argument("--skip-large", action="store_true", help="leave the 1 GiB size out")
    args = ap.parse_args()

    import neuronika_amd
    from neuronika_amd import capi as c
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/rope.py needs a GPU")
    t = neuronika_amd.tape
    tdev = t.Device(0)
    dev = c.Device(handle=tdev.raw())
    rows_out = []

    def emit(row):
        rows_out.append(row)
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
        return timed(fn, max(4, int(args.min_ms / max(ms, 1e-4)) + 1))

    # ---- kernels ------------------------------------------------------------------------------------------------------------------
    H, dh, max_pos = 16, 64, 4096
    d = H * dh
    table = dev.zeros((max_pos, dh // 2, 2))
    c.rope_table(dev, table, max_pos, dh)
    sizes = [("c5_module", 32, 1024, None), ("decode_BH16", 1, 1, 1000), ("decode_BH64", 4, 1, 1000), ("decode_BH512", 32, 1, 1000)]
    if not args.skip_large:
        sizes.insert(0, ("1GiB_QK", 32, 4096, None))                    # 2^17 rows x 2 d floats = 1 GiB
    for label, B, T, first in sizes:
        rows = B * T
        nbytes = 2 * rows * 2 * d * 4
        whole = dev.zeros((rows * 3 * d + 4,))                           # one float of slack: the misaligned entry of the same buffer
        whole.fill(0.25)
        start = None if first is None else dev.int_array(np.full(B, first, dtype=np.int32))
        SRC, DST = dev.zeros((nbytes // 8,)), dev.zeros((nbytes // 8,))
        copy = lambda: c.check(c.lib.nk_copy(dev.h, DST.p, SRC.p, nbytes // 8))
        for family, off in (("vector", 0), ("scalar", 1)):
            buf = whole.view_offset(off)
            for il in (False, True):
                fwd = lambda: c.rope_fwd(dev, buf, 3 * d, buf, 3 * d, table, start, B, T, 2 * H, dh, dh, max_pos, il)
                bwd = lambda: c.rope_bwd(dev, buf, 3 * d, buf, 3 * d, table, start, B, T, 2 * H, dh, dh, max_pos, il, assign=True)
                ms_c, ms_f, ms_b = [], [], []
                for _ in range(3):
                    ms_c.append(window(copy)); ms_f.append(window(fwd)); ms_b.append(window(bwd))
                cp, fw, bw = min(ms_c), min(ms_f), min(ms_b)
                emit({"bench": "rope", "part": "kernels", "size": label, "rows": rows, "heads_in_launch": 2 * H, "dh": dh, "ld": 3 * d,
                      "family": family, "pairing": "interleaved" if il else "half-split", "algorithmic_bytes": nbytes,
                      "working_set_MB": round(rows * 3 * d * 4 / 2 ** 20, 1), "fwd_ms": round(fw, 5), "fwd_windows": [round(v, 5) for v in ms_f],
                      "bwd_assign_ms": round(bw, 5), "fwd_GBps": round(nbytes / (fw * 1e-3) / 1e9, 1), "copy_ms": round(cp, 5),
                      "copy_GBps": round(nbytes / (cp * 1e-3) / 1e9, 1), "per_byte_ratio_to_copy": round(fw / cp, 3)})
        del whole, SRC, DST, start

    # ---- module -------------------------------------------------------------------------------------------------------------------
    if not args.skip_module:
        dm, Hm, S, Bm = 1024, 16, 1024, 32
        rope = t.nn.RotaryEmbedding(tdev, dm // Hm, 2048)
        rng = np.random.default_rng(1)
        x = rng.random((Bm * S, dm), dtype=np.float32) - np.float32(0.5)
        g = t.from_ndarray(tdev, rng.random((Bm * S, dm), dtype=np.float32) - np.float32(0.5))
        steps = {}
        for name, r in (("plain", None), ("rope", rope)):
            mha = t.nn.MultiheadAttention(tdev, dm, Hm, 0.1, 3)
            mha.causal = True
            mha.rope = r
            X = t.from_ndarray(tdev, x).requires_grad()
            y = mha.forward(X, Bm)
            assert y.history_len() == 2                                  # the packed node + the output projection, with and without

            leaves = [X] + [getattr(getattr(mha, n), w) for n in "qkvo" for w in ("weight", "bias")]

            def step(y=y, leaves=leaves):                               # benchmarks/mha_step_causal.py's step
                y.forward()
                y.no_grad(); y.with_grad()
                y.backward_from(g)
                for p in leaves:
                    p.zero_grad()
            steps[name] = step
        a, b = [], []
        for _ in range(3):
            a.append(window(steps["plain"])); b.append(window(steps["rope"]))
        emit({"bench": "rope", "part": "module_fwd_bwd", "d_model": dm, "heads": Hm, "seq": S, "batch": Bm, "p": 0.1, "causal": True,
              "plain_ms": round(min(a), 4), "plain_windows": [round(v, 4) for v in a], "rope_ms": round(min(b), 4),
              "rope_windows": [round(v, 4) for v in b], "rope_share": round((min(b) - min(a)) / min(b), 4)})
        del steps, y, X
        Bd, n0 = 8, 1024
        prefix = rng.random((Bd * (n0 + 1), dm), dtype=np.float32) - np.float32(0.5)
        rows_of = lambda lo, hi: np.ascontiguousarray(np.concatenate([prefix[b * (n0 + 1) + lo:b * (n0 + 1) + hi] for b in range(Bd)]))
        nodes = {}
        for name, r in (("plain", None), ("rope", rope)):
            mha = t.nn.MultiheadAttention(tdev, dm, Hm, 0.0, 3)
            mha.causal = True
            mha.drop.eval()
            mha.rope = r
            cache = t.nn.KvCache(tdev, Bd, Hm, dm // Hm, n0 + 8)
            mha.forward_step(t.from_ndarray(tdev, rows_of(0, n0)), Bd, cache).forward()
            nodes[name] = mha.forward_step(t.from_ndarray(tdev, rows_of(n0, n0 + 1)), Bd, cache)     # forward() again and again
        a, b = [], []
        for _ in range(3):
            a.append(window(nodes["plain"].forward)); b.append(window(nodes["rope"].forward))
        emit({"bench": "rope", "part": "module_forward_step", "d_model": dm, "heads": Hm, "batch": Bd, "prefilled": n0, "T": 1,
              "plain_ms": round(min(a), 4), "plain_windows": [round(v, 4) for v in a], "rope_ms": round(min(b), 4),
              "rope_windows": [round(v, 4) for v in b], "rope_share": round((min(b) - min(a)) / min(b), 4)})
    dev.sync()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows_out:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
