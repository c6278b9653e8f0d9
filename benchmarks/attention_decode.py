"""Incremental decoding, HIP events on the compute stream (warm-up, windows of at least `min_ms`, the best of three), all in ONE
process on one device:

  kernels (through the C ABI), T = 1, B*H in {16, 64, 512}, n in {128, 1024, 4096, 16384} cached keys, dh in {64, 128}, cap = n
    decode          nk_attention_decode_fwd alone (partial launch + combine launch when n exceeds one chunk)
    append_decode   nk_kv_cache_append of the new row + nk_attention_decode_fwd: what a layer issues per token
    copy            nk_copy of the same number of bytes, timed in alternation: `per_byte_ratio_to_copy` = (ms / bytes) of decode over
                    (ms / bytes) of the copy (above 1: slower per byte moved than the copy).  Bytes counted: the K and V the step has
                    to read, 2 * B*H * n * dh * 4 (the copy moves that many bytes: half read, half written).
    recompute       the only alternative without a cache: nk_attention_causal_fwd in inference form over all n positions of the same
                    B*H problems (for ONE new token).  Where the library refuses the geometry in one call (its 2^31 guards), it runs as
                    several calls over fewer problems and the times add up; `recompute_calls` says how many.  Long calls are timed
                    singly (one warm-up, the best of two) rather than in windows.
    `working_set_MB` is K + V: at or below the 256 MB Infinity Cache a repeated call is cache-assisted, and the row says so.
  module (through the tape), d_model = 1024, H = 16, B = 8, from a prefilled length of 1024
    forward_step of one token (tokens/s = B / time) against `forward()` over the whole prefix of 1025 positions: both as the forward()
    of a node built once, so building the node (its allocations, the blocking upload of the B start positions) is not in the time.
  long cache: cap = 16384 with n = 128 / 1024 keys in it against cap = n - what the blocks past the length cost (the grid is sized by cap)

    python benchmarks/attention_decode.py [--min-ms 25] [--out profiles/r16_attention_decode.jsonl]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_attention_decode.jsonl"))
    ap.add_argument("--problems", type=int, nargs="*", default=[16, 64, 512], help="B*H values")
    ap.add_argument("--lengths", type=int, nargs="*", default=[128, 1024, 4096, 16384])
    ap.add_argument("--head-sizes", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--skip-module", action="store_true")
    args = ap.parse_args()

    import neuronika_amd
    from neuronika_amd import capi as c
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/attention_decode.py needs a GPU")
    t = neuronika_amd.tape
    tdev = t.Device(0)
    dev = c.Device(handle=tdev.raw())
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
        return timed(fn, max(4, int(args.min_ms / max(ms, 1e-4)) + 1))

    def best(fn, heavy_ms=20.0):
        first = timed(fn, 1)                                             # warm-up
        if first > heavy_ms:
            return min(timed(fn, 1), timed(fn, 1)), "single calls"
        return min(window(fn) for _ in range(3)), "windows"

    # ---- kernels ------------------------------------------------------------------------------------------------------------------
    H = 16
    for dh in args.head_sizes:
        scale = float(np.float32(1.0 / np.sqrt(dh)))
        chunk = c.attention_decode_chunk(dh)
        for bh in args.problems:
            B = bh // H
            for n in args.lengths:
                cap, d = n, H * dh
                nbytes = 2 * bh * n * dh * 4
                Kc, Vc = dev.full((B, H, cap, dh), 0.01), dev.full((B, H, cap, dh), 0.02)
                qkv = dev.array(np.random.default_rng(0).random((B, 3 * d), dtype=np.float32) - np.float32(0.5))
                start = dev.int_array(np.full(B, n - 1, dtype=np.int32))
                out = dev.zeros((B, d))
                ws = dev.zeros((c.attention_decode_workspace(B, 1, H, dh, cap),))
                SRC, DST = dev.zeros((nbytes // 8,)), dev.zeros((nbytes // 8,))
                copy = lambda: c.check(c.lib.nk_copy(dev.h, DST.p, SRC.p, nbytes // 8))
                decode = lambda: c.attention_decode_fwd(dev, qkv, 3 * d, Kc, Vc, start, out, ws, B, 1, H, dh, cap, scale)

                def append_decode():
                    c.kv_cache_append(dev, Kc, Vc, qkv.view_offset(d), qkv.view_offset(2 * d), 3 * d, start, B, 1, H, dh, cap)
                    decode()

                ms_c, ms_d, ms_a = [], [], []
                for _ in range(3):
                    ms_c.append(window(copy)); ms_d.append(window(decode)); ms_a.append(window(append_decode))
                cp, dc, ad = min(ms_c), min(ms_d), min(ms_a)
                del SRC, DST
                # the same token without a cache: the causal core over all n positions, H = 1 layout (bh * n, dh)
                per = bh
                while per > 1 and (per * (((n + 31) // 32) ** 2) >= (1 << 31) // 32 or per * n * dh >= (1 << 31)):
                    per //= 2
                Q, K, V, O = (dev.full((per * n, dh), v) for v in (0.01, 0.01, 0.02, 0.0))
                ncalls = bh // per

                def recompute():
                    for _ in range(ncalls):
                        c.attention_fwd(dev, Q, K, V, None, None, None, O, per, n, 1, dh, scale, 0.0, False, causal=True)

                rc, how = best(recompute)
                del Q, K, V, O
                emit({"bench": "attention_decode", "part": "kernels", "BH": bh, "n": n, "dh": dh, "T": 1, "chunk": chunk,
                      "chunks_per_problem": (n + chunk - 1) // chunk, "algorithmic_bytes": nbytes, "working_set_MB": round(nbytes / 2 ** 20, 1),
                      "cache_assisted": nbytes <= 256 * 2 ** 20, "decode_ms": round(dc, 5), "decode_windows": [round(v, 5) for v in ms_d],
                      "append_decode_ms": round(ad, 5), "decode_GBps": round(nbytes / (dc * 1e-3) / 1e9, 1), "copy_ms": round(cp, 5),
                      "copy_GBps": round(nbytes / (cp * 1e-3) / 1e9, 1), "per_byte_ratio_to_copy": round(dc / cp, 3),
                      "recompute_ms": round(rc, 4), "recompute_calls": ncalls, "recompute_timing": how,
                      "recompute_GFLOP": round(2.0 * bh * n * (n + 1) * dh / 1e9, 2), "recompute_over_decode": round(rc / dc, 1)})
                del Kc, Vc, qkv, start, out, ws

    # ---- a cache much longer than its contents: the grid is sized by cap, blocks past the length return at once ---------------------
    for bh, n, cap, dh in ((64, 128, 16384, 64), (64, 1024, 16384, 64), (16, 128, 16384, 128)):
        B, d, scale = bh // H, H * dh, float(np.float32(1.0 / np.sqrt(dh)))
        res = {}
        for label, cp_ in (("cap_equal_n", n), ("cap_long", cap)):
            Kc, Vc = dev.full((B, H, cp_, dh), 0.01), dev.full((B, H, cp_, dh), 0.02)
            qkv = dev.array(np.random.default_rng(0).random((B, 3 * d), dtype=np.float32) - np.float32(0.5))
            start = dev.int_array(np.full(B, n - 1, dtype=np.int32))
            out = dev.zeros((B, d))
            ws = dev.zeros((c.attention_decode_workspace(B, 1, H, dh, cp_),))
            fn = lambda: c.attention_decode_fwd(dev, qkv, 3 * d, Kc, Vc, start, out, ws, B, 1, H, dh, cp_, scale)
            res[label] = min(window(fn) for _ in range(3))
            del Kc, Vc, qkv, start, out, ws
        chunk = c.attention_decode_chunk(dh)
        emit({"bench": "attention_decode", "part": "long_cache", "BH": bh, "n": n, "cap": cap, "dh": dh,
              "blocks_launched": bh * ((cap + chunk - 1) // chunk), "blocks_with_keys": bh * ((n + chunk - 1) // chunk),
              "decode_ms_cap_equal_n": round(res["cap_equal_n"], 5), "decode_ms_cap_long": round(res["cap_long"], 5),
              "long_over_equal": round(res["cap_long"] / res["cap_equal_n"], 2)})

    # ---- module -------------------------------------------------------------------------------------------------------------------
    if not args.skip_module:
        d, Hm, Bm, n0 = 1024, 16, 8, 1024
        mha = t.nn.MultiheadAttention(tdev, d, Hm, 0.0, 3)
        mha.causal = True
        mha.drop.eval()
        rng = np.random.default_rng(1)
        prefix = (rng.random((Bm * (n0 + 1), d), dtype=np.float32) - np.float32(0.5))
        rows_of = lambda lo, hi: np.ascontiguousarray(np.concatenate([prefix[b * (n0 + 1) + lo:b * (n0 + 1) + hi] for b in range(Bm)]))
        cache = t.nn.KvCache(tdev, Bm, Hm, d // Hm, n0 + 8)
        y = mha.forward_step(t.from_ndarray(tdev, rows_of(0, n0)), Bm, cache)
        y.forward()
        step = mha.forward_step(t.from_ndarray(tdev, rows_of(n0, n0 + 1)), Bm, cache)   # the node of token 1025: forward() again and again
        full = mha.forward(t.from_ndarray(tdev, prefix).requires_grad(), Bm)
        a, b = [], []
        for _ in range(3):
            a.append(window(step.forward)); b.append(window(full.forward))
        emit({"bench": "attention_decode", "part": "module", "d_model": d, "heads": Hm, "batch": Bm, "prefilled": n0,
              "forward_step_ms": round(min(a), 4), "forward_step_windows": [round(v, 4) for v in a],
              "tokens_per_s": round(Bm / (min(a) * 1e-3), 1), "forward_whole_prefix_ms": round(min(b), 4),
              "forward_whole_prefix_windows": [round(v, 4) for v in b], "tokens_per_s_by_recompute": round(Bm / (min(b) * 1e-3), 1),
              "forward_over_forward_step": round(min(b) / min(a), 1)})
    dev.sync()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
