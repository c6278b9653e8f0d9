"""Inventory of the kernel instantiations of the three MFMA translation units - nk_gemm.hip, nk_conv.hip (with every nk_conv_*.h it
includes) and nk_attention.hip - and of the test that reaches each one, in the format of tests/dispatch_paths.py.

One row per instantiation, named as a kernel trace summary prints it (tools/rocpd_kernel_stats.py), with the entry point(s), the
dispatch condition read off the dispatcher, and exactly one of

    tests=(...)         ids in tests/test_gpu_dispatch_paths_mfma.py that enter it
    covered_by="..."    a test elsewhere in the suite that enters it
    unreachable="..."   why no call this suite may make can launch it

The template grids are regular, so entry and condition are composed from the template arguments (`_describe`); which test enters a
kernel is not composed but MEASURED: `_REACHED` was written from kernel traces of the GPU suite, one test file per traced process,
each launch attributed to the test that was running (profiles/r11_suite_kernels_entered.md for the suite as it was,
profiles/r11_mfma_dispatch_paths_kernels.md for the new file).  tests/test_dispatch_inventory.py compares the rows with the code
object of the built library, with the collected test ids and with the new file's trace: a new instantiation needs a row.

NOT_INVENTORIED names the translation units that have no inventory yet; every kernel of the library belongs to an inventoried unit
or to one of these (tests/test_dispatch_inventory.py::test_every_kernel_of_the_library_is_accounted_for)."""
import re
from collections import namedtuple

UNITS = ("nk_gemm.hip", "nk_conv.hip", "nk_attention.hip")
TEST_FILE = "tests/test_gpu_dispatch_paths_mfma.py"
TRACE_SUMMARY = "profiles/r11_mfma_dispatch_paths_kernels.md"

NOT_INVENTORIED = (
    ("nk_batchnorm.hip", "32 instantiations; tests/test_gpu_batchnorm.py is written from shapes, its dispatch branches are not listed yet"),
    ("nk_pool.hip", "38 instantiations (window / index-width / kernel-size templates); tests/test_gpu_pooling.py is written from shapes"),
    ("nk_norm.hip", "230 instantiations: the LayerNorm and RMSNorm row kernels, embedding, cross entropy, activations and GLU, the "
                    "multi-tensor optimizer, rope, sampling, band attention and every decode and paged-cache kernel; their test files "
                    "(tests/test_gpu_layernorm.py, test_gpu_rms_norm.py, test_gpu_rope.py, ...) are written from shapes"),
    ("nk_comm.hip", "2 replica-sum kernels; they run under a communicator only (tests/test_gpu_multi.py needs two GPUs)"),
    ("nk_runtime.hip", "1 copy kernel (nk_copy from 1 Mi floats on); entered by tests/test_gpu_parity.py, no dispatch grid to list"),
)

_Row = namedtuple("Row", "kernel entry condition tests covered_by unreachable")


def Row(kernel, entry, condition, tests=(), covered_by=None, unreachable=None):
    return _Row(kernel, entry, condition, tuple(tests), covered_by, unreachable)


def _split(kernel):
    fn, _, rest = kernel.partition("<")
    return fn, [a.strip() for a in rest.rstrip(">").split(",")] if rest else []


_LAYOUT = {("false", "false"): "NN", ("false", "true"): "NT", ("true", "false"): "TN", ("true", "true"): "TT"}
_TI_M = {"1": "Mg <= 64 or Mg % 128 == 64 (64-row tiles)", "2": "Mg > 64 and not Mg % 128 == 64 (128-row tiles)"}
_TI_C = {"1": "Cg <= 64 or Cg % 128 == 64 (64-row tiles)", "2": "Cg > 64 and not Cg % 128 == 64 (128-row tiles)"}
_TAPS = {("3", "3"): "3 x 3 taps", ("5", "5"): "5 x 5 taps", ("1", "3"): "1 x 3 taps", ("0", "0"): "any other tap count (run-time loops)"}
_CONV_FWD = "nk_conv_fwd, nk_conv_bias_fwd, nk_conv_bias_fwd_padded (copied padding)"
_CONV_DX = "nk_conv_bwd_input[_assign], nk_conv_bwd_input_padded[_assign]"
_CONV_DW = "nk_conv_bwd_kernel[_assign], nk_conv_bwd_kernel_bias, nk_conv_bwd_kernel_bias_padded (copied padding)"
_DIRECT = "use_direct: Cg <= 16 and Mg <= 16"
_NOT_SPECIAL = "not direct, not taken by the Winograd / stride-2 tap-plane kernels"


def _gemm(fn, a):
    if fn == "sgemm_kernel":
        ta, tb, al, ti, tj, kg, epx = a
        lay = _LAYOUT[ta, tb]
        entry = {"NN": "nk_sgemm[_batched], nk_mm_fwd, nk_mm_t_bwd_left; EPX: nk_linear_bwd_input_relu",
                 "NT": "nk_sgemm[_batched], nk_mm_t_fwd, nk_mm_bwd_left, nk_linear_fwd, nk_linear_relu_fwd",
                 "TN": "nk_sgemm[_batched], nk_mm_bwd_right, nk_mm_t_bwd_right, the two-launch route of nk_sgemm_pair[_batched]",
                 "TT": "nk_sgemm[_batched]"}[lay]
        cond = f"gemm_impl -> launch<{ta}, {tb}>: layout {lay}; tile {64 * int(ti)} x {64 * int(tj)} by the block-count rules or NK_TUNE_GEMM_FORCE; "
        cond += ("ALIGNED: M, N whole tiles, K % 32 == 0, lda / ldb / batch strides % 4 == 0, A and B 16-byte aligned" if al == "true"
                 else "guarded loader: a ragged M / N / K, a leading dimension % 4 != 0 or an offset A / B")
        if kg == "2":
            cond += "; k-pair block: ALIGNED, one tile per block, an even number >= 8 of whole k-tiles; by rule a grid of at most one block per CU with >= 32 (64 x 64: 16) k-tiles, or NK_TUNE_GEMM_KPAIR > 0"
        cond += ("; EPX: " + ("every NT launch" if lay == "NT" else "a ReLU or mask epilogue")) if epx == "true" else "; plain epilogue (no ReLU, no mask)"
        return entry, cond
    if fn == "sgemm_pair_kernel":
        lay = _LAYOUT[a[0], a[1]]
        return ("nk_sgemm_pair[_batched], nk_mm_bwd, nk_mm_t_bwd, nk_attention[_qkv][_causal]_bwd (dK / dV)",
                f"gemm_pair_impl: first problem {lay}, second TN, both ALIGNED, unsplit, one tile per block, the same {64 * int(a[4])} x {64 * int(a[5])} tile, "
                "no output overlapping the other problem; by rule when both grids fit the resident slots together, NK_TUNE_GEMM_PAIR = 1 whenever eligible")
    if fn == "sgemm_tail_kernel":
        lay = _LAYOUT[a[0], a[1]]
        return ("nk_sgemm, nk_linear_fwd, nk_linear_relu_fwd, nk_linear_bwd_input_relu, the MatMul wrappers - after nk_device_set_busy_slots(n > 0)",
                f"gemm_tail_launch: layout {lay}, 128 x 128 tiles by rule (no forced configuration), ALIGNED, unsplit, unbatched, 256-thread blocks; the tile "
                "count is above the free slots (2 * CUs - busy >= CUs), leaves a ragged last round and >= 4 k-pieces per left-over tile; "
                + ("EPX: NT, ReLU or mask" if a[2] == "true" else "plain epilogue"))
    if fn == "splitk_reduce_kernel":
        return ("every split-K launch of gemm_impl, every sgemm_tail launch",
                "splits > 1 and C is not one dense block (ldc != N, N % 4 != 0, an offset C / bias / mask, strided batches); always for the rectangle of gemm_tail_launch")
    assert fn == "splitk_reduce_flat_kernel", fn
    return ("every split-K launch of gemm_impl", "splits > 1 and C is one dense block: ldc == N, N % 4 == 0, C / bias / mask 16-byte aligned, batches back to back")


def _attention(fn, a):
    assert fn == "attention_kernel", fn
    bwd, masked, full, occ, keep, dh, ragged, causal = a
    c = "_causal" if causal == "true" else ""
    entry = f"nk_attention{c}_bwd, nk_attention_qkv{c}_bwd" if bwd == "true" else f"nk_attention{c}_fwd, nk_attention_qkv{c}_fwd"
    cond = f"attention_launch_dh: dh == {dh}; "
    cond += "S % 32 != 0 (RAGGED)" if ragged == "true" else ("S % 128 == 0 (FULL)" if full == "true" else "S % 32 == 0, S % 128 != 0")
    cond += "; training with 0 < p < 1 (MASKED)" if masked == "true" else "; evaluation or p == 0"
    if bwd == "false":
        cond += "; scores / stats kept (KEEP)" if keep == "true" else "; scores == NULL: inference, out only"
        if keep == "true" and causal == "false" and dh != "128":
            cond += "; NK_TUNE_ATTENTION_OCC == 2" if occ == "2" else "; NK_TUNE_ATTENTION_OCC != 2"
    return entry, cond


def _conv(fn, a):
    if fn == "conv_fwd_kernel":
        return _CONV_FWD, (f"generic forward: {_NOT_SPECIAL}, and Cg % 32 != 0 or last stride > 2 or out width < 4; {_TI_M[a[1]]}; "
                           + ("ALIGNED_A: Mg whole tiles, Cg * taps % 32 == 0, w aligned" if a[0] == "true" else "guarded weight loads") + "; "
                           + ("QUADV: last stride 1 and out width % 4 == 0" if a[2] == "true" else "scalar column gathers"))
    if fn == "conv_bwd_input_kernel":
        return _CONV_DX, (f"generic input gradient: {_NOT_SPECIAL}, and Mg % 32 != 0 or out width < 4 or more than 16 stride phases; {_TI_C[a[2]]}; "
                          + ("ALIGNED_A: Cg whole tiles, Mg * taps % 32 == 0" if a[0] == "true" else "guarded weight loads") + "; "
                          + ("every stride 1" if a[1] == "true" else "some stride > 1"))
    if fn == "conv_bwd_kernel_kernel":
        vg, ti, tj, q, sw = a
        stage = ("quad staging: last stride 2, out width >= 4" if sw == "2" else "quad staging: last stride 1, out width >= 4 (and not the mixed launch)" if q == "true"
                 else "no quad staging (last stride > 2 or out width < 4); " + ("L % 4 == 0 and gy aligned" if vg == "true" else "L % 4 != 0 or gy offset"))
        return _CONV_DW, f"kernel gradient, {_NOT_SPECIAL}: {_TI_M[ti]}; " + ("Cg * taps <= 64 (64 columns)" if tj == "1" else "Cg * taps > 64 (128 columns)") + "; " + stage
    if fn == "conv_bwd_kernel_mixed_kernel":
        return _CONV_DW, ("kernel gradient, mixed launch: quad staging, last stride 1, 128-column tiles with Cg * taps % 128 == 64, one group, the narrow tile's price "
                          f"(rule or NK_TUNE_CONV_NARROW) > 0 and its splits fewer than the wide ones; {_TI_M[a[1]]}")
    if fn == "conv_dw_reduce_kernel":
        return _CONV_DW, "after every direct or implicit-GEMM kernel gradient: sums the split slabs in order (and the fused bias slabs)"
    if fn == "conv_koff_kernel":
        return _CONV_FWD, "in front of every generic forward (offset table)"
    if fn in ("conv_ktab_kernel", "conv_wt_kernel"):
        return _CONV_DX, "in front of every generic input gradient (" + ("tap table" if fn == "conv_ktab_kernel" else "transposed weights") + ")"
    if fn == "conv_wp_kernel":
        return _CONV_FWD, "in front of every fast forward (tap-major weights, tap tables)"
    if fn == "conv_wq_tables_kernel":
        return _CONV_DX, "in front of every fast input gradient (re-laid weights, tap and phase tables)"
    if fn == "conv_fwd_fast_kernel":
        return _CONV_FWD, (f"fast forward: {_NOT_SPECIAL}, Cg % 32 == 0, last stride {a[3]}, out width >= 4; {_TI_M[a[1]]}; "
                           + ("Mg whole tiles" if a[0] == "true" else "Mg not whole tiles (guarded rows)") + "; "
                           + ("RP: out width % 4 != 0" if a[2] == "true" else "out width % 4 == 0"))
    if fn == "conv_fwd_tail_reduce_kernel":
        return _CONV_FWD, (f"fast forward, one group, >= 4 k-tiles: the tiles past the last whole round of 2 * CUs slots (or a grid of at most half of them) are cut "
                           f"along k; {a[0]}-row tiles")
    if fn == "conv_bwd_input_fast_kernel":
        return _CONV_DX, (f"fast input gradient: {_NOT_SPECIAL}, Mg % 32 == 0, out width >= 4, at most 16 stride phases; {_TI_C[a[1]]}; "
                          + ("Cg whole tiles" if a[0] == "true" else "Cg not whole tiles (guarded rows)"))
    if fn == "conv_bwd_input_tail_reduce_kernel":
        return _CONV_DX, f"fast input gradient, one group, one stride phase, >= 4 k-tiles: the ragged last round (or a small grid) cut along k; {a[0]}-row tiles"
    if fn == "conv_direct_fwd_rows_kernel":
        return _CONV_FWD, f"{_DIRECT}; two spatial dims, last stride and dilation 1, out width % 4 == 0, y aligned; {_TAPS[a[0], a[1]]}"
    if fn == "conv_direct_fwd_kernel":
        return _CONV_FWD, f"{_DIRECT}; not the rows form; " + ("L >= 512 (4 positions per thread)" if a[0] == "4" else "L < 512") + f"; {_TAPS[a[1], a[2]]}"
    if fn == "conv_direct_bwd_input_rows_kernel":
        return _CONV_DX, (f"{_DIRECT}; every stride 1, two spatial dims, last dilation 1, width % 4 == 0, dx aligned; {_TAPS[a[0], a[1]]}; "
                          + ("gy below 2 GiB (buffer descriptor)" if a[2] == "true" else "gy of 2 GiB or more (64-bit addresses)"))
    if fn == "conv_direct_bwd_input_strided_kernel":
        return _CONV_DX, f"{_DIRECT}; not the rows form, some stride > 1, every dilation 1; " + ("plane >= 512" if a[0] == "4" else "plane < 512")
    if fn == "conv_direct_bwd_input_kernel":
        return _CONV_DX, (f"{_DIRECT}; neither the rows nor the strided form; " + ("every stride 1" if a[0] == "true" else "some stride > 1 and some dilation > 1") + "; "
                          + ("plane >= 512" if a[1] == "4" else "plane < 512") + f"; {_TAPS[a[2], a[3]]}")
    if fn == "conv_direct_bwd_kernel_kernel":
        return _CONV_DW, f"{_DIRECT}; taps other than 3 x 3 / 5 x 5 in two dimensions: one block per (co, ci, tap)"
    if fn == "conv_direct_bwd_kernel_taps_kernel":
        return _CONV_DW, f"{_DIRECT}; two spatial dims, {_TAPS[a[0], a[1]]}: all taps of a (co, ci) pair per block"
    wino = "3 x 3, stride 1, dilation 1, one group, two spatial dims, aligned tensors below 2 GiB, not direct"
    if fn == "wino_weights_kernel":
        return f"{_CONV_FWD.split(' (')[0]} (folded padding too), {_CONV_DX}", f"in front of every wino_kernel launch ({wino})"
    if fn == "wino_kernel":
        return (f"{_CONV_FWD.split(' (')[0]} (folded padding too), {_CONV_DX}",
                f"wino_launch ({wino}): " + ("wide blocks: Cm % 128 == 0 and Ck % 32 == 0" if a[0] == "4" else "narrow blocks: Cm % 64 == 0, Ck % 16 == 0 and not wide")
                + ("; ODD: an odd destination extent" if len(a) > 4 and a[4] == "true" else "; even destination extents")
                + "; by rule from CUs / 8 wide (CUs narrow) blocks, NK_TUNE_CONV_WINOGRAD 1 whenever the shape allows, always with folded padding")
    if fn == "wino_dw_kernel":
        return (f"{_CONV_DW.split(' (')[0]} (folded padding)",
                f"wino_dw_launch ({wino}): Ci % 64 == 0, Co % 64 == 0, (Co / 64) * (Ci / 64) <= CUs, >= 16 items per slice by rule (knob: whenever the shape allows); "
                + ("FOLD: zero padding 1 folded in" if a[0] == "true" else "no folded padding") + ("; ODD: an odd output extent" if len(a) > 1 and a[1] == "true" else "; even output extents"))
    if fn == "wino_dw_reduce_kernel":
        return f"{_CONV_DW.split(' (')[0]} (folded padding)", "after every wino_dw_kernel launch: sums the slice slabs (and the bias slabs)"
    s2 = "3 x 3, stride 2, dilation 1, one group, two spatial dims, padding 0 or 1"
    if fn == "s2dx_weights_kernel":
        return _CONV_DX, f"in front of every s2dx_kernel launch ({s2})"
    if fn == "s2dx_kernel":
        return _CONV_DX, (f"s2dx_launch ({s2}, even H and W, dx aligned): " + ("wide blocks: Cin % 128 == 0, Cout % 32 == 0 and >= 8 blocks per CU by rule, NK_TUNE_CONV_S2DX 3 forces"
                          if a[0] == "4" else "narrow blocks: Cin % 64 == 0, Cout % 16 == 0, NK_TUNE_CONV_S2DX 2 forces") + f"; padding {a[2]} folded in; by rule from one block per CU")
    if fn == "s2f_weights_kernel":
        return _CONV_FWD.split(" (")[0] + " (folded padding 1 too)", f"in front of every s2f_kernel launch ({s2})"
    assert fn == "s2f_kernel", fn
    return _CONV_FWD.split(" (")[0] + " (folded padding 1 too)", (f"s2f_launch ({s2}): " + ("wide blocks: Cout % 128 == 0, Cin % 32 == 0; by rule with >= 8 blocks per CU" if a[0] == "4"
                                                                    else "narrow blocks: Cout % 64 == 0, Cin % 16 == 0; only under NK_TUNE_CONV_S2DX 1 / 2") )


def _describe(kernel):
    fn, a = _split(kernel)
    if fn.startswith(("sgemm", "splitk")):
        return _gemm(fn, a)
    return _attention(fn, a) if fn == "attention_kernel" else _conv(fn, a)


_SIZE = ("needs a gy of 2 GiB or more (N * Cout * L * 4 >= 2^31); no tensor of this suite is above 256 MiB, and the branches at 2^31 "
         "are a run-time matter the instantiation inventory leaves to a pull request of its own")
_UNREACHABLE = {
    "conv_direct_bwd_input_rows_kernel<1, 3, false>": _SIZE,
    "conv_direct_bwd_input_rows_kernel<3, 3, false>": _SIZE,
    "conv_direct_bwd_input_rows_kernel<5, 5, false>": _SIZE,
}

# kernel -> what enters it, measured (see the module docstring); kernels of the template grids the new file walks carry its ids
_REACHED = {
    # ---- nk_gemm.hip -----------------------------------------------------------------------------------------
    'sgemm_kernel<false, false, false, 1, 1, 1, false>': ("tests", ('test_sgemm_forced_tiles[nn-ragged-1x1]', 'test_sgemm_forced_tiles[nn-ragged_ld-1x1]', 'test_sgemm_forced_tiles[nn-offset-1x1]')),
    'sgemm_kernel<false, false, false, 1, 1, 1, true>': ("tests", ('test_sgemm_epilogues_equal_the_separate_nodes[mask-ragged-1x1-kg1]', 'test_sgemm_epilogues_equal_the_separate_nodes[mask-k_plus1-1x1-kg1]')),
    'sgemm_kernel<false, false, false, 1, 2, 1, false>': ("tests", ('test_sgemm_forced_tiles[nn-ragged-1x2]', 'test_sgemm_forced_tiles[nn-ragged_ld-1x2]', 'test_sgemm_forced_tiles[nn-offset-1x2]')),
    'sgemm_kernel<false, false, false, 1, 2, 1, true>': ("tests", ('test_sgemm_epilogues_equal_the_separate_nodes[mask-ragged-1x2-kg1]', 'test_sgemm_epilogues_equal_the_separate_nodes[mask-k_plus1-1x2-kg1]')),
    'sgemm_kernel<false, false, false, 2, 1, 1, false>': ("tests", ('test_sgemm_forced_tiles[nn-ragged-2x1]', 'test_sgemm_forced_tiles[nn-ragged_ld-2x1]', 'test_sgemm_forced_tiles[nn-offset-2x1]')),
    'sgemm_kernel<false, false, false, 2, 1, 1, true>': ("tests", ('test_sgemm_epilogues_equal_the_separate_nodes[mask-ragged-2x1-kg1]', 'test_sgemm_epilogues_equal_the_separate_nodes[mask-k_plus1-2x1-kg1]')),
    'sgemm_kernel<false, false, false, 2, 2, 1, false>': ("tests", ('test_sgemm_forced_tiles[nn-ragged-2x2]', 'test_sgemm_forced_tiles[nn-ragged_ld-2x2]', 'test_sgemm_forced_tiles[nn-offset-2x2]')),
    'sgemm_kernel<false, false, false, 2, 2, 1, true>': ("tests", ('test_sgemm_epilogues_equal_the_separate_nodes[mask-ragged-2x2-kg1]', 'test_sgemm_epilogues_equal_the_separate_nodes[mask-k_plus1-2x2-kg1]')),
    'sgemm_kernel<false, false, true, 1, 1, 1, false>': ("tests", ('test_sgemm_forced_tiles[nn-aligned-1x1]', 'test_sgemm_epilogues_equal_the_separate_nodes[mask-aligned-1x1-kg1]', 'test_sgemm_pair_kernel[nn-1x1]')),
    'sgemm_kernel<false, false, true, 1, 1, 1, true>': ("tests", ('test_sgemm_epilogues_equal_the_separate_nodes[mask-aligned-1x1-kg1]',)),
    'sgemm_kernel<false, false, true, 1, 1, 2, false>': ("tests", ('test_sgemm_epilogues_equal_the_separate_nodes[mask-aligned-1x1-kg2]',)),
    'sgemm_kernel<false, false, true, 1, 1, 2, true>': ("tests", ('test_sgemm_epilogues_equal_the_separate_nodes[mask-aligned-1x1-kg2]',)),
    'sgemm_kernel<false, false, true, 1, 2, 1, false>': ("tests", ('test_sgemm_forced_tiles[nn-aligned-1x2]', 'test_sgemm_epilogues_equal_the_separate_nodes[mask-aligned-1x2-kg1]')),
    'sgemm_kernel<false, false, true, 1, 2, 1, true>': ("tests", ('test_sgemm_epilogues_equal_the_separate_nodes[mask-aligned-1x2-kg1]',)),
    'sgemm_kernel<false, false, true, 2, 1, 1, false>': ("tests", ('test_sgemm_forced_tiles[nn-aligned-2x1]', 'test_sgemm_epilogues_equal_the_separate_nodes[mask-aligned-2x1-kg1]', 'test_sgemm_pair_kernel[nn-2x1]')),
    'sgemm_kernel<false, false, true, 2, 1, 1, true>': ("tests", ('test_sgemm_epilogues_equal_the_separate_nodes[mask-aligned-2x1-kg1]',)),
    'sgemm_kernel<false, false, true, 2, 2, 1, false>': ("tests", ('test_sgemm_forced_tiles[nn-aligned-2x2]', 'test_sgemm_epilogues_equal_the_separate_nodes[mask-aligned-2x2-kg1]', 'test_sgemm_pair_kernel[nn-2x2]')),
    'sgemm_kernel<false, false, true, 2, 2, 1, true>': ("tests", ('test_sgemm_epilogues_equal_the_separate_nodes[mask-aligned-2x2-kg1]',)),
    'sgemm_kernel<false, false, true, 2, 2, 2, false>': ("tests", ('test_sgemm_epilogues_equal_the_separate_nodes[mask-aligned-2x2-kg2]',)),
    'sgemm_kernel<false, false, true, 2, 2, 2, true>': ("tests", ('test_sgemm_epilogues_equal_the_separate_nodes[mask-aligned-2x2-kg2]',)),
    'sgemm_kernel<false, true, false, 1, 1, 1, true>': ("tests", ('test_sgemm_forced_tiles[nt-ragged-1x1]', 'test_sgemm_forced_tiles[nt-ragged_ld-1x1]', 'test_sgemm_forced_tiles[nt-offset-1x1]')),
    'sgemm_kernel<false, true, false, 1, 2, 1, true>': ("tests", ('test_sgemm_forced_tiles[nt-ragged-1x2]', 'test_sgemm_forced_tiles[nt-ragged_ld-1x2]', 'test_sgemm_forced_tiles[nt-offset-1x2]')),
    'sgemm_kernel<false, true, false, 2, 1, 1, true>': ("tests", ('test_sgemm_forced_tiles[nt-ragged-2x1]', 'test_sgemm_forced_tiles[nt-ragged_ld-2x1]', 'test_sgemm_forced_tiles[nt-offset-2x1]')),
    'sgemm_kernel<false, true, false, 2, 2, 1, true>': ("tests", ('test_sgemm_forced_tiles[nt-ragged-2x2]', 'test_sgemm_forced_tiles[nt-ragged_ld-2x2]', 'test_sgemm_forced_tiles[nt-offset-2x2]')),
    'sgemm_kernel<false, true, true, 1, 1, 1, true>': ("tests", ('test_sgemm_forced_tiles[nt-aligned-1x1]', 'test_sgemm_epilogues_equal_the_separate_nodes[bias-aligned-1x1-kg1]', 'test_sgemm_epilogues_equal_the_separate_nodes[bias_relu-aligned-1x1-kg1]')),
    'sgemm_kernel<false, true, true, 1, 1, 2, true>': ("tests", ('test_sgemm_epilogues_equal_the_separate_nodes[bias-aligned-1x1-kg2]', 'test_sgemm_epilogues_equal_the_separate_nodes[bias_relu-aligned-1x1-kg2]')),
    'sgemm_kernel<false, true, true, 1, 2, 1, true>': ("tests", ('test_sgemm_forced_tiles[nt-aligned-1x2]', 'test_sgemm_epilogues_equal_the_separate_nodes[bias-aligned-1x2-kg1]', 'test_sgemm_epilogues_equal_the_separate_nodes[bias_relu-aligned-1x2-kg1]')),
    'sgemm_kernel<false, true, true, 2, 1, 1, true>': ("tests", ('test_sgemm_forced_tiles[nt-aligned-2x1]', 'test_sgemm_epilogues_equal_the_separate_nodes[bias-aligned-2x1-kg1]', 'test_sgemm_epilogues_equal_the_separate_nodes[bias_relu-aligned-2x1-kg1]')),
    'sgemm_kernel<false, true, true, 2, 2, 1, true>': ("tests", ('test_sgemm_forced_tiles[nt-aligned-2x2]', 'test_sgemm_epilogues_equal_the_separate_nodes[bias-aligned-2x2-kg1]', 'test_sgemm_epilogues_equal_the_separate_nodes[bias_relu-aligned-2x2-kg1]')),
    'sgemm_kernel<false, true, true, 2, 2, 2, true>': ("tests", ('test_sgemm_epilogues_equal_the_separate_nodes[bias-aligned-2x2-kg2]', 'test_sgemm_epilogues_equal_the_separate_nodes[bias_relu-aligned-2x2-kg2]')),
    'sgemm_kernel<true, false, false, 1, 1, 1, false>': ("tests", ('test_sgemm_forced_tiles[tn-ragged-1x1]', 'test_sgemm_forced_tiles[tn-ragged_ld-1x1]', 'test_sgemm_forced_tiles[tn-offset-1x1]')),
    'sgemm_kernel<true, false, false, 1, 2, 1, false>': ("tests", ('test_sgemm_forced_tiles[tn-ragged-1x2]', 'test_sgemm_forced_tiles[tn-ragged_ld-1x2]', 'test_sgemm_forced_tiles[tn-offset-1x2]')),
    'sgemm_kernel<true, false, false, 2, 1, 1, false>': ("tests", ('test_sgemm_forced_tiles[tn-ragged-2x1]', 'test_sgemm_forced_tiles[tn-ragged_ld-2x1]', 'test_sgemm_forced_tiles[tn-offset-2x1]')),
    'sgemm_kernel<true, false, false, 2, 2, 1, false>': ("tests", ('test_sgemm_forced_tiles[tn-ragged-2x2]', 'test_sgemm_forced_tiles[tn-ragged_ld-2x2]', 'test_sgemm_forced_tiles[tn-offset-2x2]')),
    'sgemm_kernel<true, false, true, 1, 1, 1, false>': ("tests", ('test_sgemm_forced_tiles[tn-aligned-1x1]', 'test_sgemm_pair_kernel[nn-1x1]', 'test_sgemm_pair_kernel[nt-1x1]')),
    'sgemm_kernel<true, false, true, 1, 1, 2, false>': ("covered_by", 'tests/test_gpu_parity.py::test_sgemm_lookahead_loop_is_bit_identical[1,1-1-0]'),
    'sgemm_kernel<true, false, true, 1, 2, 1, false>': ("tests", ('test_sgemm_forced_tiles[tn-aligned-1x2]',)),
    'sgemm_kernel<true, false, true, 2, 1, 1, false>': ("tests", ('test_sgemm_forced_tiles[tn-aligned-2x1]', 'test_sgemm_pair_kernel[nn-2x1]', 'test_sgemm_pair_kernel[nt-2x1]')),
    'sgemm_kernel<true, false, true, 2, 2, 1, false>': ("tests", ('test_sgemm_forced_tiles[tn-aligned-2x2]', 'test_sgemm_pair_kernel[nn-2x2]', 'test_sgemm_pair_kernel[nt-2x2]')),
    'sgemm_kernel<true, false, true, 2, 2, 2, false>': ("covered_by", 'tests/test_gpu_parity.py::test_sgemm_lookahead_loop_is_bit_identical[2,2-1-0]'),
    'sgemm_kernel<true, true, false, 1, 1, 1, false>': ("tests", ('test_sgemm_forced_tiles[tt-ragged-1x1]', 'test_sgemm_forced_tiles[tt-ragged_ld-1x1]', 'test_sgemm_forced_tiles[tt-offset-1x1]')),
    'sgemm_kernel<true, true, false, 1, 2, 1, false>': ("tests", ('test_sgemm_forced_tiles[tt-ragged-1x2]', 'test_sgemm_forced_tiles[tt-ragged_ld-1x2]', 'test_sgemm_forced_tiles[tt-offset-1x2]')),
    'sgemm_kernel<true, true, false, 2, 1, 1, false>': ("tests", ('test_sgemm_forced_tiles[tt-ragged-2x1]', 'test_sgemm_forced_tiles[tt-ragged_ld-2x1]', 'test_sgemm_forced_tiles[tt-offset-2x1]')),
    'sgemm_kernel<true, true, false, 2, 2, 1, false>': ("tests", ('test_sgemm_forced_tiles[tt-ragged-2x2]', 'test_sgemm_forced_tiles[tt-ragged_ld-2x2]', 'test_sgemm_forced_tiles[tt-offset-2x2]')),
    'sgemm_kernel<true, true, true, 1, 1, 1, false>': ("tests", ('test_sgemm_forced_tiles[tt-aligned-1x1]',)),
    'sgemm_kernel<true, true, true, 1, 1, 2, false>': ("covered_by", 'tests/test_gpu_parity.py::test_sgemm_lookahead_loop_is_bit_identical[1,1-1-1]'),
    'sgemm_kernel<true, true, true, 1, 2, 1, false>': ("tests", ('test_sgemm_forced_tiles[tt-aligned-1x2]',)),
    'sgemm_kernel<true, true, true, 2, 1, 1, false>': ("tests", ('test_sgemm_forced_tiles[tt-aligned-2x1]',)),
    'sgemm_kernel<true, true, true, 2, 2, 1, false>': ("tests", ('test_sgemm_forced_tiles[tt-aligned-2x2]',)),
    'sgemm_kernel<true, true, true, 2, 2, 2, false>': ("covered_by", 'tests/test_gpu_parity.py::test_sgemm_lookahead_loop_is_bit_identical[2,2-1-1]'),
    'sgemm_pair_kernel<false, false, true, false, 1, 1>': ("tests", ('test_sgemm_pair_kernel[nn-1x1]',)),
    'sgemm_pair_kernel<false, false, true, false, 2, 1>': ("tests", ('test_sgemm_pair_kernel[nn-2x1]',)),
    'sgemm_pair_kernel<false, false, true, false, 2, 2>': ("tests", ('test_sgemm_pair_kernel[nn-2x2]',)),
    'sgemm_pair_kernel<false, true, true, false, 1, 1>': ("tests", ('test_sgemm_pair_kernel[nt-1x1]',)),
    'sgemm_pair_kernel<false, true, true, false, 2, 1>': ("tests", ('test_sgemm_pair_kernel[nt-2x1]',)),
    'sgemm_pair_kernel<false, true, true, false, 2, 2>': ("tests", ('test_sgemm_pair_kernel[nt-2x2]',)),
    'sgemm_pair_kernel<true, false, true, false, 1, 1>': ("tests", ('test_sgemm_pair_kernel[tn-1x1]', 'test_attention_backward_forms[dh64-S128-p0.0-full]', 'test_attention_backward_forms[dh64-S128-p0.0-causal]')),
    'sgemm_pair_kernel<true, false, true, false, 2, 1>': ("tests", ('test_sgemm_pair_kernel[tn-2x1]',)),
    'sgemm_pair_kernel<true, false, true, false, 2, 2>': ("tests", ('test_sgemm_pair_kernel[tn-2x2]',)),
    'sgemm_tail_kernel<false, false, false>': ("tests", ('test_sgemm_tail_kernel[nn]',)),
    'sgemm_tail_kernel<false, false, true>': ("covered_by", 'tests/test_gpu_parity.py::test_gemm_shared_chip_schedule[4096-4096-256-16-NN]'),
    'sgemm_tail_kernel<false, true, true>': ("tests", ('test_sgemm_tail_kernel[nt]',)),
    'sgemm_tail_kernel<true, false, false>': ("tests", ('test_sgemm_tail_kernel[tn]',)),
    'splitk_reduce_flat_kernel': ("covered_by", 'tests/test_gpu_parity.py::test_sgemm_random[0-0-64-200-1000]'),
    'splitk_reduce_kernel': ("tests", ('test_sgemm_tail_kernel[nn]', 'test_sgemm_tail_kernel[nt]', 'test_sgemm_tail_kernel[tn]')),
    # ---- nk_conv.hip -----------------------------------------------------------------------------------------
    'conv_bwd_input_fast_kernel<false, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs7-ws7-s7-d7-2]'),
    'conv_bwd_input_fast_kernel<false, 2>': ("tests", ('test_conv_input_gradient_fast_ragged_128',)),
    'conv_bwd_input_fast_kernel<true, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs5-ws5-s5-d5-1]'),
    'conv_bwd_input_fast_kernel<true, 2>': ("tests", ('test_conv_s2dx_wide_blocks[1]',)),
    'conv_bwd_input_kernel<false, false, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs28-ws28-s28-d28-1]'),
    'conv_bwd_input_kernel<false, false, 2>': ("covered_by", 'tests/test_gpu_conv_s2dx.py::test_s2dx_fuzz_equals_the_per_phase_kernels_on_integer_data[4-128-48-10-20-0]'),
    'conv_bwd_input_kernel<false, true, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs18-ws18-s18-d18-1]'),
    'conv_bwd_input_kernel<false, true, 2>': ("tests", ('test_conv_input_gradient_fast_ragged_128',)),
    'conv_bwd_input_kernel<true, false, 1>': ("covered_by", 'tests/test_gpu_conv_fuzz.py::test_conv_random_geometry[73]'),
    'conv_bwd_input_kernel<true, false, 2>': ("tests", ('test_conv_s2dx_wide_blocks[0]',)),
    'conv_bwd_input_kernel<true, true, 1>': ("covered_by", 'tests/test_gpu_conv_fuzz.py::test_conv_random_geometry[158]'),
    'conv_bwd_input_kernel<true, true, 2>': ("covered_by", 'tests/test_gpu_winograd.py::test_winograd_fuzz_all_three_passes_equal_the_direct_kernels_on_integer_data[2-128-256-2-2-pad34]'),
    'conv_bwd_input_tail_reduce_kernel<128>': ("covered_by", 'tests/test_gpu_winograd.py::test_winograd_equals_direct_exactly_on_integer_data[1-128-128-12-12]'),
    'conv_bwd_input_tail_reduce_kernel<64>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs5-ws5-s5-d5-1]'),
    'conv_bwd_kernel_kernel<false, 1, 1, false, 1>': ("covered_by", 'tests/test_gpu_conv_fuzz.py::test_conv_random_geometry[6]'),
    'conv_bwd_kernel_kernel<false, 1, 2, false, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs18-ws18-s18-d18-1]'),
    'conv_bwd_kernel_kernel<false, 2, 1, false, 1>': ("tests", ('test_conv_kernel_gradient_paths[scalar_s3_L9]',)),
    'conv_bwd_kernel_kernel<false, 2, 2, false, 1>': ("covered_by", 'tests/test_gpu_winograd.py::test_winograd_fuzz_all_three_passes_equal_the_direct_kernels_on_integer_data[5-192-256-19-3-pad56]'),
    'conv_bwd_kernel_kernel<true, 1, 1, false, 1>': ("covered_by", 'tests/test_gpu_conv_fuzz.py::test_conv_random_geometry[12]'),
    'conv_bwd_kernel_kernel<true, 1, 1, true, 1>': ("covered_by", 'tests/test_gpu_conv_fuzz.py::test_conv_random_geometry[22]'),
    'conv_bwd_kernel_kernel<true, 1, 1, true, 2>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs24-ws24-s24-d24-1]'),
    'conv_bwd_kernel_kernel<true, 1, 2, false, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs25-ws25-s25-d25-1]'),
    'conv_bwd_kernel_kernel<true, 1, 2, true, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs7-ws7-s7-d7-2]'),
    'conv_bwd_kernel_kernel<true, 1, 2, true, 2>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs19-ws19-s19-d19-1]'),
    'conv_bwd_kernel_kernel<true, 2, 1, false, 1>': ("tests", ('test_conv_kernel_gradient_paths[vec_s3_L12]',)),
    'conv_bwd_kernel_kernel<true, 2, 1, true, 1>': ("tests", ('test_conv_kernel_gradient_paths[quad_s1]',)),
    'conv_bwd_kernel_kernel<true, 2, 1, true, 2>': ("tests", ('test_conv_kernel_gradient_paths[quad_s2]',)),
    'conv_bwd_kernel_kernel<true, 2, 2, false, 1>': ("covered_by", 'tests/test_gpu_winograd.py::test_winograd_fuzz_all_three_passes_equal_the_direct_kernels_on_integer_data[5-192-256-20-2-pad16]'),
    'conv_bwd_kernel_kernel<true, 2, 2, true, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs4-ws4-s4-d4-1]'),
    'conv_bwd_kernel_kernel<true, 2, 2, true, 2>': ("covered_by", 'tests/test_gpu_winograd.py::test_padding_folds_query_and_fallbacks'),
    'conv_bwd_kernel_mixed_kernel<true, 1, true, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs11-ws11-s11-d11-1]'),
    'conv_bwd_kernel_mixed_kernel<true, 2, true, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs5-ws5-s5-d5-1]'),
    'conv_direct_bwd_input_kernel<false, 1, 0, 0>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_golden_exact[conv1d_dilated]'),
    'conv_direct_bwd_input_kernel<false, 1, 3, 3>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs37-ws37-s37-d37-8]'),
    'conv_direct_bwd_input_kernel<false, 4, 0, 0>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_bwd_input_padded_vs_oracle[xs9-ws9-pad9-s9-d9-2]'),
    'conv_direct_bwd_input_kernel<false, 4, 3, 3>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs46-ws46-s46-d46-8]'),
    'conv_direct_bwd_input_kernel<true, 1, 0, 0>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_golden_exact[conv1d]'),
    'conv_direct_bwd_input_kernel<true, 1, 3, 3>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs0-ws0-s0-d0-1]'),
    'conv_direct_bwd_input_kernel<true, 4, 0, 0>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs43-ws43-s43-d43-3]'),
    'conv_direct_bwd_input_kernel<true, 4, 3, 3>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs41-ws41-s41-d41-8]'),
    'conv_direct_bwd_input_rows_kernel<1, 3, true>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_bwd_input_padded_vs_oracle[xs26-ws26-pad26-s26-d26-8]'),
    'conv_direct_bwd_input_rows_kernel<3, 3, true>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs40-ws40-s40-d40-1]'),
    'conv_direct_bwd_input_rows_kernel<5, 5, true>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs47-ws47-s47-d47-3]'),
    'conv_direct_bwd_input_strided_kernel<1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_golden_exact[conv1d_strided]'),
    'conv_direct_bwd_input_strided_kernel<4>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs42-ws42-s42-d42-8]'),
    'conv_direct_bwd_kernel_kernel': ("covered_by", 'tests/test_gpu_parity.py::test_conv_golden_exact[conv1d]'),
    'conv_direct_bwd_kernel_taps_kernel<3, 3>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs0-ws0-s0-d0-1]'),
    'conv_direct_bwd_kernel_taps_kernel<5, 5>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs43-ws43-s43-d43-3]'),
    'conv_direct_fwd_kernel<1, 0, 0>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_golden_exact[conv1d]'),
    'conv_direct_fwd_kernel<1, 3, 3>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs37-ws37-s37-d37-8]'),
    'conv_direct_fwd_kernel<1, 5, 5>': ("tests", ('test_conv_forward_paths[direct_5x5_w5]', 'test_conv_forward_paths[direct_5x5_dil2]')),
    'conv_direct_fwd_kernel<4, 0, 0>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs44-ws44-s44-d44-3]'),
    'conv_direct_fwd_kernel<4, 3, 3>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs41-ws41-s41-d41-8]'),
    'conv_direct_fwd_kernel<4, 5, 5>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs43-ws43-s43-d43-3]'),
    'conv_direct_fwd_rows_kernel<1, 3>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs48-ws48-s48-d48-8]'),
    'conv_direct_fwd_rows_kernel<3, 3>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs0-ws0-s0-d0-1]'),
    'conv_direct_fwd_rows_kernel<5, 5>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs47-ws47-s47-d47-3]'),
    'conv_dw_reduce_kernel': ("tests", ('test_conv_kernel_gradient_paths[quad_s1]', 'test_conv_kernel_gradient_paths[quad_s2]', 'test_conv_kernel_gradient_paths[vec_s3_L12]')),
    'conv_fwd_fast_kernel<false, 1, false, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs7-ws7-s7-d7-2]'),
    'conv_fwd_fast_kernel<false, 1, false, 2>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs23-ws23-s23-d23-1]'),
    'conv_fwd_fast_kernel<false, 1, true, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs13-ws13-s13-d13-1]'),
    'conv_fwd_fast_kernel<false, 1, true, 2>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs19-ws19-s19-d19-1]'),
    'conv_fwd_fast_kernel<false, 2, false, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs8-ws8-s8-d8-1]'),
    'conv_fwd_fast_kernel<false, 2, false, 2>': ("tests", ('test_conv_forward_paths[fast_m96_s2_w4]',)),
    'conv_fwd_fast_kernel<false, 2, true, 1>': ("tests", ('test_conv_forward_paths[fast_m96_s1_w5]',)),
    'conv_fwd_fast_kernel<false, 2, true, 2>': ("tests", ('test_conv_forward_paths[fast_m96_s2_w5]',)),
    'conv_fwd_fast_kernel<true, 1, false, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs9-ws9-s9-d9-1]'),
    'conv_fwd_fast_kernel<true, 1, false, 2>': ("tests", ('test_conv_forward_paths[fast_m64_s2_w4]', 'test_conv_forward_paths[fast_m64_s2_w4_g2]')),
    'conv_fwd_fast_kernel<true, 1, true, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs14-ws14-s14-d14-1]'),
    'conv_fwd_fast_kernel<true, 1, true, 2>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs24-ws24-s24-d24-1]'),
    'conv_fwd_fast_kernel<true, 2, false, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs6-ws6-s6-d6-1]'),
    'conv_fwd_fast_kernel<true, 2, false, 2>': ("covered_by", 'tests/test_gpu_winograd.py::test_padding_folds_query_and_fallbacks'),
    'conv_fwd_fast_kernel<true, 2, true, 1>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs5-ws5-s5-d5-1]'),
    'conv_fwd_fast_kernel<true, 2, true, 2>': ("covered_by", 'tests/test_gpu_winograd.py::test_winograd_rule_and_knob'),
    'conv_fwd_kernel<false, 1, false>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs18-ws18-s18-d18-1]'),
    'conv_fwd_kernel<false, 1, true>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs30-ws30-s30-d30-1]'),
    'conv_fwd_kernel<false, 2, false>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs4-ws4-s4-d4-1]'),
    'conv_fwd_kernel<false, 2, true>': ("covered_by", 'tests/test_gpu_winograd.py::test_winograd_rule_and_knob'),
    'conv_fwd_kernel<true, 1, false>': ("covered_by", 'tests/test_gpu_conv_fuzz.py::test_conv_random_geometry[73]'),
    'conv_fwd_kernel<true, 1, true>': ("tests", ('test_conv_forward_paths[generic_m64_k32_w4]',)),
    'conv_fwd_kernel<true, 2, false>': ("covered_by", 'tests/test_gpu_winograd.py::test_winograd_fuzz_all_three_passes_equal_the_direct_kernels_on_integer_data[5-192-256-20-2-pad16]'),
    'conv_fwd_kernel<true, 2, true>': ("tests", ('test_conv_forward_paths[generic_m128_k32_w4]', 'test_conv_forward_paths[generic_m128_k32_w4_3d]')),
    'conv_fwd_tail_reduce_kernel<128>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs5-ws5-s5-d5-1]'),
    'conv_fwd_tail_reduce_kernel<64>': ("covered_by", 'tests/test_gpu_parity.py::test_conv_random_vs_oracle[xs11-ws11-s11-d11-1]'),
    'conv_koff_kernel': ("tests", ('test_conv_forward_paths[generic_m64_k32_w4]', 'test_conv_forward_paths[generic_m128_k32_w4]', 'test_conv_forward_paths[generic_m128_k32_w4_3d]')),
    'conv_ktab_kernel': ("tests", ('test_conv_input_gradient_fast_ragged_128', 'test_conv_s2dx_wide_blocks[0]')),
    'conv_wp_kernel': ("tests", ('test_conv_forward_paths[fast_m96_s2_w4]', 'test_conv_forward_paths[fast_m96_s1_w5]', 'test_conv_forward_paths[fast_m96_s2_w5]')),
    'conv_wq_tables_kernel': ("tests", ('test_conv_input_gradient_fast_ragged_128', 'test_conv_s2dx_wide_blocks[1]')),
    'conv_wt_kernel': ("tests", ('test_conv_input_gradient_fast_ragged_128', 'test_conv_s2dx_wide_blocks[0]')),
    's2dx_kernel<2, 16, 0>': ("tests", ('test_conv_s2dx_wide_blocks[0]',)),
    's2dx_kernel<2, 16, 1>': ("tests", ('test_conv_s2dx_wide_blocks[1]',)),
    's2dx_kernel<4, 32, 0>': ("tests", ('test_conv_s2dx_wide_blocks[0]',)),
    's2dx_kernel<4, 32, 1>': ("tests", ('test_conv_s2dx_wide_blocks[1]',)),
    's2dx_weights_kernel': ("tests", ('test_conv_s2dx_wide_blocks[0]', 'test_conv_s2dx_wide_blocks[1]')),
    's2f_kernel<2, 16>': ("covered_by", 'tests/test_gpu_conv_s2dx.py::test_s2_forward_tap_planes_equal_the_implicit_gemm_exactly_on_integer_data[2-64-128-8-8-1]'),
    's2f_kernel<4, 32>': ("covered_by", 'tests/test_gpu_conv_s2dx.py::test_s2_forward_tap_planes_equal_the_implicit_gemm_exactly_on_integer_data[2-64-128-8-8-1]'),
    's2f_weights_kernel': ("covered_by", 'tests/test_gpu_conv_s2dx.py::test_s2_forward_tap_planes_equal_the_implicit_gemm_exactly_on_integer_data[2-64-128-8-8-1]'),
    'wino_dw_kernel<false, false>': ("covered_by", 'tests/test_gpu_winograd.py::test_winograd_kernel_gradient_equals_direct_exactly_on_integer_data[2-64-64-10-10]'),
    'wino_dw_kernel<false, true>': ("covered_by", 'tests/test_gpu_winograd.py::test_winograd_kernel_gradient_equals_direct_exactly_on_integer_data[2-64-64-9-9]'),
    'wino_dw_kernel<true, false>': ("covered_by", 'tests/test_gpu_winograd.py::test_folded_padding_equals_the_padded_copy_bit_for_bit[2-64-64-8-8-pad0]'),
    'wino_dw_kernel<true, true>': ("covered_by", 'tests/test_gpu_winograd.py::test_folded_padding_equals_the_padded_copy_bit_for_bit[2-64-64-7-7-pad7]'),
    'wino_dw_reduce_kernel': ("covered_by", 'tests/test_gpu_winograd.py::test_winograd_kernel_gradient_equals_direct_exactly_on_integer_data[2-64-64-10-10]'),
    'wino_kernel<2, 1, 16, 4, false>': ("covered_by", 'tests/test_gpu_winograd.py::test_winograd_equals_direct_exactly_on_integer_data[2-64-128-10-10]'),
    'wino_kernel<2, 1, 16, 4, true>': ("covered_by", 'tests/test_gpu_winograd.py::test_winograd_equals_direct_exactly_on_integer_data[2-64-128-9-9]'),
    'wino_kernel<4, 1, 32, 2, false>': ("covered_by", 'tests/test_gpu_winograd.py::test_winograd_equals_direct_exactly_on_integer_data[2-64-128-10-10]'),
    'wino_kernel<4, 1, 32, 2, true>': ("covered_by", 'tests/test_gpu_winograd.py::test_winograd_equals_direct_exactly_on_integer_data[2-64-128-9-9]'),
    'wino_weights_kernel': ("covered_by", 'tests/test_gpu_winograd.py::test_winograd_equals_direct_exactly_on_integer_data[2-64-128-10-10]'),
    # ---- nk_attention.hip ------------------------------------------------------------------------------------
    'attention_kernel<false, false, false, 1, false, 128, false, false>': ("tests", ('test_attention_forward_forms[dh128-S32-p0.0-full]', 'test_attention_forward_forms[dh128-S96-p0.0-full]')),
    'attention_kernel<false, false, false, 1, false, 128, false, true>': ("tests", ('test_attention_forward_forms[dh128-S32-p0.0-causal]', 'test_attention_forward_forms[dh128-S96-p0.0-causal]')),
    'attention_kernel<false, false, false, 1, false, 128, true, false>': ("tests", ('test_attention_forward_forms[dh128-S1-p0.0-full]', 'test_attention_forward_forms[dh128-S31-p0.0-full]', 'test_attention_forward_forms[dh128-S33-p0.0-full]')),
    'attention_kernel<false, false, false, 1, false, 128, true, true>': ("tests", ('test_attention_forward_forms[dh128-S1-p0.0-causal]', 'test_attention_forward_forms[dh128-S31-p0.0-causal]', 'test_attention_forward_forms[dh128-S33-p0.0-causal]')),
    'attention_kernel<false, false, false, 1, true, 128, false, false>': ("tests", ('test_attention_forward_forms[dh128-S32-p0.0-full]', 'test_attention_forward_forms[dh128-S96-p0.0-full]', 'test_attention_backward_forms[dh128-S96-p0.0-full]')),
    'attention_kernel<false, false, false, 1, true, 128, false, true>': ("tests", ('test_attention_forward_forms[dh128-S32-p0.0-causal]', 'test_attention_forward_forms[dh128-S96-p0.0-causal]', 'test_attention_backward_forms[dh128-S96-p0.0-causal]')),
    'attention_kernel<false, false, false, 1, true, 128, true, false>': ("tests", ('test_attention_forward_forms[dh128-S1-p0.0-full]', 'test_attention_forward_forms[dh128-S31-p0.0-full]', 'test_attention_forward_forms[dh128-S33-p0.0-full]')),
    'attention_kernel<false, false, false, 1, true, 128, true, true>': ("tests", ('test_attention_forward_forms[dh128-S1-p0.0-causal]', 'test_attention_forward_forms[dh128-S31-p0.0-causal]', 'test_attention_forward_forms[dh128-S33-p0.0-causal]')),
    'attention_kernel<false, false, false, 2, true, 32, false, false>': ("tests", ('test_attention_forward_forms[dh32-S32-p0.0-full]', 'test_attention_forward_forms[dh32-S96-p0.0-full]')),
    'attention_kernel<false, false, false, 2, true, 32, true, false>': ("tests", ('test_attention_forward_forms[dh32-S1-p0.0-full]', 'test_attention_forward_forms[dh32-S31-p0.0-full]', 'test_attention_forward_forms[dh32-S33-p0.0-full]')),
    'attention_kernel<false, false, false, 2, true, 64, false, false>': ("tests", ('test_attention_forward_forms[dh64-S32-p0.0-full]', 'test_attention_forward_forms[dh64-S96-p0.0-full]')),
    'attention_kernel<false, false, false, 2, true, 64, true, false>': ("tests", ('test_attention_forward_forms[dh64-S1-p0.0-full]', 'test_attention_forward_forms[dh64-S31-p0.0-full]', 'test_attention_forward_forms[dh64-S33-p0.0-full]')),
    'attention_kernel<false, false, false, 3, false, 32, false, false>': ("tests", ('test_attention_forward_forms[dh32-S32-p0.0-full]', 'test_attention_forward_forms[dh32-S96-p0.0-full]')),
    'attention_kernel<false, false, false, 3, false, 32, false, true>': ("tests", ('test_attention_forward_forms[dh32-S32-p0.0-causal]', 'test_attention_forward_forms[dh32-S96-p0.0-causal]')),
    'attention_kernel<false, false, false, 3, false, 32, true, false>': ("tests", ('test_attention_forward_forms[dh32-S1-p0.0-full]', 'test_attention_forward_forms[dh32-S31-p0.0-full]', 'test_attention_forward_forms[dh32-S33-p0.0-full]')),
    'attention_kernel<false, false, false, 3, false, 32, true, true>': ("tests", ('test_attention_forward_forms[dh32-S1-p0.0-causal]', 'test_attention_forward_forms[dh32-S31-p0.0-causal]', 'test_attention_forward_forms[dh32-S33-p0.0-causal]')),
    'attention_kernel<false, false, false, 3, false, 64, false, false>': ("tests", ('test_attention_forward_forms[dh64-S32-p0.0-full]', 'test_attention_forward_forms[dh64-S96-p0.0-full]')),
    'attention_kernel<false, false, false, 3, false, 64, false, true>': ("tests", ('test_attention_forward_forms[dh64-S32-p0.0-causal]', 'test_attention_forward_forms[dh64-S96-p0.0-causal]')),
    'attention_kernel<false, false, false, 3, false, 64, true, false>': ("tests", ('test_attention_forward_forms[dh64-S1-p0.0-full]', 'test_attention_forward_forms[dh64-S31-p0.0-full]', 'test_attention_forward_forms[dh64-S33-p0.0-full]')),
    'attention_kernel<false, false, false, 3, false, 64, true, true>': ("tests", ('test_attention_forward_forms[dh64-S1-p0.0-causal]', 'test_attention_forward_forms[dh64-S31-p0.0-causal]', 'test_attention_forward_forms[dh64-S33-p0.0-causal]')),
    'attention_kernel<false, false, false, 3, true, 32, false, false>': ("tests", ('test_attention_forward_forms[dh32-S32-p0.0-full]', 'test_attention_forward_forms[dh32-S96-p0.0-full]', 'test_attention_backward_forms[dh32-S96-p0.0-full]')),
    'attention_kernel<false, false, false, 3, true, 32, false, true>': ("tests", ('test_attention_forward_forms[dh32-S32-p0.0-causal]', 'test_attention_forward_forms[dh32-S96-p0.0-causal]', 'test_attention_backward_forms[dh32-S96-p0.0-causal]')),
    'attention_kernel<false, false, false, 3, true, 32, true, false>': ("tests", ('test_attention_forward_forms[dh32-S1-p0.0-full]', 'test_attention_forward_forms[dh32-S31-p0.0-full]', 'test_attention_forward_forms[dh32-S33-p0.0-full]')),
    'attention_kernel<false, false, false, 3, true, 32, true, true>': ("tests", ('test_attention_forward_forms[dh32-S1-p0.0-causal]', 'test_attention_forward_forms[dh32-S31-p0.0-causal]', 'test_attention_forward_forms[dh32-S33-p0.0-causal]')),
    'attention_kernel<false, false, false, 3, true, 64, false, false>': ("tests", ('test_attention_forward_forms[dh64-S32-p0.0-full]', 'test_attention_forward_forms[dh64-S96-p0.0-full]', 'test_attention_backward_forms[dh64-S96-p0.0-full]')),
    'attention_kernel<false, false, false, 3, true, 64, false, true>': ("tests", ('test_attention_forward_forms[dh64-S32-p0.0-causal]', 'test_attention_forward_forms[dh64-S96-p0.0-causal]', 'test_attention_backward_forms[dh64-S96-p0.0-causal]')),
    'attention_kernel<false, false, false, 3, true, 64, true, false>': ("tests", ('test_attention_forward_forms[dh64-S1-p0.0-full]', 'test_attention_forward_forms[dh64-S31-p0.0-full]', 'test_attention_forward_forms[dh64-S33-p0.0-full]')),
    'attention_kernel<false, false, false, 3, true, 64, true, true>': ("tests", ('test_attention_forward_forms[dh64-S1-p0.0-causal]', 'test_attention_forward_forms[dh64-S31-p0.0-causal]', 'test_attention_forward_forms[dh64-S33-p0.0-causal]')),
    'attention_kernel<false, false, true, 1, false, 128, false, false>': ("tests", ('test_attention_forward_forms[dh128-S128-p0.0-full]', 'test_attention_forward_forms[dh128-S256-p0.0-full]')),
    'attention_kernel<false, false, true, 1, false, 128, false, true>': ("tests", ('test_attention_forward_forms[dh128-S128-p0.0-causal]', 'test_attention_forward_forms[dh128-S256-p0.0-causal]')),
    'attention_kernel<false, false, true, 1, true, 128, false, false>': ("tests", ('test_attention_forward_forms[dh128-S128-p0.0-full]', 'test_attention_forward_forms[dh128-S256-p0.0-full]', 'test_attention_backward_forms[dh128-S128-p0.0-full]')),
    'attention_kernel<false, false, true, 1, true, 128, false, true>': ("tests", ('test_attention_forward_forms[dh128-S128-p0.0-causal]', 'test_attention_forward_forms[dh128-S256-p0.0-causal]', 'test_attention_backward_forms[dh128-S128-p0.0-causal]')),
    'attention_kernel<false, false, true, 2, true, 32, false, false>': ("tests", ('test_attention_forward_forms[dh32-S128-p0.0-full]', 'test_attention_forward_forms[dh32-S256-p0.0-full]')),
    'attention_kernel<false, false, true, 2, true, 64, false, false>': ("tests", ('test_attention_forward_forms[dh64-S128-p0.0-full]', 'test_attention_forward_forms[dh64-S256-p0.0-full]')),
    'attention_kernel<false, false, true, 3, false, 32, false, false>': ("tests", ('test_attention_forward_forms[dh32-S128-p0.0-full]', 'test_attention_forward_forms[dh32-S256-p0.0-full]')),
    'attention_kernel<false, false, true, 3, false, 32, false, true>': ("tests", ('test_attention_forward_forms[dh32-S128-p0.0-causal]', 'test_attention_forward_forms[dh32-S256-p0.0-causal]')),
    'attention_kernel<false, false, true, 3, false, 64, false, false>': ("tests", ('test_attention_forward_forms[dh64-S128-p0.0-full]', 'test_attention_forward_forms[dh64-S256-p0.0-full]')),
    'attention_kernel<false, false, true, 3, false, 64, false, true>': ("tests", ('test_attention_forward_forms[dh64-S128-p0.0-causal]', 'test_attention_forward_forms[dh64-S256-p0.0-causal]')),
    'attention_kernel<false, false, true, 3, true, 32, false, false>': ("tests", ('test_attention_forward_forms[dh32-S128-p0.0-full]', 'test_attention_forward_forms[dh32-S256-p0.0-full]', 'test_attention_backward_forms[dh32-S128-p0.0-full]')),
    'attention_kernel<false, false, true, 3, true, 32, false, true>': ("tests", ('test_attention_forward_forms[dh32-S128-p0.0-causal]', 'test_attention_forward_forms[dh32-S256-p0.0-causal]', 'test_attention_backward_forms[dh32-S128-p0.0-causal]')),
    'attention_kernel<false, false, true, 3, true, 64, false, false>': ("tests", ('test_attention_forward_forms[dh64-S128-p0.0-full]', 'test_attention_forward_forms[dh64-S256-p0.0-full]', 'test_attention_backward_forms[dh64-S128-p0.0-full]')),
    'attention_kernel<false, false, true, 3, true, 64, false, true>': ("tests", ('test_attention_forward_forms[dh64-S128-p0.0-causal]', 'test_attention_forward_forms[dh64-S256-p0.0-causal]', 'test_attention_backward_forms[dh64-S128-p0.0-causal]')),
    'attention_kernel<false, true, false, 1, false, 128, false, false>': ("tests", ('test_attention_forward_forms[dh128-S32-p0.25-full]', 'test_attention_forward_forms[dh128-S96-p0.25-full]')),
    'attention_kernel<false, true, false, 1, false, 128, false, true>': ("tests", ('test_attention_forward_forms[dh128-S32-p0.25-causal]', 'test_attention_forward_forms[dh128-S96-p0.25-causal]')),
    'attention_kernel<false, true, false, 1, false, 128, true, false>': ("tests", ('test_attention_forward_forms[dh128-S1-p0.25-full]', 'test_attention_forward_forms[dh128-S31-p0.25-full]', 'test_attention_forward_forms[dh128-S33-p0.25-full]')),
    'attention_kernel<false, true, false, 1, false, 128, true, true>': ("tests", ('test_attention_forward_forms[dh128-S1-p0.25-causal]', 'test_attention_forward_forms[dh128-S31-p0.25-causal]', 'test_attention_forward_forms[dh128-S33-p0.25-causal]')),
    'attention_kernel<false, true, false, 1, true, 128, false, false>': ("tests", ('test_attention_forward_forms[dh128-S32-p0.25-full]', 'test_attention_forward_forms[dh128-S96-p0.25-full]', 'test_attention_backward_forms[dh128-S96-p0.25-full]')),
    'attention_kernel<false, true, false, 1, true, 128, false, true>': ("tests", ('test_attention_forward_forms[dh128-S32-p0.25-causal]', 'test_attention_forward_forms[dh128-S96-p0.25-causal]', 'test_attention_backward_forms[dh128-S96-p0.25-causal]')),
    'attention_kernel<false, true, false, 1, true, 128, true, false>': ("tests", ('test_attention_forward_forms[dh128-S1-p0.25-full]', 'test_attention_forward_forms[dh128-S31-p0.25-full]', 'test_attention_forward_forms[dh128-S33-p0.25-full]')),
    'attention_kernel<false, true, false, 1, true, 128, true, true>': ("tests", ('test_attention_forward_forms[dh128-S1-p0.25-causal]', 'test_attention_forward_forms[dh128-S31-p0.25-causal]', 'test_attention_forward_forms[dh128-S33-p0.25-causal]')),
    'attention_kernel<false, true, false, 2, true, 32, false, false>': ("tests", ('test_attention_forward_forms[dh32-S32-p0.25-full]', 'test_attention_forward_forms[dh32-S96-p0.25-full]')),
    'attention_kernel<false, true, false, 2, true, 32, true, false>': ("tests", ('test_attention_forward_forms[dh32-S1-p0.25-full]', 'test_attention_forward_forms[dh32-S31-p0.25-full]', 'test_attention_forward_forms[dh32-S33-p0.25-full]')),
    'attention_kernel<false, true, false, 2, true, 64, false, false>': ("tests", ('test_attention_forward_forms[dh64-S32-p0.25-full]', 'test_attention_forward_forms[dh64-S96-p0.25-full]')),
    'attention_kernel<false, true, false, 2, true, 64, true, false>': ("tests", ('test_attention_forward_forms[dh64-S1-p0.25-full]', 'test_attention_forward_forms[dh64-S31-p0.25-full]', 'test_attention_forward_forms[dh64-S33-p0.25-full]')),
    'attention_kernel<false, true, false, 3, false, 32, false, false>': ("tests", ('test_attention_forward_forms[dh32-S32-p0.25-full]', 'test_attention_forward_forms[dh32-S96-p0.25-full]')),
    'attention_kernel<false, true, false, 3, false, 32, false, true>': ("tests", ('test_attention_forward_forms[dh32-S32-p0.25-causal]', 'test_attention_forward_forms[dh32-S96-p0.25-causal]')),
    'attention_kernel<false, true, false, 3, false, 32, true, false>': ("tests", ('test_attention_forward_forms[dh32-S1-p0.25-full]', 'test_attention_forward_forms[dh32-S31-p0.25-full]', 'test_attention_forward_forms[dh32-S33-p0.25-full]')),
    'attention_kernel<false, true, false, 3, false, 32, true, true>': ("tests", ('test_attention_forward_forms[dh32-S1-p0.25-causal]', 'test_attention_forward_forms[dh32-S31-p0.25-causal]', 'test_attention_forward_forms[dh32-S33-p0.25-causal]')),
    'attention_kernel<false, true, false, 3, false, 64, false, false>': ("tests", ('test_attention_forward_forms[dh64-S32-p0.25-full]', 'test_attention_forward_forms[dh64-S96-p0.25-full]')),
    'attention_kernel<false, true, false, 3, false, 64, false, true>': ("tests", ('test_attention_forward_forms[dh64-S32-p0.25-causal]', 'test_attention_forward_forms[dh64-S96-p0.25-causal]')),
    'attention_kernel<false, true, false, 3, false, 64, true, false>': ("tests", ('test_attention_forward_forms[dh64-S1-p0.25-full]', 'test_attention_forward_forms[dh64-S31-p0.25-full]', 'test_attention_forward_forms[dh64-S33-p0.25-full]')),
    'attention_kernel<false, true, false, 3, false, 64, true, true>': ("tests", ('test_attention_forward_forms[dh64-S1-p0.25-causal]', 'test_attention_forward_forms[dh64-S31-p0.25-causal]', 'test_attention_forward_forms[dh64-S33-p0.25-causal]')),
    'attention_kernel<false, true, false, 3, true, 32, false, false>': ("tests", ('test_attention_forward_forms[dh32-S32-p0.25-full]', 'test_attention_forward_forms[dh32-S96-p0.25-full]', 'test_attention_backward_forms[dh32-S96-p0.25-full]')),
    'attention_kernel<false, true, false, 3, true, 32, false, true>': ("tests", ('test_attention_forward_forms[dh32-S32-p0.25-causal]', 'test_attention_forward_forms[dh32-S96-p0.25-causal]', 'test_attention_backward_forms[dh32-S96-p0.25-causal]')),
    'attention_kernel<false, true, false, 3, true, 32, true, false>': ("tests", ('test_attention_forward_forms[dh32-S1-p0.25-full]', 'test_attention_forward_forms[dh32-S31-p0.25-full]', 'test_attention_forward_forms[dh32-S33-p0.25-full]')),
    'attention_kernel<false, true, false, 3, true, 32, true, true>': ("tests", ('test_attention_forward_forms[dh32-S1-p0.25-causal]', 'test_attention_forward_forms[dh32-S31-p0.25-causal]', 'test_attention_forward_forms[dh32-S33-p0.25-causal]')),
    'attention_kernel<false, true, false, 3, true, 64, false, false>': ("tests", ('test_attention_forward_forms[dh64-S32-p0.25-full]', 'test_attention_forward_forms[dh64-S96-p0.25-full]', 'test_attention_backward_forms[dh64-S96-p0.25-full]')),
    'attention_kernel<false, true, false, 3, true, 64, false, true>': ("tests", ('test_attention_forward_forms[dh64-S32-p0.25-causal]', 'test_attention_forward_forms[dh64-S96-p0.25-causal]', 'test_attention_backward_forms[dh64-S96-p0.25-causal]')),
    'attention_kernel<false, true, false, 3, true, 64, true, false>': ("tests", ('test_attention_forward_forms[dh64-S1-p0.25-full]', 'test_attention_forward_forms[dh64-S31-p0.25-full]', 'test_attention_forward_forms[dh64-S33-p0.25-full]')),
    'attention_kernel<false, true, false, 3, true, 64, true, true>': ("tests", ('test_attention_forward_forms[dh64-S1-p0.25-causal]', 'test_attention_forward_forms[dh64-S31-p0.25-causal]', 'test_attention_forward_forms[dh64-S33-p0.25-causal]')),
    'attention_kernel<false, true, true, 1, false, 128, false, false>': ("tests", ('test_attention_forward_forms[dh128-S128-p0.25-full]', 'test_attention_forward_forms[dh128-S256-p0.25-full]')),
    'attention_kernel<false, true, true, 1, false, 128, false, true>': ("tests", ('test_attention_forward_forms[dh128-S128-p0.25-causal]', 'test_attention_forward_forms[dh128-S256-p0.25-causal]')),
    'attention_kernel<false, true, true, 1, true, 128, false, false>': ("tests", ('test_attention_forward_forms[dh128-S128-p0.25-full]', 'test_attention_forward_forms[dh128-S256-p0.25-full]', 'test_attention_backward_forms[dh128-S128-p0.25-full]')),
    'attention_kernel<false, true, true, 1, true, 128, false, true>': ("tests", ('test_attention_forward_forms[dh128-S128-p0.25-causal]', 'test_attention_forward_forms[dh128-S256-p0.25-causal]', 'test_attention_backward_forms[dh128-S128-p0.25-causal]')),
    'attention_kernel<false, true, true, 2, true, 32, false, false>': ("tests", ('test_attention_forward_forms[dh32-S128-p0.25-full]', 'test_attention_forward_forms[dh32-S256-p0.25-full]')),
    'attention_kernel<false, true, true, 2, true, 64, false, false>': ("tests", ('test_attention_forward_forms[dh64-S128-p0.25-full]', 'test_attention_forward_forms[dh64-S256-p0.25-full]')),
    'attention_kernel<false, true, true, 3, false, 32, false, false>': ("tests", ('test_attention_forward_forms[dh32-S128-p0.25-full]', 'test_attention_forward_forms[dh32-S256-p0.25-full]')),
    'attention_kernel<false, true, true, 3, false, 32, false, true>': ("tests", ('test_attention_forward_forms[dh32-S128-p0.25-causal]', 'test_attention_forward_forms[dh32-S256-p0.25-causal]')),
    'attention_kernel<false, true, true, 3, false, 64, false, false>': ("tests", ('test_attention_forward_forms[dh64-S128-p0.25-full]', 'test_attention_forward_forms[dh64-S256-p0.25-full]')),
    'attention_kernel<false, true, true, 3, false, 64, false, true>': ("tests", ('test_attention_forward_forms[dh64-S128-p0.25-causal]', 'test_attention_forward_forms[dh64-S256-p0.25-causal]')),
    'attention_kernel<false, true, true, 3, true, 32, false, false>': ("tests", ('test_attention_forward_forms[dh32-S128-p0.25-full]', 'test_attention_forward_forms[dh32-S256-p0.25-full]', 'test_attention_backward_forms[dh32-S128-p0.25-full]')),
    'attention_kernel<false, true, true, 3, true, 32, false, true>': ("tests", ('test_attention_forward_forms[dh32-S128-p0.25-causal]', 'test_attention_forward_forms[dh32-S256-p0.25-causal]', 'test_attention_backward_forms[dh32-S128-p0.25-causal]')),
    'attention_kernel<false, true, true, 3, true, 64, false, false>': ("tests", ('test_attention_forward_forms[dh64-S128-p0.25-full]', 'test_attention_forward_forms[dh64-S256-p0.25-full]', 'test_attention_backward_forms[dh64-S128-p0.25-full]')),
    'attention_kernel<false, true, true, 3, true, 64, false, true>': ("tests", ('test_attention_forward_forms[dh64-S128-p0.25-causal]', 'test_attention_forward_forms[dh64-S256-p0.25-causal]', 'test_attention_backward_forms[dh64-S128-p0.25-causal]')),
    'attention_kernel<true, false, false, 1, true, 128, false, false>': ("tests", ('test_attention_backward_forms[dh128-S96-p0.0-full]', 'test_attention_backward_forms[dh128-S160-p0.0-full]')),
    'attention_kernel<true, false, false, 1, true, 128, false, true>': ("tests", ('test_attention_backward_forms[dh128-S96-p0.0-causal]', 'test_attention_backward_forms[dh128-S160-p0.0-causal]')),
    'attention_kernel<true, false, false, 1, true, 128, true, false>': ("tests", ('test_attention_backward_forms[dh128-S33-p0.0-full]',)),
    'attention_kernel<true, false, false, 1, true, 128, true, true>': ("tests", ('test_attention_backward_forms[dh128-S33-p0.0-causal]',)),
    'attention_kernel<true, false, false, 2, true, 32, false, false>': ("tests", ('test_attention_backward_forms[dh32-S96-p0.0-full]', 'test_attention_backward_forms[dh32-S160-p0.0-full]')),
    'attention_kernel<true, false, false, 2, true, 32, false, true>': ("tests", ('test_attention_backward_forms[dh32-S96-p0.0-causal]', 'test_attention_backward_forms[dh32-S160-p0.0-causal]')),
    'attention_kernel<true, false, false, 2, true, 32, true, false>': ("tests", ('test_attention_backward_forms[dh32-S33-p0.0-full]',)),
    'attention_kernel<true, false, false, 2, true, 32, true, true>': ("tests", ('test_attention_backward_forms[dh32-S33-p0.0-causal]',)),
    'attention_kernel<true, false, false, 2, true, 64, false, false>': ("tests", ('test_attention_backward_forms[dh64-S96-p0.0-full]', 'test_attention_backward_forms[dh64-S160-p0.0-full]')),
    'attention_kernel<true, false, false, 2, true, 64, false, true>': ("tests", ('test_attention_backward_forms[dh64-S96-p0.0-causal]', 'test_attention_backward_forms[dh64-S160-p0.0-causal]')),
    'attention_kernel<true, false, false, 2, true, 64, true, false>': ("tests", ('test_attention_backward_forms[dh64-S33-p0.0-full]',)),
    'attention_kernel<true, false, false, 2, true, 64, true, true>': ("tests", ('test_attention_backward_forms[dh64-S33-p0.0-causal]',)),
    'attention_kernel<true, false, true, 1, true, 128, false, false>': ("tests", ('test_attention_backward_forms[dh128-S128-p0.0-full]',)),
    'attention_kernel<true, false, true, 1, true, 128, false, true>': ("tests", ('test_attention_backward_forms[dh128-S128-p0.0-causal]',)),
    'attention_kernel<true, false, true, 2, true, 32, false, false>': ("tests", ('test_attention_backward_forms[dh32-S128-p0.0-full]',)),
    'attention_kernel<true, false, true, 2, true, 32, false, true>': ("tests", ('test_attention_backward_forms[dh32-S128-p0.0-causal]',)),
    'attention_kernel<true, false, true, 2, true, 64, false, false>': ("tests", ('test_attention_backward_forms[dh64-S128-p0.0-full]',)),
    'attention_kernel<true, false, true, 2, true, 64, false, true>': ("tests", ('test_attention_backward_forms[dh64-S128-p0.0-causal]',)),
    'attention_kernel<true, true, false, 1, true, 128, false, false>': ("tests", ('test_attention_backward_forms[dh128-S96-p0.25-full]', 'test_attention_backward_forms[dh128-S160-p0.25-full]')),
    'attention_kernel<true, true, false, 1, true, 128, false, true>': ("tests", ('test_attention_backward_forms[dh128-S96-p0.25-causal]', 'test_attention_backward_forms[dh128-S160-p0.25-causal]')),
    'attention_kernel<true, true, false, 1, true, 128, true, false>': ("tests", ('test_attention_backward_forms[dh128-S33-p0.25-full]',)),
    'attention_kernel<true, true, false, 1, true, 128, true, true>': ("tests", ('test_attention_backward_forms[dh128-S33-p0.25-causal]',)),
    'attention_kernel<true, true, false, 2, true, 32, false, false>': ("tests", ('test_attention_backward_forms[dh32-S96-p0.25-full]', 'test_attention_backward_forms[dh32-S160-p0.25-full]')),
    'attention_kernel<true, true, false, 2, true, 32, false, true>': ("tests", ('test_attention_backward_forms[dh32-S96-p0.25-causal]', 'test_attention_backward_forms[dh32-S160-p0.25-causal]')),
    'attention_kernel<true, true, false, 2, true, 32, true, false>': ("tests", ('test_attention_backward_forms[dh32-S33-p0.25-full]',)),
    'attention_kernel<true, true, false, 2, true, 32, true, true>': ("tests", ('test_attention_backward_forms[dh32-S33-p0.25-causal]',)),
    'attention_kernel<true, true, false, 2, true, 64, false, false>': ("tests", ('test_attention_backward_forms[dh64-S96-p0.25-full]', 'test_attention_backward_forms[dh64-S160-p0.25-full]')),
    'attention_kernel<true, true, false, 2, true, 64, false, true>': ("tests", ('test_attention_backward_forms[dh64-S96-p0.25-causal]', 'test_attention_backward_forms[dh64-S160-p0.25-causal]')),
    'attention_kernel<true, true, false, 2, true, 64, true, false>': ("tests", ('test_attention_backward_forms[dh64-S33-p0.25-full]',)),
    'attention_kernel<true, true, false, 2, true, 64, true, true>': ("tests", ('test_attention_backward_forms[dh64-S33-p0.25-causal]',)),
    'attention_kernel<true, true, true, 1, true, 128, false, false>': ("tests", ('test_attention_backward_forms[dh128-S128-p0.25-full]',)),
    'attention_kernel<true, true, true, 1, true, 128, false, true>': ("tests", ('test_attention_backward_forms[dh128-S128-p0.25-causal]',)),
    'attention_kernel<true, true, true, 2, true, 32, false, false>': ("tests", ('test_attention_backward_forms[dh32-S128-p0.25-full]',)),
    'attention_kernel<true, true, true, 2, true, 32, false, true>': ("tests", ('test_attention_backward_forms[dh32-S128-p0.25-causal]',)),
    'attention_kernel<true, true, true, 2, true, 64, false, false>': ("tests", ('test_attention_backward_forms[dh64-S128-p0.25-full]',)),
    'attention_kernel<true, true, true, 2, true, 64, false, true>': ("tests", ('test_attention_backward_forms[dh64-S128-p0.25-causal]',)),
}


def _rows(built_names):
    rows = []
    for kernel in built_names:
        entry, condition = _describe(kernel)
        if kernel in _UNREACHABLE:
            rows.append(Row(kernel, entry, condition, unreachable=_UNREACHABLE[kernel]))
        else:
            how, what = _REACHED[kernel]
            rows.append(Row(kernel, entry, condition, tests=what) if how == "tests" else Row(kernel, entry, condition, covered_by=what))
    return rows


ROWS = _rows(sorted(set(_REACHED) | set(_UNREACHABLE)))
