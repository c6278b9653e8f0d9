"""Ledger of the streaming switch: one entry per call site of `nk_streams_past_cache(bytes)` (neuronika_amd/csrc/nk_common.h,
`bytes > 384 MiB`), the launch-time choice between plain and `nt` loads and stores of the HBM-bound kernels.

Every entry says where the site is, the bytes expression as the source writes it, the passes it switches, whether the switch reaches
the kernel as a template parameter or as a run-time bit, the largest call the suite made into it before
tests/test_gpu_streaming_switch.py existed (with the arithmetic), and the test that crosses it.  `bytes` restates the expression over
the names of `shape`, the call of the crossing test: tests/test_streaming_sites.py holds `bytes(**shape) > THRESHOLD` for every
entry, and the GPU tests assert the same from here before they launch, so a changed formula fails a test and does not go quiet.

tests/test_streaming_sites.py compares (file, expression) of this list with a regex over csrc/: a new site fails there until it has
an entry.  A site may appear twice in a file with the same expression (`bytes` in nk_pool.hip); the comparison counts them."""
from collections import namedtuple

THRESHOLD = 384 << 20          # nk_streams_past_cache: bytes > (size_t(384) << 20)
SOURCE_LINE = "static inline bool nk_streams_past_cache(size_t bytes_touched) { return bytes_touched > (size_t(384) << 20); }"

Site = namedtuple("Site", "file entry expr passes switch largest largest_bytes bytes shape test")

NEW = "tests/test_gpu_streaming_switch.py::"
PAST_CACHE = "tests/test_gpu_dispatch_paths.py::test_past_cache_switch"
# the buffers of test_past_cache_switch: n = 32769 * 1024 + 3, m = n - 3
_N, _M = 32769 * 1024 + 3, 32769 * 1024

SITES = [
    # ---- nk_layout.hip -------------------------------------------------------------------------------------------------------
    Site("nk_layout.hip", "nk_dropout_bwd", "n * 16", "dropout backward `+=` and assign (g, noise, dx)", "run-time bit",
         "test_past_cache_switch, n = 32769 * 1024 + 3", _N * 16, lambda n: n * 16, dict(n=_N), PAST_CACHE),
    # ---- nk_optim_multi.h ----------------------------------------------------------------------------------------------------
    Site("nk_optim_multi.h", "nk_adamw_step_multi", "bytes", "the AdamW step; bytes = sum n[i] * (max_exp_avg_sq ? 36 : 28)", "run-time bit",
         "test_gpu_adamw.py LIST: 1 Mi + 5 and 38 short entries, 1 109 806 elements * 28 (36 with amsgrad)", 1109806 * 36,
         lambda n, amsgrad: n * (36 if amsgrad else 28), dict(n=(384 << 20) // 28 // 4 * 4 + 4 + 3, amsgrad=False),
         NEW + "test_adamw_step"),
    Site("nk_optim_multi.h", "nk_clip_grad_norm_multi", "elems * 8", "the scale pass of the clip (one read, one write); the norm's sum is not switched",
         "run-time bit", "test_gpu_adamw.py LIST: 1 109 806 elements * 8", 1109806 * 8,
         lambda elems: elems * 8, dict(elems=(384 << 20) // 8 + 4 + 3), NEW + "test_clip_grad_norm"),
    # ---- nk_pool.hip ---------------------------------------------------------------------------------------------------------
    Site("nk_pool.hip", "nk_max_pool_fwd / nk_avg_pool_fwd", "bytes", "windowed forward; bytes = (planes * in_plane + planes * out_plane * (idx ? 2 : 1)) * 4",
         "run-time bit", "test_gpu_fullsize_pooling.py stem: (128, 64, 112, 112) -> 56 x 56 with idx",
         (128 * 64 * 112 * 112 + 128 * 64 * 56 * 56 * 2) * 4,
         lambda planes, in_plane, out_plane, idx: (planes * in_plane + planes * out_plane * (2 if idx else 1)) * 4,
         dict(planes=128 * 64, in_plane=112 * 112, out_plane=56 * 56, idx=True), "tests/test_gpu_fullsize_pooling.py::test_stem_max_pool_3_2_1"),
    Site("nk_pool.hip", "nk_max_pool_bwd / nk_avg_pool_bwd (+ _assign)", "bytes",
         "the windowed max backward is what the named test runs; the plane kernels and the windowed average backward take the same bit and "
         "are crossed by no test; bytes = (planes * in_plane * (assign ? 1 : 2) + planes * out_plane * (MAX ? 2 : 1)) * 4", "run-time bit",
         "test_gpu_fullsize_pooling.py stem, `+=`: (128, 64, 112, 112) <- 56 x 56 with idx",
         (128 * 64 * 112 * 112 * 2 + 128 * 64 * 56 * 56 * 2) * 4,
         lambda planes, in_plane, out_plane, assign, is_max: (planes * in_plane * (1 if assign else 2) + planes * out_plane * (2 if is_max else 1)) * 4,
         dict(planes=128 * 64, in_plane=112 * 112, out_plane=56 * 56, assign=True, is_max=True),
         "tests/test_gpu_fullsize_pooling.py::test_stem_max_pool_3_2_1"),
    # ---- nk_rope.h -----------------------------------------------------------------------------------------------------------
    Site("nk_rope.h", "nk_rope_fwd / nk_rope_bwd / nk_rope_bwd_assign", "items * (il ? 16 : (size_t)32) * (ACC ? 3 : 2)",
         "the vector family of all three entries; items = B * T * NH * (rot / (il ? 4 : 8) + (dh - rot) / 4), 0 pass-through items in place",
         "template parameter NT of rope_vec_kernel<IL, INV, ACC, NT>",
         "test_gpu_rope.py: 201 rows x 16 heads x 128, half-split `+=`: 201 * 16 * 16 items * 32 * 3", 201 * 16 * 16 * 32 * 3,
         lambda rows, NH, dh, rot, il, acc: rows * NH * (rot // (4 if il else 8) + (dh - rot) // 4) * (16 if il else 32) * (3 if acc else 2),
         dict(rows=24577, NH=16, dh=128, rot=128, il=False, acc=False), NEW + "test_rope"),
    # ---- nk_reduce.hip -------------------------------------------------------------------------------------------------------
    Site("nk_reduce.hip", "nk_mse_bwd (+ _assign)", "n * (assign ? 12 : 16)", "MSE backward (MODE >= 2; sum and mean backward read no operand)",
         "run-time bit", "test_past_cache_switch, `+=`, n = 32769 * 1024 + 3", _N * 16,
         lambda n, assign: n * (12 if assign else 16), dict(n=_N, assign=False), PAST_CACHE),
    Site("nk_reduce.hip", "nk_softmax_bwd / nk_log_softmax_bwd (+ _assign)", "(size_t)outer * L * 12", "the row kernels of softmax and log-softmax backward",
         "run-time bit", "test_past_cache_switch, (32769, 1024)", 32769 * 1024 * 12,
         lambda outer, L: outer * L * 12, dict(outer=32769, L=1024), PAST_CACHE),
    Site("nk_reduce.hip", "nk_scale_softmax_dropout_bwd (+ _assign, _from_scores)", "(size_t)rows * L * 12",
         "the fused attention-probability backward, stored and recomputed probabilities", "run-time bit",
         "test_gpu_parity.py::test_attention_probs_paths_agree_at_benchmark_width, (512, 1024)", 512 * 1024 * 12,
         lambda rows, L: rows * L * 12, dict(rows=32769, L=1024), NEW + "test_attention_probs_bwd"),
    # ---- nk_batchnorm.hip ----------------------------------------------------------------------------------------------------
    Site("nk_batchnorm.hip", "nk_batch_norm_bwd (+ _assign)", "(size_t)N * C * L * 4 * (DxOp<ASSIGN, INFER>::NIN + 1)",
         "dx as a map; NIN = g (+ x in training) (+ dx for `+=`)", "run-time bit",
         "test_gpu_fullsize_batchnorm.py: (128, 128, 3136), training assign, NIN = 2", 128 * 128 * 3136 * 4 * 3,
         lambda N, C, L, nin: N * C * L * 4 * (nin + 1), dict(N=128, C=128, L=3136, nin=2), "tests/test_gpu_fullsize_batchnorm.py::test_c3_output"),
    Site("nk_batchnorm.hip", "nk_batch_norm_bwd_sums", "(size_t)N * C * L * 8", "the channel sums of the backward (g and x read once)", "run-time bit",
         "test_gpu_fullsize_batchnorm.py: (128, 128, 3136)", 128 * 128 * 3136 * 8,
         lambda N, C, L: N * C * L * 8, dict(N=128, C=128, L=3136), "tests/test_gpu_fullsize_batchnorm.py::test_c3_output"),
    # ---- nk_cross_entropy.h --------------------------------------------------------------------------------------------------
    Site("nk_cross_entropy.h", "nk_cross_entropy_bwd (+ _assign)", "(size_t)s.positions * C * (ASSIGN ? 8 : 12)",
         "backward: the block kernel is what the named test runs (C = 50257); the row and generic kernels take the same bit and are crossed by no test",
         "run-time bit", "test_gpu_fullsize_cross_entropy.py: (16384, 32000), `+=`", 16384 * 32000 * 12,
         lambda positions, C, assign: positions * C * (8 if assign else 12), dict(positions=8192, C=50257, assign=True),
         "tests/test_gpu_fullsize_cross_entropy.py::test_language_model_heads[8192-50257]"),
    # ---- nk_activation.h -----------------------------------------------------------------------------------------------------
    Site("nk_activation.h", "nk_activation_bwd (+ _assign)", "n * (ASSIGN ? 12 : 16)", "GELU / GELU-tanh / SiLU / sigmoid backward", "run-time bit",
         "test_gpu_fullsize_activation.py: 8192 x 4096; `+=` 2^25 * 16 crosses, assign 2^25 * 12 is the threshold itself and does not",
         (1 << 25) * 16, lambda n, assign: n * (12 if assign else 16), dict(n=(1 << 25) + 4 + 3, assign=True), NEW + "test_activation_bwd_assign"),
    Site("nk_activation.h", "nk_glu_bwd (+ _assign)", "(size_t)items * 4 * (ASSIGN ? 5 : 7)", "the vector kernel of the gated backward; items = rows * H",
         "run-time bit", "test_gpu_fullsize_activation.py: rows = 8192, H = 11008, `+=`", 8192 * 11008 * 4 * 7,
         lambda items, assign: items * 4 * (5 if assign else 7), dict(items=8192 * 11008, assign=True),
         "tests/test_gpu_fullsize_activation.py::test_swiglu_feed_forward"),
    # ---- nk_norm.hip ---------------------------------------------------------------------------------------------------------
    Site("nk_norm.hip", "nk_layer_norm_bwd / nk_rms_norm_bwd (+ _assign)", "(size_t)rows * D * (assign ? 12 : 16)",
         "dx of both norms, row-in-registers kernels only (the general kernels take no switch; neither does any forward)", "run-time bit",
         "test_gpu_fullsize_layernorm.py 32768 x 1024 and test_gpu_fullsize_rms_norm.py 8192 x 4096, assign: 2^25 * 12 is the threshold "
         "itself and does not cross", (1 << 25) * 12,
         lambda rows, D, assign: rows * D * (12 if assign else 16), dict(rows=32769, D=1024, assign=True), NEW + "test_norm_dx"),
    Site("nk_norm.hip", "nk_layer_norm_bwd_params / nk_rms_norm_bwd_gamma (+ _assign)", "(size_t)rows * D * 8",
         "stage 1 of the parameter gradients (g and x read once), VEC = 4 loads", "run-time bit",
         "the same calls: 2^25 * 8 = 256 MiB", (1 << 25) * 8,
         lambda rows, D: rows * D * 8, dict(rows=49153, D=1024), NEW + "test_norm_params"),
    # ---- nk_elementwise.hip --------------------------------------------------------------------------------------------------
    Site("nk_elementwise.hip", "nk_binary_bwd_left / nk_binary_bwd_right (+ _assign), same shape", "(size_t)total * (assign ? 8 : 12)",
         "binary backward without a reduced axis", "run-time bit", "test_past_cache_switch, `+=`, total = 32769 * 1024", _M * 12,
         lambda total, assign: total * (8 if assign else 12), dict(total=_M, assign=False), PAST_CACHE),
    Site("nk_elementwise.hip", "nk_relu_bwd (+ _assign)", "n * (assign ? 12 : 16)", "ReLU backward", "run-time bit",
         "test_past_cache_switch, `+=`, n = 32769 * 1024 + 3", _N * 16,
         lambda n, assign: n * (12 if assign else 16), dict(n=_N, assign=False), PAST_CACHE),
    Site("nk_elementwise.hip", "nk_relu_mask_inplace", "n * 12", "the in-place ReLU mask, vector kernel", "run-time bit",
         "test_past_cache_switch, n = 32769 * 1024 + 3", _N * 12, lambda n: n * 12, dict(n=_N), PAST_CACHE),
]

# 19 call sites in ten files; the definition's own line in nk_common.h is pinned by SOURCE_LINE and is no entry


def site(entry_prefix):
    """the one entry whose `entry` starts with the given text"""
    found = [s for s in SITES if s.entry.startswith(entry_prefix)]
    assert len(found) == 1, (entry_prefix, [s.entry for s in found])
    return found[0]


def crosses(s, **shape):
    return s.bytes(**shape) > THRESHOLD
