/*
 * neuronika_hip.h — C ABI of the MI355X (gfx950) dense-tensor backend for neuronika's
 * Var/VarDiff op graph.
 *
 * This is the drop-in boundary.  The reference has no FFI of its own:
 * the seam is the pair of crate-private traits
 *     trait Forward  { fn forward(&self);  }   neuronika-variable/src/autograd.rs:7-12
 *     trait Backward { fn backward(&self); }   neuronika-variable/src/autograd.rs:20-25
 * implemented by node structs that own handles to their operand/output buffers.  Each entry
 * point below replaces the BODY of one such `forward()` / `backward()` (cited per function);
 * the reference's own accelerator template (`neuronika-variable/src/cuda/`) shows the shape a
 * backend takes: a `Device` handle (cuda/device.rs:11-58), a device array replacing
 * `ndarray::Array` (cuda/cuarray.rs:10-19) and nodes that call the library in `forward()`
 * (cuda/cunode/binary_op/mod.rs:55-82).  INTEGRATION.md shows the Rust binding.
 *
 * Conventions (identical to the reference's ndarray path):
 *   - every tensor is dense f32, C-contiguous (row-major), described by (pointer, shape[]);
 *   - every *_fwd OVERWRITES its output (GEMM beta = 0); every *_bwd ACCUMULATES (`+=`)
 *     into the operand gradient (GEMM beta = 1);
 *   - the host owns every device buffer; the library never keeps a data pointer past a call;
 *   - calls are asynchronous on the device's compute stream, in call (= tape) order; the host
 *     synchronises only in nk_download / nk_device_sync / nk_event_* queries;
 *   - one host thread per nk_device (the reference graph is Rc<RefCell<..>>, i.e. !Send);
 *     different devices may be driven from different threads / processes concurrently;
 *   - every function returns NK_OK (0) or an error code; nk_last_error() gives the message
 *     of the calling thread's last failure.  The reference convention is panic
 *     (`.unwrap()`, cuda/device.rs:36-45; `assert!`, utils.rs:438-496): a host binding turns
 *     a non-zero status into a panic.  Shape validation that the reference does on the host
 *     (`check_conv_args`, `cobroadcast`) is repeated here and reported as NK_ERR_INVALID.
 *
 * No torch / C++ types cross this boundary: plain pointers, sizes and scalars only.
 */
#ifndef NEURONIKA_HIP_H
#define NEURONIKA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nk_device nk_device; /* cuda/device.rs:11-16  `Device`            */
typedef struct nk_event nk_event;   /* hipEvent on a device stream (timing/ordering) */
typedef struct nk_comm nk_comm;     /* one rank of a RCCL communicator (net-new)  */

enum nk_status {
    NK_OK = 0,
    NK_ERR_INVALID = 1,     /* bad argument / shape (reference: assert!/panic!)      */
    NK_ERR_HIP = 2,         /* HIP runtime failure                                   */
    NK_ERR_RCCL = 3,        /* RCCL failure                                          */
    NK_ERR_OOM = 4,         /* device allocation failed                              */
    NK_ERR_UNSUPPORTED = 5  /* valid in the reference, not implemented by this build */
};

enum nk_binary_op { NK_ADD = 0, NK_SUB = 1, NK_MUL = 2, NK_DIV = 3 };
enum nk_reduction { NK_REDUCTION_SUM = 0, NK_REDUCTION_MEAN = 1 }; /* lib.rs:29-36 */

#define NK_MAX_DIMS 8

/* ------------------------------------------------------------------ lifecycle ---------- */
/* `Device::new(idx)` cuda/device.rs:34-58.  Creates the compute stream and the side
 * (communication) stream of GPU `idx`. */
int nk_device_count(int* out);
int nk_device_create(int idx, nk_device** out);
int nk_device_destroy(nk_device* dev);
int nk_device_sync(nk_device* dev);
int nk_device_index(const nk_device* dev);
void* nk_stream_compute(nk_device* dev); /* hipStream_t */
void* nk_stream_comm(nk_device* dev);    /* hipStream_t */
const char* nk_last_error(void);
const char* nk_version(void);
/* Development overrides of the kernels' launch heuristics, per device handle (the library reads NO environment variable):
 *   NK_TUNE_GEMM_FORCE     values = ti, tj, splits[, tiles per block[, tile-order group height[, look-ahead threshold]]]
 *                          (ti, tj in {1, 2}: 64- or 128-wide tile sides); n = 0 returns to the rules
 *   NK_TUNE_GEMM_KPAIR     values[0] = -1 rule / 0 never / 1 k-pair blocks, lock-step groups / 2 skewed groups
 *   NK_TUNE_ATTENTION_OCC  values[0] = 0 rule / 2: forward register budget sized for two blocks per CU
 *   NK_TUNE_GEMM_PAIR      values[0] = -1 rule / 0 nk_sgemm_pair always launches twice / 1 one launch whenever eligible
 *   NK_TUNE_CONV_NARROW    values[0] = 0 the conv kernel gradient's uniform launch / 1..100 its mixed launch (the last, half-empty
 *                          column tile through 64-wide blocks), a narrow block's k-tile priced at that percentage of a wide one's;
 *                          n = 0: the measured rules (65 % with 128-row tiles, 80 % with 64-row tiles)
 *   NK_TUNE_CONV_WINOGRAD  values[0] = -1 rule / 0 the 3x3 stride-1 forward and input gradient never take the Winograd F(2x2, 3x3)
 *                          kernels (implicit GEMM as in rounds 1 - 4) / 1 whenever the shape allows (also below the block-count rule);
 *                          values[1] (optional) = -1 rule / 0 no staggered start of its persistent blocks / > 0 the stagger unit in
 *                          shader clocks (blocks one tile block short of the longest walk start 1 - 3 units late);
 *                          values[2] (optional) = -1 rule / 0 narrow blocks (two waves, 64 output channels, chunks of 16 reduction
 *                          channels) / 1 wide blocks (four waves, 128 channels, chunks of 32) where the channel counts allow both;
 *                          values[3] (optional) = -1 rule / 0 the kernel gradient never takes its Winograd F(3x3, 2x2) form / 1 whenever
 *                          the shape allows (64 | both channel counts)
 *   NK_TUNE_GEMM_CHAIN     values[0] = -1 rule / 0 an unsplit GEMM sums K as ONE f32 chain whatever its length / L (a multiple of 64):
 *                          unsplit plain-epilogue GEMMs (MatMul, MatMulT, weight gradients) with K > L run as consecutive launches
 *                          over equal pieces of K, each on top of the last (beta = 1): chains of at most L.  Rule: L = 2048 - what
 *                          keeps 4096- and 8192-long contractions inside 1e-6 K |a| |b| of the f64 result (SURVEY.md 8c ii; the
 *                          reference's matrixmultiply sums K in cache blocks too, matrix_matrix_mul/mod.rs:33-39)
 *   NK_TUNE_CONV_S2DX      values[0] = -1 rule / 0 the 3x3 stride-2 input gradient never takes its fused-phase kernel (the four stride
 *                          phases of a tile in one block walk; per-phase implicit GEMMs as in rounds 1 - 5) and the 3x3 stride-2 forward
 *                          never its tap-plane kernel (by rule only with 128 | output channels and eight or more blocks per CU) / 1 whenever the shape
 *                          allows (one group, even input extents, padding 0 or 1 alike on both axes, 64 | input channels, 16 | output
 *                          channels) / 2, 3: the same with narrow (two waves, 64 channels) / wide (four waves, 128 channels) blocks forced
 *   NK_TUNE_GEMM_WINDOW    values[0] = 0 rule / W > 0: the aligned 128 x 128 GEMM launches (NN, NT, TN, 256-thread blocks) load their
 *                          tiles through buffer descriptors - 32-bit byte offsets from the block's tile origin - only while the window
 *                          a tile spans in EACH operand is at most W bytes: (127 ld + K) * 4 for an operand whose k runs along its
 *                          rows, (K ld + 128) * 4 for one whose k runs down its columns.  Rule: W = 2^31 - 1.  A launch above the limit
 *                          takes the guarded instantiations of the same layout, tile and epilogue (64-bit base per k-tile, 32-bit
 *                          element offsets inside it, one k-tile of look-ahead); both give the same bits.  k-pair blocks are decided
 *                          first and are not affected.  A small W lets a test reach that route with small matrices.
 *   NK_TUNE_QUANT_ROWS     values[0] = -1 rule / 0 nk_quant_linear_fwd never takes its rows kernels (always unpack + GEMM) / L > 0 the
 *                          rows kernels for M <= L, in ceil(M / 8) passes.  Rule: L = nk_quant_linear_rows_rule(bits)
 * For schedule sweeps (benchmarks/ab_*.py) and the tests that pit one schedule against another bit for bit; results never
 * depend on them beyond summation order (split-K, chain length, algorithm). */
enum { NK_TUNE_GEMM_FORCE = 0, NK_TUNE_GEMM_KPAIR = 1, NK_TUNE_ATTENTION_OCC = 2, NK_TUNE_GEMM_PAIR = 3, NK_TUNE_CONV_NARROW = 4,
       NK_TUNE_CONV_WINOGRAD = 5, NK_TUNE_GEMM_CHAIN = 6, NK_TUNE_CONV_S2DX = 7, NK_TUNE_GEMM_WINDOW = 8, NK_TUNE_QUANT_ROWS = 9 };
int nk_dev_tune(nk_device* dev, int knob, const int* values, int n);
/* How many GEMM launches on this handle took the buffer-addressed kernels so far (NK_TUNE_GEMM_WINDOW decides per launch; a launch
 * sent to the guarded instantiations instead does not count). */
int nk_gemm_buffer_launches(nk_device* dev, uint64_t* count);
/* The num_records (bytes) of the buffer descriptor a block on that path builds for one operand: the window of its R-row tile
 * at (row0, k0) up to k = kend, clipped to the operand's extent (`rows` rows or columns, leading dimension ld, floats).
 * k_contiguous: element (row, k) at X[row * ld + k], else at X[k * ld + row].  Host arithmetic only, shared with the kernels. */
long long nk_gemm_buffer_records(int k_contiguous, int R, long long ld, int row0, int rows, int k0, int kend);
/* How many convolution launches on this handle took the Winograd F(2x2, 3x3) kernels so far (forward + input gradient; the rule
 * of NK_TUNE_CONV_WINOGRAD decides per launch).  For harnesses that must say which algorithm produced a time: bench.py quotes the
 * C3 roofline on the DIRECT algorithmic flops of node/convolution/mod.rs:85-123,146-189 and states beside it what was executed. */
int nk_conv_winograd_launches(nk_device* dev, uint64_t* count);
/* Tell the device handle that `n` of the GPU's resident-block slots (two 128x128 GEMM blocks per CU) are held by work on another
 * stream until further notice - the channel workgroups of an all-reduce in flight beside the backward pass
 * (vardiff.rs:125-141 -> optimizer.rs:81-86 is where the exchange sits; dp::GradientSync sets it when it hands the first
 * gradient over and clears it in join()).  GEMM launches whose tile count no longer divides the free slots then run whole
 * rounds of one tile per block and cut the left-over tiles along K (sgemm_tail_kernel, nk_gemm.hip): deterministic, bits a
 * function of (shape, n); every tile outside the left-over rectangle is the plain launch's.  n = 0 (the default): the chip is
 * ours, plain launches.  0 <= n <= CUs. */
int nk_device_set_busy_slots(nk_device* dev, int n);

/* ------------------------------------------------------------------ memory ------------- */
/* `CuArray::zeroed` cuda/cuarray.rs:35-42; outputs and gradients are allocated zeroed at
 * graph-build time (var.rs:224,1041; gradient.rs:47-54). */
int nk_alloc_zeroed(nk_device* dev, size_t n_f32, float** out);
int nk_free(nk_device* dev, float* ptr);
/* `CuArray::from_slice / from_ndarray` cuda/cuarray.rs:62-72,114-117 (H2D) */
int nk_upload(nk_device* dev, float* dst, const float* host_src, size_t n);
/* `CuArray::as_ndarray` cuda/cuarray.rs:101-106 (D2H, synchronises the compute stream) */
int nk_download(nk_device* dev, float* host_dst, const float* src, size_t n);
/* root-gradient seeding `grad_mut().fill(seed)` vardiff.rs:133; `zero_grad` vardiff.rs:100-102;
 * `Gradient::with_grad` re-zero gradient.rs:71-78 */
int nk_fill(nk_device* dev, float* ptr, size_t n, float value);
int nk_copy(nk_device* dev, float* dst, const float* src, size_t n);

/* H2D input pipeline = the device half of `for batch in dataset.batch(n)` (neuronika-data/src/lib.rs:81,570):
 * page-locked host staging + a third (copy) stream, so that the upload of batch k+1 overlaps the compute of
 * batch k.  nk_upload_async returns immediately; order it against the compute stream with events recorded /
 * waited on stream 2. */
int nk_host_alloc(size_t bytes, void** out);
int nk_host_free(void* ptr);
int nk_upload_async(nk_device* dev, float* dst, const float* pinned_src, size_t n);

/* ------------------------------------------------------------------ events ------------- */
int nk_event_create(nk_device* dev, nk_event** out);
int nk_event_destroy(nk_event* ev);
int nk_event_record(nk_event* ev, int on_comm_stream); /* 0: compute stream, 1: comm stream, 2: copy stream */
int nk_event_sync(nk_event* ev);
int nk_event_elapsed_ms(nk_event* start, nk_event* stop, float* ms);
int nk_stream_wait_event(nk_device* dev, int on_comm_stream, nk_event* ev);

/* ------------------------------------------------------------------ graph capture ------ */
/* Small graphs (the reference's quickstart MLP: 64x3 inputs) are launch-bound: tens of kernels of a few
 * microseconds each.  Everything a tape step enqueues on the compute stream between nk_graph_begin and nk_graph_end
 * is recorded into a hipGraph instead of executed; nk_graph_launch replays it with one submission.  The captured
 * region must not synchronise with the host (no nk_download / nk_device_sync / item()) nor grow an allocation, and
 * it replays the SAME launches: scalars baked into kernel arguments (the learning rate) stay what they were at capture
 * time.  A captured SGD / RMSProp / undecayed-Adagrad step therefore keeps the rate it was captured with: `set_lr` or an
 * lr_scheduler step after the capture changes the host's value, not what a replay applies - capture again after
 * changing the rate (tests/test_gpu_tape_optim.py pins this).  Calls whose kernel arguments must change from call to
 * call REFUSE to be captured (NK_ERR_INVALID) instead of freezing them: optimizer steps that depend on the step count (nk_adam_step, nk_adamw_step, nk_adamw_step_multi: 1 - beta^step; nk_adagrad_step with
 * lr_decay != 0), and the forwards that draw a dropout mask (nk_dropout_fwd / nk_scale_softmax_dropout_fwd /
 * nk_attention_fwd with train != 0 and 0 < p < 1: the Philox offset - every replay would drop the same elements).
 * SGD / RMSProp steps, nk_clip_grad_norm_multi, evaluation-mode and p = 0 dropout capture fine.  A workspace the
 * device outgrows later stays allocated while any nk_graph of that device exists (captured kernels keep its address);
 * destroy a device's graphs before the device. */
typedef struct nk_graph nk_graph;
int nk_graph_begin(nk_device* dev);
int nk_graph_end(nk_device* dev, nk_graph** out);
int nk_graph_launch(nk_graph* graph);
int nk_graph_destroy(nk_graph* graph);
/* For host-side set-up that uploads with a synchronising copy (nn::Segments): NK_ERR_INVALID, with `what` in the message, while the
 * compute stream is being captured - checked BEFORE anything touches the stream, so the capture stays valid, as nk_rope_table's
 * own refusal; NK_OK otherwise.  Nothing is launched or copied. */
int nk_graph_refuse_capture(nk_device* dev, const char* what);

/* ------------------------------------------------------------------ kernel timing ------ */
/* Bench instrumentation: between nk_profile_begin and nk_profile_end every launch of the
 * MFMA kernels is bracketed by a HIP event pair on the compute stream.  nk_profile_end
 * synchronises and returns, for one kernel class, the number of launches, the sum of their
 * durations and the algorithmic flop they performed (2*M*N*K per GEMM; 2*N*Cout*L*K per conv
 * pass). */
enum nk_kernel_class { NK_KERNEL_SGEMM = 0, NK_KERNEL_CONV = 1, NK_KERNEL_ATTENTION = 2 };
int nk_profile_begin(nk_device* dev);
/* Suspends (paused != 0) / resumes the bracketing inside a window without dropping its records: an event pair costs the stream
 * ~10 us per launch, so a harness may instrument every n-th step of its timed region instead of all of them. */
int nk_profile_pause(nk_device* dev, int paused);
int nk_profile_end(nk_device* dev, int kernel_class, int* launches, double* total_ms, double* total_flop);

/* ------------------------------------------------------------------ GEMM (MFMA) -------- */
/* Row-major C(MxN) = alpha * op(A)(MxK) * op(B)(KxN) + beta * C; op(X) = X or X^T
 * (trans != 0: the stored matrix is the transpose, i.e. A is stored KxM with leading
 * dimension lda).  Replaces `ndarray::linalg::general_mat_mul` at its six call sites:
 * node/matrix_matrix_mul/mod.rs:33,65,97 and node/matrix_matrix_mul_t/mod.rs:33,65,97. */
int nk_sgemm(nk_device* dev, int transA, int transB, int M, int N, int K, float alpha,
             const float* A, int lda, const float* B, int ldb, float beta, float* C, int ldc);
/* Batched over a two-level batch index b = bo * batch_inner + bi; operand offset =
 * bo * stride_outer + bi * stride_inner (elements).  Used by the composed multi-head
 * attention: bo = sample, bi = head, so Q_bh is a strided view of the (B*S) x d projection. */
int nk_sgemm_batched(nk_device* dev, int transA, int transB, int M, int N, int K, float alpha,
                     const float* A, int lda, long long sAo, long long sAi,
                     const float* B, int ldb, long long sBo, long long sBi, float beta,
                     float* C, int ldc, long long sCo, long long sCi,
                     int batch_outer, int batch_inner);

/* Two independent products in ONE launch: C0 = op(A0).op(B0) + beta0*C0 and C1 = op(A1).op(B1) + beta1*C1 (alpha = 1).  When
 * neither product fills the chip by itself (1024^3: 256 blocks, one per CU) the two grids run side by side - every CU gets the
 * second resident block a large launch has, and launch boundary, dispatch ramp and tail are paid once.  Taken by rule for
 * aligned, unsplit (NN | NT | TN) + TN pairs of equal tile shape whose blocks together fit the chip's resident slots; two
 * ordinary launches otherwise (and whenever an output overlaps the other product's output or operands).  Every output is the fma chain nk_sgemm gives it without k-pair blocks (NK_TUNE_GEMM_KPAIR = 0):
 * bit-identical to two calls under that setting. */
int nk_sgemm_pair(nk_device* dev,
                  int transA0, int transB0, int M0, int N0, int K0, const float* A0, int lda0, const float* B0, int ldb0,
                  float beta0, float* C0, int ldc0,
                  int transA1, int transB1, int M1, int N1, int K1, const float* A1, int lda1, const float* B1, int ldb1,
                  float beta1, float* C1, int ldc1);
/* ... over a two-level batch (nk_sgemm_batched's strides, per operand): the dK / dV products of the attention backward (one
 * launch at small batch x heads; C5's 2 x 4096 blocks measure 0.5 - 1 % faster as two launches and stay two) */
int nk_sgemm_pair_batched(nk_device* dev, int batch_outer, int batch_inner,
                          int transA0, int transB0, int M0, int N0, int K0, const float* A0, int lda0, long long sA0o, long long sA0i,
                          const float* B0, int ldb0, long long sB0o, long long sB0i, float beta0, float* C0, int ldc0,
                          long long sC0o, long long sC0i,
                          int transA1, int transB1, int M1, int N1, int K1, const float* A1, int lda1, long long sA1o, long long sA1i,
                          const float* B1, int ldb1, long long sB1o, long long sB1i, float beta1, float* C1, int ldc1,
                          long long sC1o, long long sC1i);

/* Node-level wrappers, one per reference forward()/backward() body. */
/* MatrixMatrixMul::forward  node/matrix_matrix_mul/mod.rs:31-41   C(n,o) = A(n,m).B(m,o) */
int nk_mm_fwd(nk_device* dev, const float* A, const float* B, float* C, int n, int m, int o);
/* MatrixMatrixMulBackwardLeft::backward  :63-73    dA(n,m) += G(n,o).B(m,o)^T */
int nk_mm_bwd_left(nk_device* dev, float* dA, const float* G, const float* B, int n, int m, int o);
/* MatrixMatrixMulBackwardRight::backward :95-105   dB(m,o) += A(n,m)^T.G(n,o) */
int nk_mm_bwd_right(nk_device* dev, float* dB, const float* A, const float* G, int n, int m, int o);
/* MatrixMatrixMulBackward::backward :121-126 (both operands differentiable: `self.left.backward(); self.right.backward()`)
 * as one call = nk_sgemm_pair of the two products above; assign_x != 0: that gradient is freshly zeroed, written unread. */
int nk_mm_bwd(nk_device* dev, float* dA, float* dB, const float* G, const float* A, const float* B, int n, int m, int o,
              int assign_a, int assign_b);
/* MatrixMatrixMulT::forward  node/matrix_matrix_mul_t/mod.rs:31-41  C(n,o) = A(n,m).B(o,m)^T */
int nk_mm_t_fwd(nk_device* dev, const float* A, const float* B, float* C, int n, int m, int o);
/* MatrixMatrixMulTBackwardLeft::backward  :63-73   dA(n,m) += G(n,o).B(o,m) */
int nk_mm_t_bwd_left(nk_device* dev, float* dA, const float* G, const float* B, int n, int m, int o);
/* MatrixMatrixMulTBackwardRight::backward :95-105  dB(o,m) += G(n,o)^T.A(n,m) */
int nk_mm_t_bwd_right(nk_device* dev, float* dB, const float* G, const float* A, int n, int m, int o);
/* MatrixMatrixMulTBackward::backward :121-126, both products as one call (see nk_mm_bwd) */
int nk_mm_t_bwd(nk_device* dev, float* dA, float* dB, const float* G, const float* A, const float* B, int n, int m, int o,
                int assign_a, int assign_b);

/* `Linear::forward` neuronika-nn/src/lib.rs:425-447  Y(n,o) = X(n,m).W(o,m)^T + b(o): the MatrixMatrixMulT node
 * (matrix_matrix_mul_t/mod.rs:31-41) and the broadcast Addition node (addition/mod.rs:39-50) as ONE kernel - the
 * bias is added to the f32 accumulator in the GEMM epilogue, bit-identical to the two-node result.  Its backward is
 * nk_mm_t_bwd_left (dX += G.W), nk_mm_t_bwd_right (dW += G^T.X) and nk_unbroadcast_add (db += column sums of G). */
int nk_linear_fwd(nk_device* dev, const float* X, const float* W, const float* bias, float* Y, int n, int m, int o);
/* `Linear::forward` followed by `ReLU::forward` (node/relu/mod.rs:29-38) as ONE kernel: Y = max(X.W^T + b, 0), the ReLU
 * applied to the f32 value the Linear epilogue would have stored (`o.max(0.)`: a NaN gives 0) - bit-identical to the two
 * launches; the pre-activation is never written.  ReLU's backward needs only `x > 0`, and max(x, 0) > 0 <=> x > 0, so Y
 * itself is the mask (nk_linear_bwd_input_relu, nk_relu_mask_inplace). */
int nk_linear_relu_fwd(nk_device* dev, const float* X, const float* W, const float* bias, float* Y, int n, int m, int o);
/* MatrixMatrixMulTBackwardLeft::backward (matrix_matrix_mul_t/mod.rs:63-73) followed by ReLUBackward::backward
 * (relu/mod.rs:67-79) of the node that produced this Linear's input X(n,m) = max(Z, 0):
 *   dZ(n,m) (+)= mask * (G(n,o).W(o,m)),  mask = ((X > 0.) as usize as f32)   (0 * inf = NaN, as the reference's product)
 * applied when the GEMM tile is stored: the gradient w.r.t. X is never written.  assign != 0: dZ is a freshly zeroed
 * gradient, written without being read. */
int nk_linear_bwd_input_relu(nk_device* dev, float* dZ, const float* G, const float* W, const float* X, int n, int m, int o,
                             int assign);
/* ReLUBackward::backward in place: g = ((y > 0.) as f32) * g  (the fused Linear+ReLU node's fallback when a consumer other
 * than nk_linear_bwd_input_relu wrote into its gradient; idempotent, so contributions that arrived masked stay as they are) */
int nk_relu_mask_inplace(nk_device* dev, float* g, const float* y, size_t n);

/* ------------------------------------------------------------------ convolution -------- */
/* N-d (nd = 1,2,3) cross-correlation without internal padding, NC[D]HW layout.
 *   x: [N, Cin, in...]   w: [Cout, Cin/groups, k...]   y: [N, Cout, out...]
 *   out_i = (in_i - dilation_i*(k_i-1) - 1)/stride_i + 1          utils.rs:207-237
 * x_shape has 2+nd entries, w_shape 2+nd entries.
 * Convolution::forward            node/convolution/mod.rs:331-355 (-> :85-144)  y  = conv(x,w)
 * ConvolutionBackwardInput        :427-449 (-> :146-189, 256-274)               dx += ...
 * ConvolutionBackwardKernel       :488-510 (-> :191-226, 276-294)               dw += ...
 * Algorithms, chosen inside each call by geometry and size (rules in csrc/nk_conv.hip, overridable through nk_dev_tune): Winograd
 * F(2x2, 3x3) (forward, input gradient) and F(3x3, 2x2) (kernel gradient) on the f32 MFMA core for 3 x 3 / stride 1 / dilation 1 / one
 * group with 64 | channel counts and any output extents from 2 x 2 on (odd ones through instantiations with masked border tiles); implicit GEMM on the same core for channel counts that are multiples of 32 and
 * a generic form for the rest; direct kernels for <= 16 channels per group.  Every form sums in a fixed order (run-to-run identical);
 * the forms differ from each other in that order only (equal on integer-valued data, to contraction tolerance otherwise). */
int nk_conv_fwd(nk_device* dev, int nd, const float* x, const int* x_shape, const float* w,
                const int* w_shape, float* y, const int* stride, const int* dilation, int groups);
int nk_conv_bwd_input(nk_device* dev, int nd, float* dx, const int* x_shape, const float* g,
                      const float* w, const int* w_shape, const int* stride, const int* dilation,
                      int groups);
int nk_conv_bwd_kernel(nk_device* dev, int nd, float* dw, const int* w_shape, const float* g,
                       const float* x, const int* x_shape, const int* stride, const int* dilation,
                       int groups);
/* `Conv{1,2,3}d` module forward = convolution node + broadcast Addition of the (Cout,1,..) bias (neuronika-nn/src/
 * lib.rs:630-916; addition/mod.rs:39-50) as ONE kernel: bias[co] is added to the f32 accumulator in the epilogue,
 * bit-identical to the two-node result.  Backward = nk_conv_bwd_input, nk_conv_bwd_kernel, nk_unbroadcast_add. */
int nk_conv_bias_fwd(nk_device* dev, int nd, const float* x, const int* x_shape, const float* w,
                     const int* w_shape, const float* bias, float* y, const int* stride,
                     const int* dilation, int groups);
/* The same module's backward towards its kernel AND its bias in one pass: ConvolutionBackwardKernel (convolution/mod.rs:
 * 191-226) plus AdditionBackwardRight of the (Cout,1,..) bias (addition/mod.rs:109-135), db[co] (+)= sum of g over samples
 * and positions.  The implicit-GEMM pass stages g as its A operand anyway and sums it on the way (no separate 200 MB
 * reduction at C3); geometries that take other kernels run the reduction behind the scenes.  `assign_*` != 0: first write. */
int nk_conv_bwd_kernel_bias(nk_device* dev, int nd, float* dw, float* db, const int* w_shape, const float* g,
                            const float* x, const int* x_shape, const int* stride, const int* dilation, int groups,
                            int assign_dw, int assign_db);
/* The `Conv2d` module (lib.rs:724-812: pad -> convolution -> + bias) with Zero padding FOLDED INTO the forward and the kernel-gradient
 * pass: `x` / `x_shape` are the UNPADDED input, `padding[i]` the symmetric zero padding of spatial axis i; the padded copy (Pad::forward,
 * pad/zero/mod.rs:5-31 - 110 MB and a 40 us kernel at C3) is never made.  Only the Winograd kernels read their operands through
 * out-of-range-is-zero buffer loads, so only their geometries fold: 3 x 3, stride 1, dilation 1, one group, padding 0 or 1 per axis (not
 * all zero), 64 | both channel counts.  nk_conv_padding_folds answers, for a geometry and the rules in force on the
 * handle, whether BOTH passes would run their Winograd kernels anyway (*folds = 1: build the module node without the Pad node and
 * call the two `_padded` entries; 0: pad, then nk_conv_bias_fwd / nk_conv_bwd_kernel_bias).  The `_padded` entries themselves fold for
 * every geometry the kernels can (whatever the block-count rules say); for the others - and when the rules in force at CALL time decline,
 * e.g. a nk_dev_tune change after the graph was built - they are the two nodes they stand for: Pad::forward into a scratch region of the
 * device handle, then the convolution entry on the copy (any nd, stride, dilation, groups; never NK_ERR_UNSUPPORTED).  Same values as the
 * two-node form, bit for bit, either way (zeros are read instead of stored).  bias / db may be NULL.  The input gradient's padded form is
 * below. */
int nk_conv_padding_folds(nk_device* dev, int nd, const int* x_shape, const int* padding, const int* w_shape, const int* stride,
                          const int* dilation, int groups, int* folds);
int nk_conv_bias_fwd_padded(nk_device* dev, int nd, const float* x, const int* x_shape, const int* padding, const float* w,
                            const int* w_shape, const float* bias, float* y, const int* stride, const int* dilation, int groups);
int nk_conv_bwd_kernel_bias_padded(nk_device* dev, int nd, float* dw, float* db, const int* w_shape, const float* g, const float* x,
                                   const int* x_shape, const int* padding, const int* stride, const int* dilation, int groups,
                                   int assign_dw, int assign_db);
/* `Conv{1,2,3}d` module backward towards its input when the module's padding mode is Zero (lib.rs:630-916: pad ->
 * convolution): ConvolutionBackwardInput (convolution/mod.rs:146-189) followed by PadBackward (pad/mod.rs:131-181, the
 * centre block of the padded gradient is accumulated into dx) as ONE kernel.  x_shape is the UNPADDED input
 * [N, Cin, in...], `padding[i]` the symmetric zero padding of spatial axis i the forward convolution saw; only the
 * columns dx needs are computed and the padded gradient is never stored.  Same values as the two-node form.  `_assign`:
 * see the first-write variants below. */
int nk_conv_bwd_input_padded(nk_device* dev, int nd, float* dx, const int* x_shape, const int* padding,
                             const float* g, const float* w, const int* w_shape, const int* stride,
                             const int* dilation, int groups);
int nk_conv_bwd_input_padded_assign(nk_device* dev, int nd, float* dx, const int* x_shape,
                                    const int* padding, const float* g, const float* w,
                                    const int* w_shape, const int* stride, const int* dilation,
                                    int groups);
/* Pad<Constant|Zero>::forward  node/pad/mod.rs:97-129 + pad/constant/mod.rs:14-39;
 * symmetric `padding[i]` on both sides of spatial axis i.  x_shape = [N, C, in...]. */
int nk_pad_const_fwd(nk_device* dev, int nd, const float* x, const int* x_shape, float* y,
                     const int* padding, float value);
/* Pad<Reflective>::forward  pad/reflective/mod.rs:9-136 (border i<pad reads index pad-i, i>=len+pad reads
 * 2(len-1)-(i-pad); requires padding[i] < in[i]);  Pad<Replicative>::forward  pad/replicative/mod.rs:9-134
 * (borders repeat the edge element).  Same shapes as nk_pad_const_fwd. */
int nk_pad_reflective_fwd(nk_device* dev, int nd, const float* x, const int* x_shape, float* y,
                          const int* padding);
int nk_pad_replicative_fwd(nk_device* dev, int nd, const float* x, const int* x_shape, float* y,
                           const int* padding);
/* PadBackward::backward  node/pad/mod.rs:157-181   dx += centre(g)  (every padding mode: the reference
 * does not fold the border gradients back for Reflective/Replicative, neither do we) */
int nk_pad_bwd(nk_device* dev, int nd, float* dx, const int* x_shape, const float* g,
               const int* padding);

/* ------------------------------------------------------------------ broadcast binaries - */
/* Addition|Subtraction|Multiplication|Division::forward node/<op>/mod.rs:39-50.
 * out_shape must equal cobroadcast(l_shape, r_shape) (utils.rs:97-125). */
int nk_binary_fwd(nk_device* dev, int op, float* out, const int* out_shape, int out_nd,
                  const float* l, const int* l_shape, int l_nd,
                  const float* r, const int* r_shape, int r_nd);
/* <Op>BackwardLeft::backward : d_left += unbroadcast(local),
 *   add/sub: local = g; mul: g*r; div: g/r            (addition/mod.rs:86-91, subtraction
 *   :87-92, multiplication :91-103, division :90-99).  `l` may be NULL for add/sub/mul/div
 *   (unused); `r` is needed for mul/div. */
int nk_binary_bwd_left(nk_device* dev, int op, float* d_left, const int* l_shape, int l_nd,
                       const float* g, const int* g_shape, int g_nd,
                       const float* r, const int* r_shape, int r_nd);
/* <Op>BackwardRight::backward : d_right += unbroadcast(local),
 *   add: g; sub: -g; mul: g*l; div: -g*l/r^2          (addition/mod.rs:129-134, subtraction
 *   :130-136, multiplication :138-149, division :139-149). */
int nk_binary_bwd_right(nk_device* dev, int op, float* d_right, const int* r_shape, int r_nd,
                        const float* g, const int* g_shape, int g_nd,
                        const float* l, const int* l_shape, int l_nd, const float* r);
/* `utils::accumulate` (utils.rs:152-192) with the INTENDED semantics: dst += src summed
 * over every axis dst lacks or has with extent 1 (the reference's lane-axis choice is
 * defective for non-square shapes; not replicated). */
int nk_unbroadcast_add(nk_device* dev, float* dst, const int* dst_shape, int dst_nd,
                       const float* src, const int* src_shape, int src_nd);
/* ReLU::forward node/relu/mod.rs:29-38; ReLUBackward::backward :67-79 (dx += (x>0)*g) */
int nk_relu_fwd(nk_device* dev, const float* x, float* y, size_t n);
int nk_relu_bwd(nk_device* dev, float* dx, const float* g, const float* x, size_t n);

/* Pointwise unary nodes ("next" row f-2): forward y = f(x) overwrites; backward dx += f'(.)*g with
 * `ref` = the buffer the reference node keeps (its INPUT for ln, softplus, leaky_relu, pow; its
 * OUTPUT for exp, sqrt, sigmoid, tanh; unused for neg).  node/<op>/mod.rs:35 and :73-86.
 *   NEG   y = -x                       dx -= g                       negation
 *   EXP   y = exp(x)                   dx += g*y                     exp
 *   LN    y = ln(x)                    dx += g/x                     logn
 *   SQRT  y = sqrt(x)                  dx += g/(y*2)                 sqrt
 *   SIGMOID y = 1/(1+exp(-x))          dx += g*y*(1-y)               sigmoid
 *   TANH  y = tanh(x)                  dx += g*(1-y^2)               tanh
 *   SOFTPLUS y = ln(1+exp(x))          dx += g/(1+exp(-x))           softplus
 *   LEAKY_RELU y = x>0 ? x : 0.01x     dx += (x>0)*g + (x<=0)*0.01   leaky_relu (sic: the reference
 *                                       adds 0.01, not 0.01*g — leaky_relu/mod.rs:77-80; replicated)
 *   POW   y = x^e (integer e = iparam) dx += g * x^(e-1) * e         power */
enum nk_unary_op { NK_NEG = 0, NK_EXP = 1, NK_LN = 2, NK_SQRT = 3, NK_SIGMOID = 4, NK_TANH = 5,
                   NK_SOFTPLUS = 6, NK_LEAKY_RELU = 7, NK_POW = 8 };
int nk_unary_fwd(nk_device* dev, int op, const float* x, float* y, size_t n, int iparam);
int nk_unary_bwd(nk_device* dev, int op, float* dx, const float* g, const float* ref, size_t n, int iparam);

/* ------------------------------------------------------------------ reductions --------- */
/* Sum::forward node/sum/mod.rs:28-35 ; SumBackward :60-67 (dx += g, g a device scalar) */
int nk_sum_fwd(nk_device* dev, const float* x, size_t n, float* out);
int nk_sum_bwd(nk_device* dev, float* dx, size_t n, const float* g);
/* Mean::forward node/mean/mod.rs:28-35 ; MeanBackward :60-72 (dx += g/len) */
int nk_mean_fwd(nk_device* dev, const float* x, size_t n, float* out);
int nk_mean_bwd(nk_device* dev, float* dx, size_t n, const float* g);
/* SquaredError::forward node/squared_error/mod.rs:42-59 ; backward :94-123 */
int nk_mse_fwd(nk_device* dev, const float* x, const float* target, size_t n, int reduction,
               float* out);
int nk_mse_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* target,
               size_t n, int reduction);

/* ------------------------------------------------------------------ first-write variants */
/* The reference allocates every gradient zeroed (gradient.rs:47-54) and every backward node `+=`s into it.
 * For the FIRST node writing into a gradient of the current pass, `0 + v` needs neither the memset nor the
 * read of the destination: the `_assign` variants compute exactly what their `+=` twin computes on an all-zero
 * destination, writing without reading (the GEMM-shaped nodes get the same through nk_sgemm's beta = 0).  Only nodes
 * whose backward covers the WHOLE destination have a twin (not Chunk's tile update or NLL's scatter).
 * The tape (host `Gradient`) keeps the zero fill pending and hands it to the first writer. */
int nk_conv_bwd_input_assign(nk_device* dev, int nd, float* dx, const int* x_shape, const float* g,
                             const float* w, const int* w_shape, const int* stride,
                             const int* dilation, int groups);
int nk_conv_bwd_kernel_assign(nk_device* dev, int nd, float* dw, const int* w_shape, const float* g,
                              const float* x, const int* x_shape, const int* stride,
                              const int* dilation, int groups);
int nk_binary_bwd_left_assign(nk_device* dev, int op, float* d_left, const int* l_shape, int l_nd,
                              const float* g, const int* g_shape, int g_nd, const float* r,
                              const int* r_shape, int r_nd);
int nk_binary_bwd_right_assign(nk_device* dev, int op, float* d_right, const int* r_shape, int r_nd,
                               const float* g, const int* g_shape, int g_nd, const float* l,
                               const int* l_shape, int l_nd, const float* r);
int nk_unbroadcast_assign(nk_device* dev, float* dst, const int* dst_shape, int dst_nd,
                          const float* src, const int* src_shape, int src_nd);
int nk_unary_bwd_assign(nk_device* dev, int op, float* dx, const float* g, const float* ref, size_t n,
                        int iparam);
int nk_softmax_bwd_assign(nk_device* dev, float* dx, const float* g, const float* y, const int* shape,
                          int nd, int axis);
int nk_log_softmax_bwd_assign(nk_device* dev, float* dx, const float* g, const float* y,
                              const int* shape, int nd, int axis);
int nk_dropout_bwd_assign(nk_device* dev, float* dx, const float* g, const float* noise, size_t n,
                          double p, int train);
int nk_concat_bwd_part_assign(nk_device* dev, float* d_operand, const float* g, const int* g_shape,
                              int nd, int axis, int offset, int op_len);
int nk_transpose_bwd_assign(nk_device* dev, float* dx, const float* g, const int* x_shape, int nd);
int nk_sum_bwd_assign(nk_device* dev, float* dx, size_t n, const float* g);
int nk_mean_bwd_assign(nk_device* dev, float* dx, size_t n, const float* g);
int nk_relu_bwd_assign(nk_device* dev, float* dx, const float* g, const float* x, size_t n);
int nk_mse_bwd_assign(nk_device* dev, float* dx, const float* g, const float* x, const float* target,
                      size_t n, int reduction);
int nk_pad_bwd_assign(nk_device* dev, int nd, float* dx, const int* x_shape, const float* g,
                      const int* padding);
int nk_split_heads_bwd_assign(nk_device* dev, float* dx, const float* g, int B, int S, int H, int dh);
int nk_merge_heads_bwd_assign(nk_device* dev, float* dx, const float* g, int B, int S, int H, int dh);
int nk_scale_softmax_dropout_bwd_assign(nk_device* dev, float* d_scores, const float* g_out,
                                        const float* probs, const float* noise, long long rows, int L,
                                        float scale, double p, int train, uint64_t seed, uint64_t offset);

/* ------------------------------------------------------------------ loss criteria ------- */
/* Element-pair criteria reducing to a scalar; x and target share `shape`.
 *   NK_LOSS_MAE             AbsoluteError        node/absolute_error/mod.rs:42-58, :93-123
 *   NK_LOSS_BCE             BinaryCrossEntropy   node/bce/mod.rs:42-62, :97-127   (ln clamped at -100, bwd denominator >= EPSILON)
 *   NK_LOSS_BCE_WITH_LOGITS BCEWithLogits        node/bce_with_logits/mod.rs:42-66, :101-131
 *   NK_LOSS_KLDIV           KLDiv                node/kldiv/mod.rs:42-59, :92-113  (x = log-probabilities; terms with
 *                           target <= 0 contribute 0 - the masked form the reference's vectors require; Mean divides
 *                           by shape[0], every other criterion by the element count)
 * fwd writes out[0]; bwd: dx += d(loss)/dx * g[0]  (g = device scalar). */
enum nk_loss { NK_LOSS_MAE = 0, NK_LOSS_BCE = 1, NK_LOSS_BCE_WITH_LOGITS = 2, NK_LOSS_KLDIV = 3 };
int nk_loss_fwd(nk_device* dev, int loss, const float* x, const float* target, const int* shape, int nd,
                int reduction, float* out);
int nk_loss_bwd(nk_device* dev, int loss, float* dx, const float* g, const float* x, const float* target,
                const int* shape, int nd, int reduction);
/* NegativeLogLikelihood node/nll/mod.rs:43-69, :104-137 on the documented layout (var.rs:645-661):
 * x (minibatch, C, d1..dk) log-probabilities, target (minibatch, d1..dk) class indices stored as f32 and read
 * with Rust's saturating `as usize` (NaN / negative -> 0, fraction dropped; index >= C selects nothing).
 * fwd: out = -sum x[n, target[n,r], r]  (Mean: / shape[0], :64);  bwd: dx[n, target, r] -= g (Mean: / target.len(), :114) */
int nk_nll_fwd(nk_device* dev, const float* x, const float* target, const int* shape, int nd,
               int reduction, float* out);
int nk_nll_bwd(nk_device* dev, float* dx, const float* g, const float* target, const int* shape, int nd,
               int reduction);

/* ------------------------------------------------------------------ cross entropy */
/* Cross entropy over class logits with integer targets: log-softmax and NLL in one pass.  The reference has no such node (it
 * stops at nll); the semantics are fixed here, chosen so that the result is nk_nll(nk_log_softmax(x, 1), target) wherever that
 * composition is defined.
 *   x: logits (N, C, d1..dk), f32, C-contiguous (NLL's layout).  target: (N, d1..dk) class ids STORED AS f32 and read exactly as
 *   nk_nll_* and nk_embedding_* read them (Rust's saturating `as usize`: NaN and negatives are 0, the fraction is dropped).
 *   positions = N d1 .. dk (at most 2^31 - 1), inner = d1 .. dk.  nd in 2 .. NK_MAX_DIMS.
 *   A position is INACTIVE when its id is >= C (NLL: "selects nothing") or equals `ignore_index` (negative: none).  Inactive
 *   positions add nothing to the loss and receive a zero gradient row, whatever their logits hold.
 *   Per active position p with class t, lse = log sum_c exp(x_c) and label smoothing e = `label_smoothing` in [0, 1):
 *       loss_p = (1 - e) (lse - x_t) + e (lse - mean_c x_c)          d loss_p / d x_c = softmax_c - (1 - e) [c == t] - e / C
 *   NK_REDUCTION_SUM: the sum over the active positions.  NK_REDUCTION_MEAN: that sum divided by the NUMBER OF ACTIVE POSITIONS,
 *   an exact integer count taken on the device, forward and backward alike; with no active position the loss and the gradient
 *   are 0 (torch gives NaN there).  nk_nll's Mean divides the forward by shape[0] and the backward by target.len(): the two
 *   agree with this entry under Mean only for 2-d inputs with every position active, and under Sum always.
 *   The running maximum starts from f32::MIN as the softmax kernels' does, so -inf logits are ordinary; a NaN or +inf logit makes
 *   its position's lse, its loss and (where the position is active) its whole gradient row NaN, as nk_log_softmax + nk_nll do.
 *   fwd: writes out[0] and lse[p] for EVERY position (`positions` floats, active or not).  Nothing of size (N, C) is saved.
 *   bwd: dx += g[0] w (d loss_p / d x), w = 1 (Sum) or 1 / active count (Mean; re-derived from `target` on the device, so bwd
 *        depends on (x, target, lse) only), softmax recomputed as exp(x - lse).  Inactive rows are not touched.
 *   bwd_assign: what bwd leaves in an all-zero tensor, written without reading it (see "first-write variants"): inactive rows are
 *        written as zeros, so the whole destination is covered.
 * No float atomics: per-position losses go to the device workspace and are summed over fixed spans in a fixed order, the count
 * is an integer sum; two calls on the same data give the same bits.  Nothing synchronises or reads the count on the host; the
 * workspace use is 4 positions bytes and a little more, so the calls can be captured into a graph after one eager call of the
 * same sizes.  positions == 0 or C == 0 is a valid empty call: fwd writes out[0] = 0 and no lse, bwd writes nothing.
 * Kernels (documented because tests choose shapes against them).  inner == 1: C <= 2048 one wave per row with the row in
 * registers; larger C one block per row in one pass (256 threads up to C = 16384, 512 up to 65536, 1024 beyond).  Both walk a row
 * as scalars up to the first 16-byte boundary, 16-byte accesses, and scalars after the last: any C, any row start.  The backward
 * forms need x and dx to share their offset from a 16-byte boundary; otherwise, and for inner > 1, generic kernels run (a thread
 * per position, lanes along inner). */
int nk_cross_entropy_fwd(nk_device* dev, const float* x, const float* target, const int* shape, int nd, int reduction,
                         long long ignore_index, double label_smoothing, float* lse, float* out);
int nk_cross_entropy_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* target, const float* lse,
                         const int* shape, int nd, int reduction, long long ignore_index, double label_smoothing);
int nk_cross_entropy_bwd_assign(nk_device* dev, float* dx, const float* g, const float* x, const float* target, const float* lse,
                                const int* shape, int nd, int reduction, long long ignore_index, double label_smoothing);

/* ------------------------------------------------------------------ smooth and gated activations */
/* GELU, SiLU and the gated (GLU) family: the activation of a transformer's feed-forward block.  Ours: the reference has no such
 * node (its pointwise set is the nk_unary_op one above).  Each is ONE streaming pass forward and ONE backward; the backward keeps
 * the INPUT x and recomputes from it, so nothing but x is saved.
 *   GELU       y = x Phi(x), Phi(x) = 0.5 erfc(-x / sqrt 2)                  y' = Phi(x) + x phi(x), phi(x) = exp(-x^2 / 2) / sqrt(2 pi)
 *              (torch's approximate="none"; the erfc form, so the negative tail does not cancel)
 *   GELU_TANH  y = 0.5 x (1 + tanh u), u = sqrt(2 / pi) (x + 0.044715 x^3)   y' = the derivative of that expression
 *              (torch's approximate="tanh"; evaluated as x sigma(2 u), which is the same function without the cancellation)
 *   SILU       y = x sigma(x), sigma(x) = 1 / (1 + exp(-x))                  y' = sigma(x) (1 + x (1 - sigma(x)))
 *   SIGMOID    y = sigma(x)                                                  y' = sigma(x) (1 - sigma(x))
 *              (here so that torch's plain `glu` is expressible; the tape's sigmoid() stays the NK_SIGMOID unary node)
 * A NaN stays in its own element.  For every finite f32 x, y and y' are finite and no inf * 0 is formed: sigma is taken from
 * exp(-|v|), x^3 may overflow into it, x^2 is clamped where y' has already reached its limit, exp(-x^2 / 2) underflows to 0.
 *   fwd: y = act(x), n elements.   bwd: dx += g act'(x).   bwd_assign: what bwd leaves in an all-zero dx, written without
 *   reading it (see "first-write variants").
 * Gated form over the two halves of the last axis: x is (rows, 2 H) contiguous, y and g are (rows, H);
 *       y[r, j] = x[r, j] act(x[r, H + j])          (a = x[r, j], b = x[r, H + j])
 *       dx[r, j] (+)= g[r, j] act(b)                dx[r, H + j] (+)= g[r, j] a act'(b)
 *   act = SIGMOID is torch's F.glu, GELU is GeGLU, SILU is SwiGLU.  The products are ordinary f32 products: a and act(b) both
 *   near the top of the range overflow as a * b would.
 * Refused with NK_ERR_INVALID, the message naming the argument, before anything else is looked at: an unknown activation; H <= 0;
 * rows < 0; rows * 2 H beyond the index type of the gated kernels (2^31 - 1 elements); a null pointer or one that is not 16-byte
 * aligned (every allocation of this library is; an offset view must keep the alignment).  The device handle is looked at last.
 * n == 0 and rows == 0 succeed and launch nothing (pointers are then not looked at).
 * Kernels (documented because tests choose shapes against them): 16-byte accesses with a scalar tail of n % 4; the gated form
 * walks (row, j / 4) with 16-byte accesses when H % 4 == 0 and (row, j) with scalars for any other H.  No atomics: two calls on
 * the same data give the same bits. */
enum nk_activation { NK_ACT_GELU = 0, NK_ACT_GELU_TANH = 1, NK_ACT_SILU = 2, NK_ACT_SIGMOID = 3 };
int nk_activation_fwd(nk_device* dev, int act, const float* x, float* y, size_t n);
int nk_activation_bwd(nk_device* dev, int act, float* dx, const float* g, const float* x, size_t n);
int nk_activation_bwd_assign(nk_device* dev, int act, float* dx, const float* g, const float* x, size_t n);
int nk_glu_fwd(nk_device* dev, int act, const float* x, float* y, long long rows, int H);
int nk_glu_bwd(nk_device* dev, int act, float* dx, const float* g, const float* x, long long rows, int H);
int nk_glu_bwd_assign(nk_device* dev, int act, float* dx, const float* g, const float* x, long long rows, int H);

/* ------------------------------------------------------------------ GEMV / dot ---------- */
/* MatrixVectorMul node/matrix_vector_mul/mod.rs:31-41  y(n) = A(n,m).x(m);  BackwardLeft :63-69  dA += g (x) x;
 * BackwardRight :92-102  dx += A^T.g */
int nk_mv_fwd(nk_device* dev, const float* A, const float* x, float* y, int n, int m);
int nk_mv_bwd_left(nk_device* dev, float* dA, const float* g, const float* x, int n, int m);
int nk_mv_bwd_right(nk_device* dev, float* dx, const float* A, const float* g, int n, int m);
/* VectorMatrixMul node/vector_matrix_mul/mod.rs:31-41  y(o) = v(m).B(m,o);  BackwardLeft :63-73  dv += B.g;
 * BackwardRight :95-101  dB += v (x) g */
int nk_vm_fwd(nk_device* dev, const float* v, const float* B, float* y, int m, int o);
int nk_vm_bwd_left(nk_device* dev, float* dv, const float* B, const float* g, int m, int o);
int nk_vm_bwd_right(nk_device* dev, float* dB, const float* v, const float* g, int m, int o);
/* VectorVectorMul node/vector_vector_mul/mod.rs:31-34  out = l.r;  backward :57-63  d_operand += other * g[0] */
int nk_vv_fwd(nk_device* dev, const float* l, const float* r, size_t n, float* out);
int nk_vv_bwd(nk_device* dev, float* d_operand, const float* other, const float* g, size_t n);

/* ------------------------------------------------------------------ softmax ------------ */
/* Softmax::forward node/softmax/mod.rs:37-53 ; SoftmaxBackward :84-104
 * LogSoftmax::forward node/logsoftmax/mod.rs:37-53 ; LogSoftmaxBackward :84-102
 * `axis` is any axis of `shape`. */
int nk_softmax_fwd(nk_device* dev, const float* x, float* y, const int* shape, int nd, int axis);
int nk_softmax_bwd(nk_device* dev, float* dx, const float* g, const float* y, const int* shape,
                   int nd, int axis);
int nk_log_softmax_fwd(nk_device* dev, const float* x, float* y, const int* shape, int nd, int axis);
int nk_log_softmax_bwd(nk_device* dev, float* dx, const float* g, const float* y,
                       const int* shape, int nd, int axis);

/* Fused attention probabilities (the Multiplication-by-scalar, Softmax(last axis) and Dropout
 * nodes of the composed multi-head attention in ONE pass over the rows x L score tensor; the
 * module does not exist in the reference — SURVEY.md 8a — its oracle is the composition of
 * node/multiplication, node/softmax and node/dropout, and this produces the same values):
 *   probs = softmax(scores * scale) ; out = dropout(probs)   (mask = Philox(seed, offset), the
 *   same stream nk_dropout_fwd draws; `noise` may be NULL: the mask is then regenerated in the
 *   backward pass instead of being stored).
 * backward: g_p = g_out * mask (no 1/(1-p): reference quirk) ; d_scaled = probs*(g_p - sum(g_p*probs)) ;
 *   d_scores += d_scaled * scale. */
int nk_scale_softmax_dropout_fwd(nk_device* dev, const float* scores, float* probs, float* out, float* noise,
                                 long long rows, int L, float scale, double p, int train, uint64_t seed,
                                 uint64_t offset);
int nk_scale_softmax_dropout_bwd(nk_device* dev, float* d_scores, const float* g_out, const float* probs,
                                 const float* noise, long long rows, int L, float scale, double p, int train,
                                 uint64_t seed, uint64_t offset);
/* Same backward with the probabilities RECOMPUTED from the scores (the forward kernel's exact operation sequence, so
 * bit-identical values): pass `probs = NULL` to nk_scale_softmax_dropout_fwd and the 4-byte/element store plus the
 * buffer disappear.  `assign` != 0: first-write form (see the _assign variants). */
int nk_scale_softmax_dropout_bwd_from_scores(nk_device* dev, float* d_scores, const float* g_out,
                                             const float* scores, const float* noise, long long rows,
                                             int L, float scale, double p, int train, uint64_t seed,
                                             uint64_t offset, int assign);

/* ------------------------------------------------------------------ layer normalisation */
/* LayerNorm over the trailing extent of a contiguous row-major tensor, read as (rows, D) with D the product of the
 * normalised dimensions.  The reference has no such layer; the semantics are fixed here.  Per row, all in f32:
 *   mean = sum(x) / D ;  var = sum((x - mean)^2) / D   (biased; a second pass over the centred values, not E[x^2] - mean^2)
 *   rstd = 1 / sqrt(var + eps) ;  xhat = (x - mean) * rstd ;  y = xhat * gamma + beta     (gamma, beta of D elements)
 * fwd overwrites y and, when `stats` is not NULL, writes stats[rows][2] = {mean, rstd}.  `gamma`, `beta` and `stats` may each be
 * NULL (y = xhat * 1 + 0; nothing kept for a backward pass).  Every D in 1 .. 2^30 and every rows >= 0 is accepted; rows == 0
 * returns NK_OK and writes nothing (in every entry point below, the _assign twins included).  D % 4 == 0 with 16-byte aligned
 * pointers and D <= 16384 takes the kernels that keep the row in registers.  D = 1 gives y = beta; a constant row has var = 0
 * and stays finite through eps; non-finite inputs propagate as the arithmetic produces them, inside their own row only.
 * bwd, with gh = g * gamma (or g when gamma is NULL) and xhat recomputed from x and stats:
 *   dx     += rstd * (gh - mean_D(gh) - xhat * mean_D(gh * xhat))
 *   dgamma += sum over rows of g * xhat ;  dbeta += sum over rows of g        (either output may be NULL, not both)
 * The parameter gradients are summed without atomics (per-row-block partial sums in the device workspace, then a fixed-order
 * final sum whose order depends on (rows, D) alone): every result repeats bit for bit.  Nothing here synchronises or allocates
 * beyond the workspace, so the calls can be captured into a graph.  The `_assign` twins write what their `+=` twin would leave in
 * an all-zero destination, without reading it (see "first-write variants"). */
int nk_layer_norm_fwd(nk_device* dev, const float* x, const float* gamma, const float* beta, float* y, float* stats,
                      long long rows, int D, double eps);
int nk_layer_norm_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats,
                      long long rows, int D);
int nk_layer_norm_bwd_assign(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma,
                             const float* stats, long long rows, int D);
int nk_layer_norm_bwd_params(nk_device* dev, float* dgamma, float* dbeta, const float* g, const float* x,
                             const float* stats, long long rows, int D);
int nk_layer_norm_bwd_params_assign(nk_device* dev, float* dgamma, float* dbeta, const float* g, const float* x,
                                    const float* stats, long long rows, int D);

/* ------------------------------------------------------------------ RMS normalisation */
/* Root-mean-square normalisation over the trailing extent (LLaMA / Mistral / Qwen style).  The reference has no such layer; the
 * semantics are fixed here.  The input is a contiguous row-major tensor read as (rows, D), D the product of the normalised
 * trailing dimensions.  All arithmetic in f32:
 *   ms   = sum(x * x) / D                      (no centring, no mean)
 *   rstd = 1 / sqrt(ms + eps)
 *   xhat = x * rstd ;  y = xhat * gamma        (gamma of D elements, or NULL: y = xhat; there is no beta)
 * fwd overwrites y and, when `stats` is not NULL, writes stats[rows] = rstd (rstd ALONE: half of nk_layer_norm_fwd's record).
 * `gamma` and `stats` may each be NULL (NULL stats: inference, nothing kept).  eps must be finite and >= 0.  Every D in
 * 1 .. 2^30 and every rows >= 0 is accepted; rows == 0 returns NK_OK and writes nothing (in every entry point below, the _assign
 * twins included).  D % 4 == 0 with 16-byte aligned pointers and D <= 16384 takes the kernels that keep the row in registers.
 * bwd, with gh = g * gamma (or g when gamma is NULL), xhat recomputed from x and stats, c = sum(gh * xhat) / D:
 *   dx     += rstd * (gh - xhat * c)
 *   dgamma += sum over rows of g * xhat
 * Nothing is guarded at the edges: an all-zero row gives y = 0 and rstd = 1 / sqrt(eps) (its dx is rstd * gh); at eps = 0 that
 * row is NaN, and only that row; a row whose sum of squares overflows f32 gives rstd = 0 (y = 0 where x is finite); other
 * non-finite inputs propagate as the arithmetic produces them, inside their own row only.  Gemma's (1 + gamma) weight and a
 * bias are not part of it.
 * dgamma is summed without atomics (per-row-block partial sums in the device workspace, then a fixed-order final sum whose
 * order depends on (rows, D) alone): every result repeats bit for bit.  Nothing here synchronises or allocates beyond the
 * workspace, so the calls can be captured into a graph.  The `_assign` twins write what their `+=` twin would leave in an
 * all-zero destination, without reading it (see "first-write variants"). */
int nk_rms_norm_fwd(nk_device* dev, const float* x, const float* gamma, float* y, float* stats, long long rows, int D,
                    double eps);
int nk_rms_norm_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats,
                    long long rows, int D);
int nk_rms_norm_bwd_assign(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma,
                           const float* stats, long long rows, int D);
int nk_rms_norm_bwd_gamma(nk_device* dev, float* dgamma, const float* g, const float* x, const float* stats,
                          long long rows, int D);
int nk_rms_norm_bwd_gamma_assign(nk_device* dev, float* dgamma, const float* g, const float* x, const float* stats,
                                 long long rows, int D);

/* ------------------------------------------------------------------ embedding table */
/* Rows of a (V, D) f32 table selected by id.  The reference has no such layer; the semantics are fixed here.
 *   weight: (V, D) row-major.  idx: n ids STORED AS f32 and read exactly as nk_nll_* reads its targets (Rust's saturating
 *   `as usize`: NaN and negatives are 0, the fraction is dropped).  f32 holds ids exactly up to 2^24: V outside 1 .. 2^24 is
 *   NK_ERR_INVALID, as are n outside 0 .. 2^30 and D outside 1 .. 2^24.  The index tensor may have any shape; it is read flat.
 *   fwd:  out[t, :] = weight[idx[t], :] for t < n (out: (n, D)); an id >= V selects nothing and yields a zero row.
 *   bwd:  dweight[v, :] += the sum over the t with idx[t] == v of g[t, :], summed in f32 in ASCENDING t starting from the first
 *         contribution itself (a row one token selected receives that gradient row as it is, -0.0 included); ids >= V and ids
 *         equal to `padding_idx` contribute nothing; padding_idx < 0 means none.  A row more than 128 tokens selected is summed in
 *         chunks of 128 consecutive contributions, each as above, and the chunks' sums are added in chunk order starting from the
 *         first; 128 is a constant of the library, the same on every device.  dweight[v, :] = dweight[v, :] + that sum, one
 *         addition per element; rows no token selected are not touched.
 *   bwd_assign: what bwd leaves in an all-zero table, written without reading it (see "first-write variants"): rows no token
 *         selected are written as zeros, n == 0 included, so the whole (V, D) destination is covered.
 * No float atomics: an inverted index of the ids (per table row, its token positions ascending) is built in the device workspace
 * on every backward call and each table row has one owner, so every result repeats bit for bit.  Nothing synchronises, and nothing
 * allocates beyond the workspace (4 (2 V + n) bytes and a little more): the calls can be captured into a graph after one eager
 * call of the same sizes.  16-byte accesses where D % 4 == 0 and the pointers are 16-byte aligned, scalar accesses otherwise.
 * n == 0: fwd and bwd write nothing.  Out-of-range ids never read or write outside the buffers. */
int nk_embedding_fwd(nk_device* dev, const float* weight, const float* idx, float* out, long long n, int V, int D);
int nk_embedding_bwd(nk_device* dev, float* dweight, const float* g, const float* idx, long long n, int V, int D,
                     long long padding_idx);
int nk_embedding_bwd_assign(nk_device* dev, float* dweight, const float* g, const float* idx, long long n, int V, int D,
                            long long padding_idx);

/* ------------------------------------------------------------------ batch normalisation */
/* BatchNorm of a contiguous row-major tensor read as (N, C, L), L the product of the extents behind the channel axis (L = 1
 * for an (N, C) input).  The reference has no such layer; the semantics are fixed here.  Per channel c, over its M = N * L values
 * x[n][c][l], all in f32:
 *   mean = sum(x) / M ;  var = sum((x - mean)^2) / M   (biased; centred, not E[x^2] - mean^2)
 * The M values do not fit in registers, so the construction is part of the contract: the channel is cut into chunks, each chunk's
 * mean and centred sum of squares M2 are formed from the registers that hold it (values and means taken relative to an anchor, the
 * first value read or the first partial mean, so that a large common offset costs neither the sums nor the merges their low bits), and the (count, mean, M2) triples are merged
 * pairwise in a fixed order with Chan's formula  M2 = M2a + M2b + delta^2 * na * nb / (na + nb),  delta = mean_b - mean_a.  x is
 * read once for the statistics.
 *   rstd = 1 / sqrt(var + eps) ;  xhat = (x - mean) * rstd ;  y = xhat * gamma + beta     (gamma, beta of C elements)
 * fwd (training) overwrites y, writes stats[C][2] = {mean, rstd} when `stats` is not NULL, and updates in place, each only when
 * its pointer is not NULL,
 *   running_mean = (1 - momentum) * running_mean + momentum * mean
 *   running_var  = (1 - momentum) * running_var  + momentum * var * M / (M - 1)            (unbiased, as torch)
 * in the kernel that finishes the statistics.  M == 1 is NK_ERR_INVALID (one value has no variance); momentum outside [0, 1],
 * a negative or non-finite eps and C <= 0 likewise.  N * L must fit in 31 bits.
 * infer_fwd: mean = running_mean, rstd = 1 / sqrt(running_var + eps), the same y; nothing is updated; `stats` (optional) receives
 * {mean, rstd} for a backward pass through the inference form.
 * Backward, with xhat recomputed from x and stats, s0 = sum(g) and s1 = sum(g * xhat) over the channel:
 *   bwd_sums   sums[C][2] = {s0, s1}, overwritten: one reduction pass feeds dx and both parameter gradients
 *   bwd        dx += gamma * rstd * (g - s0 / M - xhat * s1 / M) ;  with sums == NULL the inference form  dx += gamma * rstd * g
 *              (x may then be NULL too)
 *   bwd_params dgamma += s1 ;  dbeta += s0                                                  (either output may be NULL, not both)
 * `gamma` and `beta` may be NULL (y = xhat * 1 + 0).  N == 0 or L == 0 returns NK_OK and writes nothing (the _assign twins
 * included).  No atomics, and the order of every sum is a function of (N, C, L) and the pointers' 16-byte alignment alone: every
 * output repeats bit for bit.  A non-finite value stays inside its own channel.  Nothing here synchronises or allocates beyond
 * the workspace, no block waits on another, so every call can be captured into a graph.  L % 4 == 0 with L >= 256 and 16-byte
 * aligned pointers takes float4 kernels whose blocks own one channel; L == 1 kernels whose lanes own columns; everything else
 * scalar kernels.  The `_assign` twins write what their `+=` twin would leave in an all-zero destination, without reading it. */
int nk_batch_norm_fwd(nk_device* dev, const float* x, const float* gamma, const float* beta, float* y, float* stats,
                      float* running_mean, float* running_var, int N, int C, int L, double eps, double momentum);
int nk_batch_norm_infer_fwd(nk_device* dev, const float* x, const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, float* y, float* stats, int N, int C, int L, double eps);
int nk_batch_norm_bwd_sums(nk_device* dev, float* sums, const float* g, const float* x, const float* stats, int N, int C,
                           int L);
int nk_batch_norm_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats,
                      const float* sums, int N, int C, int L);
int nk_batch_norm_bwd_assign(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma,
                             const float* stats, const float* sums, int N, int C, int L);
int nk_batch_norm_bwd_params(nk_device* dev, float* dgamma, float* dbeta, const float* sums, int C);
int nk_batch_norm_bwd_params_assign(nk_device* dev, float* dgamma, float* dbeta, const float* sums, int C);

/* ------------------------------------------------------------------ group / instance normalisation */
/* Normalisation over channel groups of a contiguous row-major tensor read as (N, C, L), L the product of the extents behind the
 * channel axis (L = 1 for an (N, C) input).  The reference has no such layer; the semantics are fixed here.  G groups with
 * C % G == 0, Cg = C / G.  Group row r = n * G + j is the D = Cg * L contiguous floats at x + r * D.  Per row, all in f32:
 *   mean = sum(x) / D ;  var = sum((x - mean)^2) / D   (biased; centred, never E[x^2] - mean^2)
 *   rstd = 1 / sqrt(var + eps) ;  xhat = (x - mean) * rstd
 *   y    = xhat * gamma[c] + beta[c] ,  c = j * Cg + (offset in the row) / L              (gamma, beta of C elements)
 * G == C is instance normalisation; G == 1 is layer normalisation over (C, L) with a per-channel affine.  torch's
 * track_running_stats of instance norm is not built.  fwd overwrites y and, when `stats` is not NULL, writes
 * stats[N * G][2] = {mean, rstd}.  `gamma`, `beta` and `stats` may each be NULL.
 * bwd, with gh = g * gamma[c] (or g when gamma is NULL) and xhat recomputed from x and stats:
 *   dx        += rstd * (gh - mean_D(gh) - xhat * mean_D(gh * xhat))
 *   dgamma[c] += sum over n and l of g * xhat ;  dbeta[c] += sum over n and l of g        (either output may be NULL, not both)
 * N * G and D must each fit in 31 bits; element offsets are 64-bit.  N == 0 or L == 0 returns NK_OK and writes nothing (the
 * _assign twins included).  NK_ERR_INVALID before any launch: G <= 0, C <= 0, C % G != 0, an eps that is negative or not finite.
 * D = 1 gives y = beta[c]; a constant row has var = 0 and stays finite through eps; a non-finite input stays inside its own group
 * row.  Three kernel classes, chosen from (Cg, L) and the pointers' 16-byte alignment alone:
 *   D % 4 == 0, aligned, D <= 16384: the row in registers, the statistics formed exactly as nk_layer_norm_fwd forms them - at
 *     G == 1 `stats` equals what nk_layer_norm_fwd(rows = N, D = C * L) writes, bit for bit (y may differ by an FMA contraction);
 *   D % 4 == 0, aligned, D > 16384: the row is cut into chunks of 8192 floats (a constant of the library), each chunk's
 *     (count, mean, M2) is formed in registers relative to an anchor, the row's first value (see batch normalisation), and every
 *     block merges its row's triples in chunk order with Chan's formula; two launches per direction, x (and g) read twice;
 *   anything else: a block per row, scalar accesses, the same construction with chunks of 2048 floats.
 * No atomics, and no block waits on another.  The order of every sum is a function of (Cg, L) and the alignment alone - not of N,
 * G, the device or its CU count - so every output repeats bit for bit, and the bits of a group row's y, stats and dx depend on that
 * row's own x / g and its Cg channels' gamma / beta and on nothing else: a sample run alone gets the bits it gets inside a batch.
 * For dgamma / dbeta (per-(n, c) sums in the workspace, then a fixed-order sum over n) the order also depends on N.  Nothing
 * here synchronises or allocates beyond the workspace: the calls can be captured into a graph after one eager call of the same
 * sizes.  The `_assign` twins write what their `+=` twin would leave in an all-zero destination, without reading it (see
 * "first-write variants"). */
int nk_group_norm_fwd(nk_device* dev, const float* x, const float* gamma, const float* beta, float* y, float* stats,
                      long long N, int C, long long L, int G, double eps);
int nk_group_norm_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats,
                      long long N, int C, long long L, int G);
int nk_group_norm_bwd_assign(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma,
                             const float* stats, long long N, int C, long long L, int G);
int nk_group_norm_bwd_params(nk_device* dev, float* dgamma, float* dbeta, const float* g, const float* x,
                             const float* stats, long long N, int C, long long L, int G);
int nk_group_norm_bwd_params_assign(nk_device* dev, float* dgamma, float* dbeta, const float* g, const float* x,
                                    const float* stats, long long N, int C, long long L, int G);

/* ------------------------------------------------------------------ pooling */
/* Max and average pooling of a contiguous f32 tensor x of shape (N, C, in_1 .. in_nd), nd = 1, 2, 3.  The reference has no pooling;
 * the semantics are fixed here and they are torch's (max_pool / avg_pool 1d, 2d, 3d).  Per spatial axis i: window k_i >= 1, stride
 * s_i >= 1, symmetric padding 0 <= p_i <= k_i / 2.  Dilation is 1 and the output extent is floored: there is no ceil_mode and no
 * dilation argument.
 *   out_i = (in_i + 2 p_i - k_i) / s_i + 1            (integer division)
 * x_shape has 2 + nd entries, kernel / stride / padding nd entries each.  NK_ERR_INVALID, with nothing launched and nothing written:
 * nd outside 1..3, a negative N or C, in_i < 1, a parameter outside the ranges above, out_i <= 0 (the window exceeds the padded
 * extent), or a plane (prod in_i or prod out_i) that does not fit in 31 bits.  nk_pool_out_shape is that arithmetic and those rules on
 * the host (y_shape: 2 + nd entries; no device is needed); the other six entries call it.  N * C == 0 returns NK_OK and writes
 * nothing, the _assign twins included.
 * Max pooling.  y[n][c][o] = the maximum over the in-range positions of window o; padding is never selected (it acts as -inf).
 *   idx[n][c][o] (int32) = the offset of the selected element inside its own (n, c) input plane, (d * in_2 + h) * in_3 + w: what
 *   torch's return_indices gives.  Ties: the first maximum in row-major window order (a later element replaces the held one only if
 *   it compares greater).  A NaN in the window makes y NaN and idx the offset of the first NaN met; a window of nothing but -inf gives
 *   -inf and the first in-range offset.  idx may be NULL in the forward.
 *   bwd:  dx[n][c][idx[n][c][o]] += g[n][c][o] for every o.  Windows overlap whenever s < k: several outputs can route to one element.
 * Average pooling.  y = (sum over the in-range positions, row-major, f32) / divisor; divisor = prod k_i with count_include_pad != 0
 *   (torch's default), the number of in-range positions otherwise.
 *   bwd:  dx[i] += sum over the windows o that contain i of g[o] / divisor(o).
 * Global average pooling is avg_pool with k_i = s_i = in_i and p_i = 0 (the plane class below).
 * No atomics: both backward passes are gathers - a thread owns input elements and walks the covering outputs (at most
 * prod ceil(k_i / s_i)) in ascending row-major order of o, adding g[o] where idx[o] is its own offset (max) or g[o] / divisor(o)
 * (average).  The order of every sum is a function of the geometry and the pointers' 16-byte alignment alone: every output repeats bit
 * for bit.  Nothing here synchronises, allocates or uses the workspace, and no block waits on another: every call can be captured
 * into a graph.  A non-finite value stays inside the windows that hold it.
 * Kernel classes, chosen inside each call:
 *   plane     every out_i == 1 with k_i == in_i and p_i == 0: 16 / 64 / 256 lanes own one contiguous plane of L = prod in_i floats
 *             (L <= 128 / <= 16384 / larger), each lane summing (or scanning) every G-th element or 16-byte group (L % 4 == 0, x
 *             16-byte aligned) in ascending order, the lanes' results merged by a butterfly; max pooling carries (value, offset)
 *             pairs.  Backward: 16-byte stores when L % 4 == 0 and dx is 16-byte aligned, the generic kernel otherwise.
 *   windowed  nd <= 2 (or in_1 == 1 of 3) with (k, s, p) of the innermost axis one of 2/2/0, 3/2/0, 3/2/1, 3/1/0, 3/1/1, any window on
 *             the other axis, in_W % 4 == 0 and x (forward) / dx (backward) 16-byte aligned: a lane makes four adjacent outputs from
 *             16-byte loads (y and idx leave as 16-byte stores when out_W % 4 == 0 and they are aligned), or owns 16 bytes of dx.
 *             Sums in the same order as the generic class.
 *   generic   everything else (nd = 3, other windows, ragged widths, unaligned pointers): scalar kernels.
 * The `_assign` twins write what their `+=` twin would leave in an all-zero dx, without reading it. */
int nk_pool_out_shape(int nd, const int* x_shape, const int* kernel, const int* stride, const int* padding, int* y_shape);
int nk_max_pool_fwd(nk_device* dev, int nd, const float* x, const int* x_shape, float* y, int* idx, const int* kernel,
                    const int* stride, const int* padding);
int nk_max_pool_bwd(nk_device* dev, int nd, float* dx, const int* x_shape, const float* g, const int* idx, const int* kernel,
                    const int* stride, const int* padding);
int nk_max_pool_bwd_assign(nk_device* dev, int nd, float* dx, const int* x_shape, const float* g, const int* idx,
                           const int* kernel, const int* stride, const int* padding);
int nk_avg_pool_fwd(nk_device* dev, int nd, const float* x, const int* x_shape, float* y, const int* kernel, const int* stride,
                    const int* padding, int count_include_pad);
int nk_avg_pool_bwd(nk_device* dev, int nd, float* dx, const int* x_shape, const float* g, const int* kernel, const int* stride,
                    const int* padding, int count_include_pad);
int nk_avg_pool_bwd_assign(nk_device* dev, int nd, float* dx, const int* x_shape, const float* g, const int* kernel,
                           const int* stride, const int* padding, int count_include_pad);

/* ------------------------------------------------------------------ upsampling */
/* Resampling of a contiguous f32 tensor x of shape (N, C, in_1 .. in_nd), nd = 1, 2, 3, to y of shape (N, C, out_1 .. out_nd).  The
 * reference has no such layer; the semantics are fixed here and they are torch's nn.Upsample / F.interpolate called with `size=`
 * (or with recompute_scale_factor=True): per axis, in_i and out_i are all the index arithmetic sees.  x_shape has 2 + nd entries,
 * out_size nd entries.  nk_upsample_out_size is the host arithmetic from a scale: out_i = floor(in_i * scale_i) in f64 (scale: nd
 * entries; no device is needed).  NK_ERR_INVALID, with nothing launched and nothing written: nd outside 1..3, an unknown mode,
 * align_corners != 0 with the nearest mode, a negative N or C, in_i < 1, out_i < 1, a scale that is not finite or not positive, or a
 * plane (prod in_i or prod out_i) that does not fit in 31 bits.  Element offsets are 64-bit.  N * C == 0 returns NK_OK and writes
 * nothing, the _assign twin included.
 * Nearest, in integers:  src(o) = min((o * in) / out, in - 1)  (64-bit integer division) per axis; y is a copy of the selected
 *   element's bits (a NaN, an infinity and -0.0 included).  torch forms the index through a rounded f32 scale and gives another
 *   index for some pairs: 83 of the (in, out) with in <= 64 and out <= 129, (2, 82) and (14, 46) among them, none of them an integer
 *   factor below 41.  The integer form is the definition.
 * Linear (bilinear over two axes, trilinear over three), per axis, all in f32, every operation rounded on its own (no FMA):
 *   align_corners == 0:  s = (float)in / (float)out;                                  src = max(s * (o + 0.5f) - 0.5f, 0)
 *   align_corners != 0:  s = out == 1 ? 0 : (float)(in - 1) / (float)(out - 1);       src = s * o
 *   i0 = min((int)floorf(src), in - 1);  i1 = min(i0 + 1, in - 1);  l1 = src - (float)i0;  l0 = 1 - l1
 *   An output is l0 * a + l1 * b - two products and one sum - applied along the innermost axis first, then outward:
 *   top = l0w * x00 + l1w * x01, bot = l0w * x10 + l1w * x11, y = l0h * top + l1h * bot, and the depth pair after that.  An axis
 *   that is not there (nd < 3) contributes no operation.  A non-finite input propagates as these operations propagate it.
 *   Downsampling is not antialiased (torch's default).
 * bwd:  dx[i] += total(i), one add.  total(i) is the f32 sum, from 0, of w * g[o] over the outputs o of the element's own (n, c)
 *   plane in ascending row-major order and, within an output, over its 2^nd corners in row-major corner order, counting the corners
 *   that land on i (a clamped edge with i0 == i1 gives both).  The weight of a corner is built innermost first: w = l_w; w = l_h * w;
 *   w = l_d * w.  Nearest has one corner of weight 1 and multiplies nothing.  Input elements that no output reads get 0 (or += 0).
 *   The forward and the backward take (i0, i1, l0, l1) from one device function, so their weights agree to the bit.
 * No atomics: the backward is a gather - a thread owns input elements and walks, per axis, a range of candidate outputs that surely
 * holds every reader (nearest: the exact range ceil(i * out / in) .. ceil((i + 1) * out / in) - 1).  The order of every sum is a
 * function of the geometry alone: every result repeats bit for bit, whatever the class.  Nothing here synchronises, allocates or
 * uses the workspace, and no block waits on another: every call can be captured into a graph.
 * Kernel classes, chosen inside each call from (mode, in, out) and the pointers' 16-byte alignment; all give the same bits:
 *   nearest x2  nearest with out_W == 2 in_W, in_W % 4 == 0 and both pointers 16-byte aligned, any ratio on the outer axes: a lane
 *               loads 16 bytes of x and stores two 16-byte groups per output row it feeds; backward, a lane owns 16 bytes of dx and
 *               reads g in 16-byte loads.
 *   vector      forward: out_W % 4 == 0 and y aligned - a lane makes four adjacent outputs and stores 16 bytes; backward:
 *               in_W % 4 == 0 and dx aligned - a lane owns 16 bytes of dx.
 *   generic     scalar, any shape, any alignment.
 * The `_assign` twin writes what `+=` would leave in an all-zero dx, without reading it. */
enum { NK_UPSAMPLE_NEAREST = 0, NK_UPSAMPLE_LINEAR = 1 };
int nk_upsample_out_size(int nd, const int* x_shape, const double* scale, int* out_size);
int nk_upsample_fwd(nk_device* dev, int nd, int mode, int align_corners, const float* x, const int* x_shape, float* y,
                    const int* out_size);
int nk_upsample_bwd(nk_device* dev, int nd, int mode, int align_corners, float* dx, const int* x_shape, const float* g,
                    const int* out_size);
int nk_upsample_bwd_assign(nk_device* dev, int nd, int mode, int align_corners, float* dx, const int* x_shape, const float* g,
                           const int* out_size);

/* ------------------------------------------------------------------ fused attention core ---
 * The composed multi-head attention's per-(sample, head) chain in one kernel per direction (SURVEY.md 8a note; the
 * composition is MatrixMatrixMulT node/matrix_matrix_mul_t/mod.rs:31-41, Multiplication node/multiplication/mod.rs:39-50,
 * Softmax node/softmax/mod.rs:37-53, Dropout node/dropout/mod.rs:53-79, MatrixMatrixMul node/matrix_matrix_mul/mod.rs:31-41):
 *   S_bh = Q_bh.K_bh^T ; P = softmax(S*scale, axis 1) ; Pd = dropout(P) ; O_bh = Pd.V_bh
 * Q, K, V, O, dO, dQ are the (B*S) x (H*dh) projection layout (head h = columns h*dh .. h*dh+dh-1, sample b = rows
 * b*S ..); scores / dS / dropped are (B*H, SP, SP) with SP = S rounded up to a multiple of 32 (row stride SP; the entries of
 * rows / columns >= S are scratch: padded keys hold a score of -inf and dS = Pd = 0); stats is (B*H, SP, 2) =
 * (m2, 1 / sum_k exp2(S*c1 - m2)) per row with
 * c1 = scale*log2(e) and the shift m2 in [max_k S*c1 - 6, max_k S*c1]: P = exp2(S*c1 - m2) * stats[..,1].  scale > 0.
 * The score tile stays on chip between the two products (online softmax forward, recomputed probabilities backward).
 * Dropout mask: score (bh, r, k) takes draw (bh*SP + r)*SP + k of the layout documented at nk_dropout_fwd - for S % 32 == 0 the
 * Philox stream of nk_scale_softmax_dropout_fwd on the (B*H, S, S) tensor (same seed / offset -> same mask); one forward
 * consumes ceil(B*H*SP*SP / 8) calls.
 * nk_attention_supported: dh in {32, 64, 128}, S >= 1, not (train and p == 1) - the answer holds for the causal entry points
 * below as well; callers fall back to the node-by-node path. */
int nk_attention_supported(int S, int dh, double p, int train);
/* forward: writes the raw scores (for the backward pass), the row statistics, the dropout draws (1 bit per score:
 * B*H*SP*SP/32 words laid out [b*H + h][SP/32 query tiles][SP/32 key tiles][32 queries of the tile], bit 16 j + e of a word =
 * key 32 kt + 16 j + e kept - opaque to callers, who only hand the buffer from the forward to the backward; may be NULL
 * when dropout is inactive) and O.  `scores` = `stats` = NULL: inference, nothing is
 * kept for a backward pass (O only: no (B*H, SP, SP) tensor exists at all). */
int nk_attention_fwd(nk_device* dev, const float* Q, const float* K, const float* V, float* scores, float* stats,
                     uint32_t* mask_bits, float* O, int B, int S, int H, int dh, float scale, double p, int train,
                     uint64_t seed, uint64_t offset);
/* backward: dQ_bh (+)= dS_bh.K_bh, dK_bh (+)= dS_bh^T.Q_bh, dV_bh (+)= Pd_bh^T.dO_bh (`assign_*` != 0: first write).  dS and
 * Pd ((B*H, SP, SP) each) are scratch the caller owns; they are WRITTEN by the fused kernel and read by the two batched
 * products this call issues after it.  The mask is the forward's (`mask_bits`), as the reference's backward node reads the
 * forward's noise buffer.  DropoutBackward multiplies by the 0/1 mask only (node/dropout/mod.rs:113-128), SoftmaxBackward
 * node/softmax/mod.rs:84-104, MatrixMatrixMul(T)Backward node/matrix_matrix_mul{,_t}/mod.rs:63-105. */
int nk_attention_bwd(nk_device* dev, float* dQ, float* dK, float* dV, float* dS, float* dropped, const float* dO,
                     const float* O, const float* scores, const float* stats, const uint32_t* mask_bits, const float* Q,
                     const float* K, const float* V, int B, int S, int H, int dh, float scale, double p, int train,
                     int assign_dq, int assign_dk, int assign_dv);
/* The same two entry points for Q, K, V (and dQ, dK, dV) that are the three column blocks of ONE (B*S, 3*H*dh) matrix - the
 * output of a single Linear over the row-stacked projection weights [Wq; Wk; Wv] (`nn::MultiheadAttention`'s packed
 * projections: one GEMM with N = 3*H*dh forward, one with K = 3*H*dh for the input gradient, instead of three each).  Row
 * stride 3*H*dh, column offsets 0, H*dh, 2*H*dh; everything else as above.  `assign`: dQKV is a fresh gradient. */
int nk_attention_qkv_fwd(nk_device* dev, const float* QKV, float* scores, float* stats, uint32_t* mask_bits, float* O, int B, int S,
                         int H, int dh, float scale, double p, int train, uint64_t seed, uint64_t offset);
int nk_attention_qkv_bwd(nk_device* dev, float* dQKV, float* dS, float* dropped, const float* dO, const float* O, const float* scores,
                         const float* stats, const uint32_t* mask_bits, const float* QKV, int B, int S, int H, int dh, float scale,
                         double p, int train, int assign);
/* Causal self-attention: query row r of a sample attends to the key rows k <= r of that sample.  As a composition it is the chain
 * above with one Addition node (node/addition/mod.rs:39-50; AdditionBackward: the gradient passes through) in front of the Softmax:
 *   P = dropout(softmax(Q_bh.K_bh^T * scale + M, axis 1)),  M (S, S) constant, M[r][k] = 0 for k <= r and -inf for k > r
 * (Softmax of a lane with -inf entries is exactly 0 there, node/softmax/mod.rs:37-53; every row keeps its diagonal).  Same parameter
 * lists, layouts, row statistics ((m2, 1 / sum) over the unmasked keys) and draw layout as the four entry points above: score
 * (bh, r, k) takes draw (bh*SP + r)*SP + k whether masked or not and one forward consumes ceil(B*H*SP*SP / 8) calls, so a masked
 * position's draw is simply unused and the mask agrees with the non-causal kernels' and nk_dropout_fwd's on every position.
 * What differs is the scratch contract.  The kernels walk the key tiles on and below the diagonal only (a block of 128 queries
 * 128 qb .. visits keys < 128 qb + 128): `scores`, `dS`, `dropped` and `mask_bits` keep their (B*H, SP, SP) allocation and layout, but
 * the 32 x 32 tiles strictly above the diagonal are NOT WRITTEN AND NOT READ - they hold whatever the buffer held.  In a visited
 * tile a masked position's score is -inf.  The backward writes zeros to dS and Pd above the diagonal INSIDE every 128 x 128 diagonal
 * block, so both are defined (and exactly 0 at masked positions) on every 128 x 128 block that touches or lies below the diagonal and
 * undefined strictly above; dK_bh (+)= dS_bh^T.Q_bh and dV_bh (+)= Pd_bh^T.dO_bh reduce, per strip of 128 keys, over the queries from
 * the strip's first row on and never read an undefined block. */
int nk_attention_causal_fwd(nk_device* dev, const float* Q, const float* K, const float* V, float* scores, float* stats,
                            uint32_t* mask_bits, float* O, int B, int S, int H, int dh, float scale, double p, int train,
                            uint64_t seed, uint64_t offset);
int nk_attention_causal_bwd(nk_device* dev, float* dQ, float* dK, float* dV, float* dS, float* dropped, const float* dO,
                            const float* O, const float* scores, const float* stats, const uint32_t* mask_bits, const float* Q,
                            const float* K, const float* V, int B, int S, int H, int dh, float scale, double p, int train,
                            int assign_dq, int assign_dk, int assign_dv);
int nk_attention_qkv_causal_fwd(nk_device* dev, const float* QKV, float* scores, float* stats, uint32_t* mask_bits, float* O, int B,
                                int S, int H, int dh, float scale, double p, int train, uint64_t seed, uint64_t offset);
int nk_attention_qkv_causal_bwd(nk_device* dev, float* dQKV, float* dS, float* dropped, const float* dO, const float* O,
                                const float* scores, const float* stats, const uint32_t* mask_bits, const float* QKV, int B, int S, int H,
                                int dh, float scale, double p, int train, int assign);
/* Sliding-window (banded causal) self-attention: query row r attends to the key rows max(0, r - window + 1) .. r.  As a composition
 * it is the causal chain above with the BANDED constant M[r][k] = 0 for r - window < k <= r and -inf elsewhere; every row keeps its
 * diagonal.  The causal entry points' parameter lists plus `window`, the same projection layouts, row statistics ((B*H, SP, 2), over
 * the unmasked keys) and draw positions: score (bh, r, k) takes draw (bh*SP + r)*SP + k of the PADDED (B*H, SP, SP) index space and one
 * forward consumes ceil(B*H*SP*SP / 8) calls, so the mask agrees with nk_dropout_fwd's and the composed path's position for position.
 * Work and scratch are O(S * window).  With k_lo(qb) = max(0, 128 qb - window + 1) and js(qb) = k_lo(qb) / 128, the block of queries
 * 128 qb .. stages the key tiles 4 js(qb) .. min(SP / 32, 4 qb + 4) - 1 only, and its wave of rows r0 = 128 qb + 32 w .. computes the
 * tiles max(0, r0 - window + 1) / 32 .. 4 qb + w of them.
 * Banded scratch: `scores`, `dS` and `dropped` hold, per (sample, head), nk_attention_band_scratch(S, window) = (SP - 1) * ld + SP
 * floats; element (r, k) is at bh * that + r * ld + k with ld = nk_attention_band_ld(S, window) = min(SP, 128 * (ceil((window - 1) /
 * 128) + 1)) - the (SP, SP) matrix with a row stride shorter than its width.  A row's touched columns start at 128 js(r / 128), which
 * never decreases with r, and span at most ld, so no two touched elements share an address.  `mask_bits` holds, per (sample, head),
 * nk_attention_band_mask_words(S, window) = SP * ld / 32 words laid out [SP/32 query tiles][ld/32 key tiles, counted from tile
 * 4 js(qb) of the query tile's block][32 queries], bits as in nk_attention_fwd.  window >= S: ld = SP and the causal layouts.
 * Scratch contract: scores are written on the computed tiles, -inf at masked positions (padded keys included); the backward defines
 * dS and Pd - exactly 0 at masked positions - on every 128 x 128 block (qb, j) with js(qb) <= j <= qb.  Nothing else is written or
 * read: the buffers need no initialisation.  dK_bh (+)= dS_bh^T.Q_bh and dV_bh (+)= Pd_bh^T.dO_bh run per strip of 128 keys over the
 * queries of the blocks that staged the strip.  For window >= S every output and every scratch element on the triangle has the bits
 * of the causal entry points.
 * NK_ERR_INVALID, nothing written: window <= 0; `scores` or `stats` NULL (there is no inference form: the forward keeps its state);
 * everything the causal entry points refuse, the 2^31 limit on the mask words taken on the banded extent.  The training-mode
 * forward with dropout active refuses stream capture (the Philox offset would be frozen); the evaluation forward can be captured.
 * The three geometry functions need no device and return 0 for S <= 0 or window <= 0. */
int nk_attention_band_ld(int S, int window);
size_t nk_attention_band_scratch(int S, int window);
size_t nk_attention_band_mask_words(int S, int window);
int nk_attention_band_fwd(nk_device* dev, const float* Q, const float* K, const float* V, float* scores, float* stats,
                          uint32_t* mask_bits, float* O, int B, int S, int H, int dh, float scale, double p, int train,
                          uint64_t seed, uint64_t offset, int window);
int nk_attention_band_bwd(nk_device* dev, float* dQ, float* dK, float* dV, float* dS, float* dropped, const float* dO,
                          const float* O, const float* scores, const float* stats, const uint32_t* mask_bits, const float* Q,
                          const float* K, const float* V, int B, int S, int H, int dh, float scale, double p, int train,
                          int assign_dq, int assign_dk, int assign_dv, int window);
int nk_attention_qkv_band_fwd(nk_device* dev, const float* QKV, float* scores, float* stats, uint32_t* mask_bits, float* O, int B,
                              int S, int H, int dh, float scale, double p, int train, uint64_t seed, uint64_t offset, int window);
int nk_attention_qkv_band_bwd(nk_device* dev, float* dQKV, float* dS, float* dropped, const float* dO, const float* O,
                              const float* scores, const float* stats, const uint32_t* mask_bits, const float* QKV, int B, int S, int H,
                              int dh, float scale, double p, int train, int assign, int window);
/* Packed sequences (document-masked causal self-attention): query row r of sample b attends to the key rows lo_eff[r] .. r with
 *   lo_eff[r] = min(r, max(lo[b][r], r - span + 1, 0)),
 * `lo` a device array of (B, S) int32 shared by the heads of a sample - for packed documents, the start of the row's document - and
 * `span` the longest run lo_eff .. r any row may keep (the longest document, or min(that, window) under a sliding window).  As a
 * composition it is the causal chain above with the per-sample constant M_b[r][k] = 0 for lo_eff[r] <= k <= r and -inf elsewhere.
 * The clamp is the memory-safety guarantee: no content of `lo` makes the call read or write outside what the band geometry for
 * (S, span) defines.  PRECONDITION: lo_eff never decreases with r inside a sample; with an array that breaks it the call stays
 * memory-safe and its results are unspecified.  A padded query (r >= S inside the last tile of 32) uses the clamped row S - 1.
 * Geometry: there are no functions of its own.  `scores`, `dS` and `dropped` hold nk_attention_band_scratch(S, span) floats per
 * (sample, head), element (r, k) at r * nk_attention_band_ld(S, span) + k; `mask_bits` holds nk_attention_band_mask_words(S, span)
 * words per (sample, head) in the band's layout; statistics (B*H, SP, 2); draws at (bh*SP + r)*SP + k.  The walk is the band's with
 * window := span for what a block stages, and per wave of 32 rows r0 .. the tiles lo_eff[r0] / 32 .. r0 / 32 are computed.  Scratch
 * contract, the band's: scores are written on the computed tiles, -inf at masked positions; the backward defines dS and Pd - exactly
 * 0 at masked positions - on every 128 x 128 block (qb, j) with js(qb) <= j <= qb; nothing else is written or read.  dK / dV run
 * per strip of 128 keys as the band's with window := span.  No entry point reads `lo` on the host or allocates.
 * Bit contracts:
 *  1. lo[b][r] = max(0, r - span + 1) for all b, r - or any array the clamp turns into that, such as every entry -7 - gives every
 *     buffer the bits nk_attention_band_* gives with window = span; with span >= S those are the causal entry points' layouts and bits.
 *  2. With documents (lo[b][r] = the start of r's document), a row's bits in O and dQ depend on its own document's queries, keys and
 *     values only - on the keys / values of lo_eff[r] .. r and, through the forward's lazy softmax shift, which the 32 rows of a tile
 *     move together, on the scores of its own document's rows; the same holds for the rows of its document in dK / dV.  They do not
 *     depend on the finite contents of other documents: masked products are exact zeros, adding them changes no bit, and a row of
 *     a later document asks for the shift only in the tile's diagonal tile, where it asks whatever it holds.
 * NK_ERR_INVALID, nothing written: lo == NULL, span <= 0, and everything nk_attention_band_* refuses with window = span. */
int nk_attention_seg_fwd(nk_device* dev, const float* Q, const float* K, const float* V, const int* lo, float* scores, float* stats,
                         uint32_t* mask_bits, float* O, int B, int S, int H, int dh, int span, float scale, double p, int train,
                         uint64_t seed, uint64_t offset);
int nk_attention_seg_bwd(nk_device* dev, float* dQ, float* dK, float* dV, float* dS, float* dropped, const float* dO,
                         const float* O, const float* scores, const float* stats, const uint32_t* mask_bits, const float* Q,
                         const float* K, const float* V, const int* lo, int B, int S, int H, int dh, int span, float scale, double p,
                         int train, int assign_dq, int assign_dk, int assign_dv);
int nk_attention_qkv_seg_fwd(nk_device* dev, const float* QKV, const int* lo, float* scores, float* stats, uint32_t* mask_bits,
                             float* O, int B, int S, int H, int dh, int span, float scale, double p, int train, uint64_t seed,
                             uint64_t offset);
int nk_attention_qkv_seg_bwd(nk_device* dev, float* dQKV, float* dS, float* dropped, const float* dO, const float* O,
                             const float* scores, const float* stats, const uint32_t* mask_bits, const float* QKV, const int* lo, int B,
                             int S, int H, int dh, int span, float scale, double p, int train, int assign);
/* ------------------------------------------------------------------ incremental decoding --
 * The causal forward above, one slice of T positions at a time, in inference (no dropout, nothing kept for a backward pass): each
 * layer's keys and values stay on the device and the new rows attend to them.  For sample b, head h and the t-th new row
 * (0 <= t < T), with n = start[b] + t + 1:
 *   o = softmax(q . K_bh[0:n]^T * scale) . V_bh[0:n]
 * where keys start[b] .. start[b] + T - 1 are the rows appended in the same step.  As a composition this is row start[b] + t of the
 * chain documented at nk_attention_causal_fwd (MatrixMatrixMulT node/matrix_matrix_mul_t/mod.rs:31-41, Multiplication
 * node/multiplication/mod.rs:39-50, Addition node/addition/mod.rs:39-50 with the causal constant, Softmax node/softmax/mod.rs:37-53,
 * MatrixMatrixMul node/matrix_matrix_mul/mod.rs:31-41) over the sample's first n positions, dropout inactive.
 * Cache layout: Kc, Vc are (B, H, cap, dh) f32, head-major - the keys of one (b, h) are one contiguous stream; cap = capacity in
 * positions.  `start`: a DEVICE array of B int32, each sample's length before this step (per sample: ragged batches).
 * nk_kv_cache_append: row b*T + t of K / V (row stride ld floats) goes to position start[b] + t of every head of sample b, head h
 *   taking columns h*dh .. h*dh + dh - 1 of the row.  K = QKV + d, V = QKV + 2d, ld = 3d addresses a packed projection output
 *   (d = H*dh); ld = d separate projections.  A grouped-query layer's (B, Hkv, cap, dh) caches take the same call with H = Hkv,
 *   K = QKV + d, V = QKV + d + dkv, ld = d + 2*dkv (d = heads*dh, dkv = Hkv*dh; see grouped-query attention below).  A bit-exact copy.  A row whose position would be >= cap (or < 0) is NOT written -
 *   never out of bounds; nothing else of the cache is touched.
 * nk_attention_decode_fwd: Q row b*T + t has stride ldq; O is (B*T, H*dh).  Query (b, t) reads keys < min(start[b] + t + 1, cap)
 *   (none, for a negative start: the output row is 0).  Split-KV: a problem (b, h, t) is cut into chunks of
 *   nk_attention_decode_chunk(dh) keys - a compile-time constant per head size (dh in {32, 64, 128}: 16-byte loads; any other dh:
 *   a scalar kernel), never derived from the CU count, B, H, T, cap or nk_dev_tune.  A partial leaves (m, l, unnormalised o[dh])
 *   in `workspace`, a second launch merges a problem's partials in chunk order in the exp2 form of the fused core.  No atomics, no
 *   reductions in arrival order: the bits of o for (b, h, t) depend on that problem's q, its n keys / values and scale ONLY - not
 *   on the other samples, B, H, T, cap, the run, or on what the cache holds at positions >= n, which is never read into the
 *   result (uninitialised memory in real use; NaN there is harmless).
 *   `workspace`: caller-owned scratch of nk_attention_decode_workspace(B, T, H, dh, cap) floats; the library allocates nothing in
 *   this call, so it can sit in a captured region.
 * NK_ERR_INVALID: non-positive B / T / H / dh / cap, scale <= 0 (or not finite), a null pointer, a row stride below H*dh, caches
 * not 16-byte aligned for dh in {32, 64, 128}, more than 65535 chunks in cap, B*T*H >= 2^24 (one block per problem and chunk). */
int nk_kv_cache_append(nk_device* dev, float* Kc, float* Vc, const float* K, const float* V, int ld, const int* start, int B, int T,
                       int H, int dh, int cap);
int nk_attention_decode_fwd(nk_device* dev, const float* Q, int ldq, const float* Kc, const float* Vc, const int* start, float* O,
                            float* workspace, int B, int T, int H, int dh, int cap, float scale);
size_t nk_attention_decode_workspace(int B, int T, int H, int dh, int cap);
int nk_attention_decode_chunk(int dh);
/* ------------------------------------------------------------------ grouped-query attention --
 * Ours (the reference has one head count): GQA, Ainslie et al. 2023, as LLaMA-2-70B / 3, Mistral and Qwen use it; multi-query
 * (Shazeer 2019) is Hkv = 1.  H query heads, Hkv key / value heads, H % Hkv == 0, G = H / Hkv: query head h attends to kv head
 * h / G.  d = H*dh, dkv = Hkv*dh; a packed projection output is (rows, d + 2*dkv) = [Q | K | V].
 * The cache of a grouped layer is (B, Hkv, cap, dh) - G times less memory and decode traffic.  nk_kv_cache_append serves it as it
 * is: call it with H = Hkv, K = QKV + d, V = QKV + d + dkv, ld = d + 2*dkv.
 * nk_attention_decode_gqa_fwd: Kc, Vc are (B, Hkv, cap, dh); Q (row stride ldq, head h at columns h*dh ..), O (B*T, H*dh), start,
 *   scale and `workspace` (nk_attention_decode_workspace(B, T, H, dh, cap) floats, the per-(b, t, h) layout) are those of
 *   nk_attention_decode_fwd.  Query head h of row b*T + t reads the n = min(start[b] + t + 1, cap) first keys of kv head h / G.
 *   dh in {32, 64, 128}: one block per ((b, t, kv head), batch of at most 8 query heads of the group, chunk of
 *   nk_attention_decode_chunk(dh) keys) loads its chunk of K and V ONCE into registers and runs nk_attention_decode_fwd's per-head
 *   arithmetic for each of its heads; a group of more than 8 heads takes ceil(G / 8) blocks.  Any other dh: a scalar kernel without
 *   sharing.  The merge of the partials is nk_attention_decode_fwd's.  No atomics.
 *   Bit contract: the bits of o for (b, h, t) are those nk_attention_decode_fwd gives for the same query on a cache whose head h
 *   holds kv head h / G's rows - same chunking, same order - so they depend on that problem's q, its n keys / values and scale
 *   ONLY: not on G, on the heads that share the block, on B, T, cap or the cache's tail.  Hkv == H forwards to
 *   nk_attention_decode_fwd: the same launches.
 *   NK_ERR_INVALID, nothing written: Hkv <= 0, Hkv > H, H % Hkv != 0, and everything nk_attention_decode_fwd refuses.
 * nk_repeat_kv_*: the training / prefill side.  The fused core keeps running on H heads: kv head k is written G times in front of
 *   it and the gradients of the copies are summed behind it.  x / dx are `rows` rows of Hkv*dh floats (row stride ldx / lddx),
 *   y / g `rows` rows of Hkv*G*dh floats (row stride ldy / ldg).
 *   fwd:        y[r, (k*G + j)*dh + e] = x[r, k*dh + e], 0 <= j < G: a bit-exact copy.
 *   bwd:        dx[r, k*dh + e] += s, s = ((g_0 + g_1) + g_2) + ... with g_j = g[r, (k*G + j)*dh + e], j ascending, in f32;
 *   bwd_assign: dx[r, k*dh + e] = s.  The bits are fixed by that order (G = 1: an add / a copy).
 *   16-byte accesses when dh % 4 == 0 and both strides and pointers allow it, scalar otherwise; row offsets are 64-bit.  Columns
 *   outside [0, Hkv*dh) of x / dx and [0, Hkv*G*dh) of y / g are never touched: the operands may be column blocks of packed
 *   buffers.  The operands must not overlap.  No atomics, no LDS.
 *   NK_ERR_INVALID: non-positive rows / Hkv / G / dh, a null pointer, a row stride below the operand's width, Hkv*G*dh >= 2^31. */
int nk_attention_decode_gqa_fwd(nk_device* dev, const float* Q, int ldq, const float* Kc, const float* Vc, const int* start, float* O,
                                float* workspace, int B, int T, int H, int Hkv, int dh, int cap, float scale);
int nk_repeat_kv_fwd(nk_device* dev, const float* x, int ldx, float* y, int ldy, int rows, int Hkv, int G, int dh);
int nk_repeat_kv_bwd(nk_device* dev, float* dx, int lddx, const float* g, int ldg, int rows, int Hkv, int G, int dh);
int nk_repeat_kv_bwd_assign(nk_device* dev, float* dx, int lddx, const float* g, int ldg, int rows, int Hkv, int G, int dh);
/* ------------------------------------------------------------------ sliding-window decoding --
 * Ours (the reference has no attention layer): the sliding window of Longformer (Beltagy et al. 2020) as Mistral 7B uses it.  Query
 * position i attends to the keys max(0, i - W + 1) .. i, so a decoding step reads at most W keys per kv head whatever the length of
 * the generation, and a cache of W + T - 1 slots serves any length.  For sample b, query head h and the t-th new row (0 <= t < T),
 * with n = start[b] + t + 1 and lo = max(0, n - W):
 *   o = softmax(q . K[lo:n]^T * scale) . V[lo:n]
 * over the rows of kv head h / (H / Hkv).  As a composition this is row n - 1 of the causal chain documented at
 * nk_attention_causal_fwd with the BANDED constant M[r][k] = 0 for r - W < k <= r and -inf elsewhere; every row keeps its diagonal,
 * so no row is empty for any W >= 1.
 * nk_attention_decode_window_fwd: Kc, Vc are (B, Hkv, cap, dh); Hkv == H is the ungrouped layer, otherwise query head h reads kv
 *   head h / (H / Hkv) exactly as nk_attention_decode_gqa_fwd does.  Q, ldq, O, start and scale are nk_attention_decode_fwd's.
 *   ring == 0: a linear cache, position p at slot p, n clipped to cap as in nk_attention_decode_fwd.
 *   ring != 0: a rolling cache, position p at slot p % cap, n NOT clipped; requires window + T - 1 <= cap.  Why: the T rows of a
 *   step are appended before they are attended to, so positions start .. start + T - 1 are written while row 0 (n = start + 1)
 *   still reads position start + 1 - W.  The write of position start + T - 1 lands on that slot iff
 *   (start + T - 1) - (start + 1 - W) = W + T - 2 is a multiple of cap; all T writes and the W - 1 older keys row 0 reads are
 *   W + T - 1 consecutive positions, distinct slots iff W + T - 1 <= cap.  Positions must stay below 2^31 - 1024.
 *   A negative start[b] gives a zero output row.
 *   Chunking: chunks stay aligned to ABSOLUTE positions - chunk c covers positions [cC, cC + C), C = nk_attention_decode_chunk(dh) -
 *   and a problem visits chunks lo / C .. (n - 1) / C only: at most (W + C - 2) / C + 1 of them (integer division), which is the
 *   grid's second extent and the workspace's per-problem stride, never a function of cap.  Positions of a visited chunk outside
 *   [lo, n): the load is redirected to position n - 1 (always inside the window), the probability is SELECTED to 0, and the chunk's
 *   shift is the exact maximum over its in-window keys; a slot outside the window is never read into a result.  Partials are merged
 *   in ascending chunk order in nk_attention_decode_fwd's exp2 form; a window inside one chunk writes O directly.  No atomics.  The
 *   slot of a position is the slot of lo (one remainder per block) plus an offset with one conditional subtract: no table and
 *   no dependent load.  The per-head arithmetic is nk_attention_decode_fwd's; a grouped layer loads a chunk once for up to 8 query heads.
 *   Bit contract:
 *   (1) n <= window: the bits are those of nk_attention_decode_gqa_fwd on the same inputs (nk_attention_decode_fwd when Hkv == H).
 *   (2) for the same positions' contents, the bits of a ring cache equal the bits of a linear cache.
 *   (3) the bits of o for (b, h, t) depend on that problem's q, its keys / values at positions [lo, n), n, W and scale ONLY: not on
 *       B, T, cap, ring, the group size, the other samples, or anything a slot outside the window holds (NaN or 1e30 is harmless).
 *   (4) grouped bits equal ungrouped bits on the cache with every kv head repeated.
 *   `workspace`: nk_attention_decode_window_workspace(B, T, H, dh, window) floats (needs no device; a function of the window,
 *   never of cap; on a linear cache a window above cap acts as the window cap - the same keys - and uses less of it).
 *   NK_ERR_INVALID, nothing written: window <= 0, ring with window + T - 1 > cap, and everything nk_attention_decode_gqa_fwd refuses.
 * nk_kv_cache_append_ring: nk_kv_cache_append with row b*T + t going to slot (start[b] + t) % cap.  Every row with a non-negative
 *   position is written; T > cap (two rows of a sample on one slot) is NK_ERR_INVALID.  A bit-exact copy; nothing else of the cache
 *   is touched. */
int nk_attention_decode_window_fwd(nk_device* dev, const float* Q, int ldq, const float* Kc, const float* Vc, const int* start, float* O,
                                   float* workspace, int B, int T, int H, int Hkv, int dh, int cap, int window, int ring, float scale);
size_t nk_attention_decode_window_workspace(int B, int T, int H, int dh, int window);
int nk_kv_cache_append_ring(nk_device* dev, float* Kc, float* Vc, const float* K, const float* V, int ld, const int* start, int B, int T,
                            int H, int dh, int cap);
/* ------------------------------------------------------------------ paged decoding --
 * Ours: the block table of vLLM's PagedAttention (Kwon et al. 2023) under the decode kernels above.  The keys and values of every
 * sequence live in fixed-size pages of two pools instead of one (B, Hkv, cap, dh) slab per batch, so memory is the sum of the lengths
 * held, a sequence can join or leave a running batch, and sequences with a common prefix can name the same pages.
 * Layout: Kp, Vp are (num_pages, Hkv, page, dh): one head's slice of a page is contiguous, a lane group still reads runs of
 *   consecutive keys.  `table` is a DEVICE int32 (B, max_pages): position p of sample b lives in page table[b*max_pages + p / page] at
 *   slot p % page.  `page` is a power of two, 16 <= page: every chunk size of the library is a power of two, so a chunk is either
 *   inside one page or made of whole pages.  The virtual capacity cap_v = max_pages * page must stay below 2^31 - 1024, the position
 *   limit of the window kernels.
 * nk_kv_pages_append: row b*T + t of K / V (row stride ld, H = the kv heads) goes to position start[b] + t, K and V in one launch, a
 *   bit-exact copy; 16-byte accesses under nk_kv_cache_append's conditions.  Rows with a negative position or one >= cap_v are
 *   dropped, and so is a row whose table entry is outside [0, num_pages).  Nothing else of the pools is touched.
 * nk_kv_pages_copy: whole pages src[i] -> dst[i], 0 <= i < n (DEVICE int32 arrays), all H heads, K and V, one streaming launch.  A
 *   pair with an id outside [0, num_pages) is dropped; src[i] == dst[i] is a no-op; a page that is the destination of one pair must
 *   not appear in another.  n == 0 is NK_OK without a launch.
 * nk_attention_decode_paged_fwd: for sample b, query head h and the t-th new row, n = min(start[b] + t + 1, cap_v);
 *   window == 0: o = softmax(q . K[0:n]^T * scale) . V[0:n], the rule of nk_attention_decode_gqa_fwd with cap := cap_v;
 *   window  > 0: the keys max(0, n - W) .. n - 1 in chunks aligned to absolute positions, the rule of nk_attention_decode_window_fwd
 *   with ring = 0.  Hkv <= H divides H; the heads of a group share one read of their chunk, 8 per block.  Q, ldq, O, start and
 *   scale are nk_attention_decode_fwd's.
 *   The kernels are the bodies of the contiguous ones with one more switch - where a position lives - and the contiguous forms'
 *   combine kernels, so the summation order is by position, never by page.  Bit contract:
 *   (1) the bits equal those of nk_attention_decode_gqa_fwd (window == 0) or nk_attention_decode_window_fwd with ring = 0 on the
 *       (B, Hkv, cap_v, dh) cache gathered through the table - whatever the page size and whichever physical pages the table names;
 *   (2) the bits of o for (b, h, t) depend on q, the keys / values at the positions it reads, n, W and scale ONLY: not on B, T,
 *       max_pages, num_pages, the other samples, nor on what any other page, slot or table entry holds (NaN or 1e30, -1 or an id past
 *       the pool are harmless);
 *   (3) two samples whose rows name the same pages for a common prefix read the same memory: equal queries give equal bits.
 *   Nothing leaves the pool: positions that do not count are redirected to position n - 1 before the lookup, so table entries past a
 *   sequence's own pages, or below its window, are never read; the entry that is read is clamped into [0, num_pages) with one unsigned
 *   min, which changes nothing for a valid entry.  A wrong table gives wrong numbers, never an access outside the two allocations.
 *   No atomics; the chunk is the compile-time constant nk_attention_decode_chunk(dh); nothing depends on the CU count.
 *   `workspace`: nk_attention_decode_paged_workspace(B, T, H, dh, max_pages, page, window) floats (needs no device): window == 0,
 *   nk_attention_decode_workspace(B, T, H, dh, cap_v); otherwise nk_attention_decode_window_workspace(B, T, H, dh, window).  0 for a
 *   geometry the entry point refuses.
 *   NK_ERR_INVALID, nothing written: everything nk_attention_decode_gqa_fwd refuses with cap := cap_v, in its order and words; page
 *   not a power of two or below 16; max_pages <= 0; num_pages <= 0; cap_v >= 2^31 - 1024; a null table; window < 0; a pool of more
 *   than 2^32 16-byte units (dh 32 / 64 / 128). */
int nk_kv_pages_append(nk_device* dev, float* Kp, float* Vp, const float* K, const float* V, int ld, const int* start, const int* table,
                       int max_pages, int B, int T, int H, int dh, int page, int num_pages);
int nk_kv_pages_copy(nk_device* dev, float* Kp, float* Vp, const int* src, const int* dst, int n, int H, int dh, int page, int num_pages);
size_t nk_attention_decode_paged_workspace(int B, int T, int H, int dh, int max_pages, int page, int window);
int nk_attention_decode_paged_fwd(nk_device* dev, const float* Q, int ldq, const float* Kp, const float* Vp, const int* start,
                                  const int* table, int max_pages, float* O, float* workspace, int B, int T, int H, int Hkv, int dh, int page,
                                  int num_pages, int window, float scale);
/* ------------------------------------------------------------------ rotary position embedding --
 * Ours (the reference has no position encoding of any kind): RoPE, Su et al. 2021 (RoFormer), as LLaMA / Mistral / Qwen / GPT-NeoX /
 * Phi apply it to the query and key rows in front of the attention scores.
 * Geometry: a buffer of B*T rows with row stride ld floats; a row holds NH heads of dh floats from column 0 (NH = 2*heads, ld = 3*d
 * addresses the Q|K blocks of a packed projection output; its V block, like every column >= NH*dh, is never read or written).
 * Row b*T + t sits at position p = (start ? start[b] : 0) + t; `start` is a DEVICE array of B int32 or NULL - the array
 * nk_kv_cache_append takes.  The first `rot` columns of each head are rotated (rot even, 2 <= rot <= dh), columns [rot, dh) pass
 * through.  Pairing: interleaved == 0 half-split pairs (j, j + rot/2) (NeoX / LLaMA-HF), otherwise interleaved pairs (2j, 2j+1)
 * (GPT-J / RoFormer), j < rot/2.  With (c, s) = table[p][j], the arithmetic is fixed to the bit:
 *     y1 = fmaf(x1, c, -(x2 * s));   y2 = fmaf(x2, c, x1 * s)          (backward / inverse: s -> -s)
 * by every kernel family: the bits of an output element depend on its pair, its position and the table only - not on the kernel
 * family (16-byte or scalar accesses), B, T, NH, the strides, in place or not, or on how p splits into start[b] + t.
 * Table: (max_pos, rot/2, 2) f32, (cos, sin) interleaved; entry (p, j) is the f32 rounding of the f64 cos / sin of
 * p * base^(-2j/rot), frequency, product and function all in f64 (an f32 angle is 1e-3 rad off at position 16 384).
 * nk_rope_table fills it on the host and uploads it (one synchronising call at model construction; refuses capture).
 * A position outside [0, max_pos) is clamped into the table by the kernel: no `start` can make it read outside the table.
 * nk_rope_fwd: y = R x.  y == x with ldy == ldx is the in-place form (a thread owns both members of each pair it touches; no other
 *   overlap of x and y is allowed).  Out of place the pass-through columns are copied.
 * nk_rope_bwd: dx += R^T g; nk_rope_bwd_assign: dx = R^T g (dx == g with lddx == ldg legal for the assign form only);
 *   pass-through columns dx (+)= g.  R is orthogonal: the backward keeps nothing of the input.
 * No atomics, no LDS.  Row offsets are 64-bit (rows * ld may exceed 2^31); B*T itself must fit 31 bits.
 * NK_ERR_INVALID, nothing written: rot odd or outside [2, dh], NH*dh > ld (either stride), non-positive B / T / NH / dh / max_pos,
 * T > max_pos with start == NULL, a null pointer, dx == g in nk_rope_bwd, x == y with different strides. */
int nk_rope_table(nk_device* dev, float* table, int max_pos, int rot, double base);
int nk_rope_fwd(nk_device* dev, const float* x, int ldx, float* y, int ldy, const float* table, const int* start, int B, int T, int NH,
                int dh, int rot, int max_pos, int interleaved);
int nk_rope_bwd(nk_device* dev, float* dx, int lddx, const float* g, int ldg, const float* table, const int* start, int B, int T, int NH,
                int dh, int rot, int max_pos, int interleaved);
int nk_rope_bwd_assign(nk_device* dev, float* dx, int lddx, const float* g, int ldg, const float* table, const int* start, int B, int T,
                       int NH, int dh, int rot, int max_pos, int interleaved);
/* ------------------------------------------------------------------ token sampling --
 * Ours (the reference has no generation loop): the next token of each row of logits - greedy, temperature, top-k (Fan et al. 2018) and
 * top-p / nucleus (Holtzman et al. 2020) - chosen on the device and written as f32, the form nk_embedding_fwd takes its ids in.
 * Row r is logits + r*ld, ld >= V (the last of T positions per sample: logits + (T-1)*V, ld = T*V).  ids[r] receives the chosen index
 * (V <= 2^20 keeps it exact).  logits is never written.  Per row, independently of every other row:
 *  1. Order.  Tokens are ordered by value; -0 counts as +0; NaN sorts below -inf; equal values: the lower index first.  m is the
 *     largest value.
 *  2. Greedy.  temperature == 0 returns the lowest index that holds m.  So does a row whose m is not finite (+inf, or a row of only
 *     -inf / NaN).  No draw is taken, top_k and top_p are ignored.
 *  3. Top-k.  top_k <= 0 or top_k >= V turns it off.  Otherwise S = {i : x_i >= the top_k-th largest value}.  Ties at the threshold
 *     all stay, as in the usual `logits < kth` filter.
 *  4. Weights.  e_i = exp2f((x_i - m) * c) with c = 1.44269504f / temperature formed once in f32; w_i = (uint64)(e_i * 2^40),
 *     truncated, for i in S; w_i = 0 for NaN and -inf.  The maximum has w = 2^40 exactly, so W = sum w_i >= 2^40.  All sums are 64-bit
 *     integer sums: exact and independent of order (V <= 2^20 keeps W < 2^61).
 *  5. Top-p.  top_p >= 1 turns it off.  Otherwise target = (uint64)((double)top_p * (double)W), at least 1, and the kept set shrinks
 *     to {i in S : x_i >= t}, t the largest value for which the weights of {i in S : x_i >= t} sum to >= target.  Ties stay again.
 *     W becomes that sum.
 *  6. Draw.  One Philox4x32-10 call, counter (lo32(offset), hi32(offset), r, 0x53414D50), key (lo32(seed), hi32(seed)); the fourth
 *     counter word keeps this stream apart from dropout, whose counters end in 0, 0.  r64 = word1 << 32 | word0, R = mulhi64(r64, W).
 *     The id is the lowest kept index whose running weight sum in index order exceeds R.  A token of weight 0 is never drawn.
 * Every decision is an integer comparison: the id of a row depends on its V logits and on (temperature, top_k, top_p, seed, offset, r)
 * only - not on rows, ld, pointer alignment, the kernel family (16-byte or scalar loads) or whether the row was staged in LDS
 * (V <= nk_sample_stage_limit(), a compile-time constant; longer rows are re-read from memory by the later passes).
 * One workgroup per row; integer LDS atomics only; the library allocates nothing in the call.  With temperature > 0 the call refuses
 * stream capture, as nk_dropout_fwd does (offset is a kernel argument); the greedy form can be captured.
 * NK_ERR_INVALID, nothing written: a null pointer, rows <= 0, V <= 0 or V > 2^20, ld < V, temperature negative or not finite, top_p
 * NaN or <= 0. */
int nk_sample_fwd(nk_device* dev, const float* logits, long long ld, int rows, int V, float* ids, float temperature, int top_k, float top_p,
                  uint64_t seed, uint64_t offset);
int nk_sample_stage_limit(void);
/* ------------------------------------------------------------------ weight-only quantised Linear --
 * Ours (the reference has no such layer): W8A32 / W4A32 - integer weights with per-group f32 scales, f32 activations and
 * accumulation - for the projections of incremental decoding, where M = 1 .. 8 rows of x meet the whole weight matrix and the
 * step is as fast as the weights can be read.  Inference only.
 * Format, for a Linear weight W of shape (N = out, K = in), row-major, so that an external packer can produce it:
 *   bits    8 or 4; qmax = 127 / 7.
 *   group   32, 64 or 128 consecutive k of one row, or 0 for one group per row.  K % 32 == 0, and K % group == 0 when group > 0.
 *   scale   per row n and group g, symmetric: s = fl32(absmax / qmax), one IEEE f32 division.
 *   q       clamp(rint(fl32(w / s)), -qmax, qmax), round-half-even; s == 0 gives q = 0.
 *   value   w^ = fl32(float(q) * s), one rounding.
 *   qw      rows contiguous, K * bits / 8 bytes each: int8 as two's-complement bytes; int4 as the unsigned nibble q + 8, element k in
 *           byte k / 2, even k in the low nibble.  nk_quant_linear_words(N, K, bits) floats hold it; the allocation is an ordinary
 *           float* of opaque words (as mask_bits are), 16-byte aligned.
 *   scales  (N, K / group) f32, or (N, 1) for group 0: nk_quant_linear_scales(N, K, group) floats.
 *   Non-finite weights give unspecified values; the calls stay memory-safe.
 * Both size functions return 0 for a geometry the calls refuse.
 * nk_quant_linear_pack: W (row stride ldw) -> qw, scales, on the device.  nk_quant_linear_unpack: w^ into W (row stride ldw; nothing
 *   beyond a row's K columns is written).
 * nk_quant_linear_fwd: y[m][n] = bias[n] + sum_k x[m][k] * w^[n][k] for M rows; x row m at x + m*ldx, y row m at y + m*ldy (a column
 *   block of a wider buffer either way); bias may be NULL.  Two paths, chosen from (M, bits) alone:
 *   rows  M <= L(bits) = nk_quant_linear_rows_rule(bits) (measured; NK_TUNE_QUANT_ROWS overrides): up to 8 rows of x per pass over the
 *         weights, ceil(M / 8) passes.  The weights go from memory to registers in 16-byte loads and are never written back as f32.
 *         The scale is applied per UNIT of 16 consecutive k (a unit lies inside one group):
 *             p   = fma(x[k+15], float(q[k+15]), ... fma(x[k], float(q[k]), 0))
 *             acc = fma(s, p, acc)
 *         i.e. acc += s * sum_unit(x * float(q)), not a sum of x * w^.  A 16-byte chunk of a weight row (16 int8 / 32 int4 elements)
 *         belongs to lane (chunk % 64) of the row's wave, a lane adds its units in ascending k, the 64 lane sums meet in an xor
 *         butterfly (offsets 32 .. 1), then the bias is added: a compile-time function of (bits, K).  No split of K, no workspace, no
 *         atomics, nothing allocated - the path can sit in a captured region.
 *         Bit contract: the bits of y[m][n] depend on x[m, :], row n of qw and scales, bias[n] and (bits, group, K) only - not on M,
 *         N, the other rows, ldx / ldy, pointer alignment of x, or the pass a row falls in.  A sequence decoded alone gets the bits it
 *         gets in a batch, as with the decode attention kernels.
 *   many  M > L: unpack into a scratch region of the device handle (N*K floats; its growth refuses stream capture like the
 *         workspace's), then the f32 GEMM.  With a bias and ldx == K, ldy == N the bits are exactly nk_linear_fwd's over the unpacked
 *         weights; otherwise nk_sgemm's with the bias added afterwards.
 * NK_ERR_INVALID, nothing written: bits not 8 / 4, group not 32 / 64 / 128 / 0, K % 32 != 0, K % group != 0, non-positive N or K,
 * M < 0 (M == 0 is an empty success), a null pointer other than bias, ldx < K, ldy < N, ldw < K, qw not 16-byte aligned. */
size_t nk_quant_linear_words(int N, int K, int bits);
size_t nk_quant_linear_scales(int N, int K, int group);
int nk_quant_linear_rows_rule(int bits);
int nk_quant_linear_pack(nk_device* dev, const float* W, int ldw, float* qw, float* scales, int N, int K, int bits, int group);
int nk_quant_linear_unpack(nk_device* dev, const float* qw, const float* scales, float* W, int ldw, int N, int K, int bits, int group);
int nk_quant_linear_fwd(nk_device* dev, const float* x, int ldx, const float* qw, const float* scales, const float* bias, float* y, int ldy,
                        int M, int N, int K, int bits, int group);
/* ------------------------------------------------------------------ dropout ------------ */
/* Dropout::forward node/dropout/mod.rs:53-79.  train && 0<p<1: noise ~ Bernoulli(1-p) in
 * {0,1} is (re)drawn from Philox4x32-10(seed, offset) and written to `noise` (f32, like the
 * reference's shared noise array); y = x*noise/(1-p).  Draw layout (shared by every masked entry point): call
 * `offset + i/8` serves elements 8(i/8) .. +7; element i takes word (i%8)/2 of it, rotated by 16 bits for odd i, and
 * is kept iff that 32-bit value < floor((1-p) * 2^32) - rand 0.8's Bernoulli construction on 32 bits.  One forward
 * over n elements consumes ceil(n/8) calls: the host advances `offset` by that much per forward.  !train or p==0: y = x.  p==1: y = 0
 * and `noise` is left untouched.  p outside [0,1] -> NK_ERR_INVALID (reference panics,
 * dropout/mod.rs:38-40). */
int nk_dropout_fwd(nk_device* dev, const float* x, float* y, float* noise, size_t n, double p,
                   int train, uint64_t seed, uint64_t offset);
/* DropoutBackward::backward :113-128.  !train or p==0: dx += g; else dx += g*noise
 * (NOT divided by 1-p: reference behaviour, kept). */
int nk_dropout_bwd(nk_device* dev, float* dx, const float* g, const float* noise, size_t n,
                   double p, int train);

/* ------------------------------------------------------------------ layout glue -------- */
/* Chunk::forward node/chunk/mod.rs:48-64 ; ChunkBackward :99-113.  `chunk_no` indexes
 * ndarray's exact_chunks(chunk_shape) iteration order (row-major over the chunk grid). */
int nk_chunk_fwd(nk_device* dev, const float* x, const int* x_shape, float* y,
                 const int* chunk_shape, int nd, int chunk_no);
int nk_chunk_bwd(nk_device* dev, float* dx, const int* x_shape, const float* g,
                 const int* chunk_shape, int nd, int chunk_no);
/* MultiConcatenate::forward node/multi_concatenate/mod.rs:37-50 ; backward :81-97.
 * One call per operand: copies/accumulates the slice [offset, offset+op_len) of `axis`. */
int nk_concat_fwd_part(nk_device* dev, const float* operand, float* out, const int* out_shape,
                       int nd, int axis, int offset, int op_len);
int nk_concat_bwd_part(nk_device* dev, float* d_operand, const float* g, const int* g_shape,
                       int nd, int axis, int offset, int op_len);
/* Transpose::forward node/transpose/mod.rs:28-37 (reversed axes) ; backward :62-69 */
int nk_transpose_fwd(nk_device* dev, const float* x, float* y, const int* x_shape, int nd);
int nk_transpose_bwd(nk_device* dev, float* dx, const float* g, const int* x_shape, int nd);
/* Head split / merge for the composed attention = Chunk((S,dh)) for every (b,h) tile followed
 * by the per-tile consumers, collapsed into one strided copy:  x[(B*S), H*dh] <-> y[B*H, S, dh].
 * fwd overwrites, bwd accumulates — the same data movement as B*H Chunk nodes
 * (var.rs:401-417) resp. cat(axis 1) per sample then cat(axis 0) (var.rs:564-584). */
int nk_split_heads_fwd(nk_device* dev, const float* x, float* y, int B, int S, int H, int dh);
int nk_split_heads_bwd(nk_device* dev, float* dx, const float* g, int B, int S, int H, int dh);
int nk_merge_heads_fwd(nk_device* dev, const float* x, float* y, int B, int S, int H, int dh);
int nk_merge_heads_bwd(nk_device* dev, float* dx, const float* g, int B, int S, int H, int dh);

/* ------------------------------------------------------------------ optimizer (next row)  */
/* Every optimizer first adds the penalty to the gradient IN PLACE, as the reference does
 * (`grad += penalize(w)`; Penalty penalty.rs:63-79: L1 -> l1*signum(w) with Rust's signum
 * (+-0 -> +-1), L2 -> 2*l2*w, ElasticNet -> both; l1 = l2 = 0: no penalty), then updates w.
 * Optimizer state buffers are owned by the host and start zeroed.
 *
 * SGDParam::optimize  neuronika-optim/src/sgd/mod.rs:186-236: velocity == NULL (momentum <=
 * f32::EPSILON): w -= grad*lr.  Otherwise buffer = buffer*momentum + grad*(1-dampening);
 * nesterov: w -= (grad + buffer*momentum)*lr, else w -= buffer*lr. */
int nk_sgd_step(nk_device* dev, float* w, float* grad, float* velocity, size_t n, float lr,
                float momentum, float dampening, int nesterov, float l1, float l2);
/* The same update for `count` parameters in ONE launch (`Optimizer::step`, optimizer.rs:81-86, walks the registered
 * parameters; their updates are independent): w[i], grad[i], n[i] as above, velocity == NULL or velocity[i] == NULL without
 * momentum.  Element for element the arithmetic of nk_sgd_step. */
int nk_sgd_step_multi(nk_device* dev, int count, float* const* w, float* const* grad, float* const* velocity, const size_t* n,
                      float lr, float momentum, float dampening, int nesterov, float l1, float l2);
/* AdamParam::optimize adam/mod.rs:131-169 ; AMSGradParam::optimize amsgrad/mod.rs:163-205 when
 * max_exp_avg_sq != NULL.  `step` is the 1-based step count (bias corrections 1 - beta^step). */
int nk_adam_step(nk_device* dev, float* w, float* grad, float* exp_avg, float* exp_avg_sq,
                 float* max_exp_avg_sq, size_t n, float lr, float beta1, float beta2, float eps, int step,
                 float l1, float l2);
/* AdamW (ours: the reference has only the coupled `Penalty`, which the Adam denominator rescales) for `count` parameters in
 * as few launches as the parameter table allows (32 entries per launch).  Per element, in f32, in this order:
 *     w   = w * (1 - lr * weight_decay)                 skipped when weight_decay == 0
 *     m   = m * beta1 + g * (1 - beta1)
 *     v   = v * beta2 + g * g * (1 - beta2)
 *     den = vmax ? (vmax = max(vmax, v)) : v
 *     w   = w - m / (sqrt(den) / sqrt(bc2) + eps) * (lr / bc1)
 * with bc1 = 1 - beta1^step[i], bc2 = 1 - beta2^step[i] formed on the host as nk_adam_step forms them; step[i] is the 1-based
 * step number of parameter i.  The Adam part is the expression of nk_adam_step: weight_decay == 0 is the project's Adam
 * without a penalty.  The gradient is read, never written.  max_exp_avg_sq == NULL, or max_exp_avg_sq[i] == NULL: no
 * AMSGrad maximum (for that parameter).  Entries of length 0 are skipped; count == 0 does nothing.  NK_ERR_INVALID: a null
 * table with count > 0, a null pointer in an entry of non-zero length, step[i] < 1, the same w pointer twice in one call (a
 * caller that registers a parameter twice issues the second update in a later call).  Refuses capture like nk_adam_step:
 * the bias corrections are kernel arguments. */
int nk_adamw_step_multi(nk_device* dev, int count, float* const* w, const float* const* grad, float* const* exp_avg,
                        float* const* exp_avg_sq, float* const* max_exp_avg_sq, const size_t* n, const int* step,
                        float lr, float beta1, float beta2, float eps, float weight_decay);
/* One parameter through the multi-parameter kernel. */
int nk_adamw_step(nk_device* dev, float* w, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                  size_t n, float lr, float beta1, float beta2, float eps, int step, float weight_decay);
/* Global-norm gradient clipping over a list of gradients, on the device, without a host synchronisation:
 *     total_norm = (float)sqrt(sum over every element of (double)g^2)      every square and the whole sum in f64
 *     coef       = max_norm / (total_norm + 1e-6f), replaced by 1.0f when it exceeds 1
 *     g         *= coef                                                    for every gradient of the list
 * out (device, 2 floats) receives {total_norm, coef}.  The sum has a fixed order that depends on the lengths alone (one f64
 * partial per 4096-element chunk, the partials added in a fixed order by one block; no atomics): the result repeats bit for
 * bit and does not depend on pointer alignment.  A coefficient of exactly 1 leaves the gradients untouched (the scaling
 * kernel returns before it reads them); max_norm == +inf measures only (no scaling launch).  Entries of length 0 are
 * skipped; count == 0 or all lengths 0: out = {0, 1}.  Non-finite gradients propagate as the arithmetic produces them: a NaN
 * anywhere makes total_norm, coef and every scaled gradient NaN; an infinite norm gives coef = 0 (inf * 0 = NaN in the
 * infinite elements).  NK_ERR_INVALID: a null table with count > 0, a null pointer in an entry of non-zero length, out ==
 * NULL, max_norm NaN or <= 0, the same grad pointer twice in one call (a caller lists a parameter once).  Takes nothing
 * step-dependent from the host and allocates nothing beyond the workspace: it CAN be captured, after one eager call of the
 * same sizes (which grows the workspace). */
int nk_clip_grad_norm_multi(nk_device* dev, int count, float* const* grad, const size_t* n, float max_norm, float* out);
/* AdagradParam::optimize adagrad/mod.rs:113-140: clr = lr / (1 + (step-1)*lr_decay). */
int nk_adagrad_step(nk_device* dev, float* w, float* grad, float* grad_sq, size_t n, float lr,
                    float lr_decay, float eps, int step, float l1, float l2);
/* RMSPropParam::optimize rmsprop/mod.rs:193-296: grad_avg != NULL selects the centered variant,
 * buffer != NULL the momentum variant (all four combinations). */
int nk_rmsprop_step(nk_device* dev, float* w, float* grad, float* square_avg, float* grad_avg,
                    float* buffer, size_t n, float lr, float alpha, float eps, float momentum, float l1,
                    float l2);

/* ------------------------------------------------------------------ data parallel ------ */
/* Net-new (the reference has no communication backend).  One nk_comm per process/GPU; the
 * 128-byte unique id is created on rank 0 and distributed by the host (any side channel). */
#define NK_COMM_ID_BYTES 128
int nk_comm_unique_id(char id[NK_COMM_ID_BYTES]);
int nk_comm_init_rank(nk_device* dev, int nranks, int rank, const char id[NK_COMM_ID_BYTES],
                      nk_comm** out);
/* Single process, one host thread per GPU: the communicators of `ndev` device handles of THIS process at
 * once (ncclCommInitAll); out[i] belongs to devs[i] and is rank i of ndev.  Each thread then drives its own communicator
 * with the calls below; no unique id has to travel. */
int nk_comm_init_all(int ndev, nk_device* const* devs, nk_comm** out);
/* A communicator of `nranks` virtual ranks that all hold THIS rank's values (no RCCL, no peers):
 * its sum all-reduce multiplies the buffer by nranks on the side stream, with the same stream
 * ordering as the real one.  Lets a single GPU check that an exchange schedule covers every
 * element of every gradient exactly once (a sum over ONE real rank is the identity and would
 * hide a wrong offset or count) and price the schedule without fabric traffic. */
int nk_comm_init_replicas(nk_device* dev, int nranks, int channels, double gbps, nk_comm** out);
int nk_comm_destroy(nk_comm* comm);
/* In-place sum all-reduce of buf[0..n) on the device's SIDE stream.  The side stream first
 * waits for `after` (an event recorded on the compute stream once the bucket's gradients are
 * final; NULL: waits for everything enqueued on the compute stream so far). */
int nk_allreduce_sum_async(nk_comm* comm, float* buf, size_t n, nk_event* after);
/* The same for a list of buffers as ONE RCCL group (one fused launch): for the small,
 * latency-bound gradients (biases) of a step. */
int nk_allreduce_sum_group_async(nk_comm* comm, float* const* bufs, const size_t* counts, int nbufs,
                                 nk_event* after);
/* Make the compute stream wait for all all-reduces issued so far (no host sync). */
int nk_comm_join(nk_comm* comm);
int nk_comm_rank(const nk_comm* comm);
int nk_comm_size(const nk_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* NEURONIKA_HIP_H */
