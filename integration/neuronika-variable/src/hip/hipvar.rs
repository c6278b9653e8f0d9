//! `HipVar` / `HipVarDiff`: the device twins of `Var` / `VarDiff` (`var.rs:34-40`, `vardiff.rs:35-42`), shaped like the
//! reference's own accelerator template (`CuVar`, `cuda/cuvar.rs:19-100`).  Every method below builds the same tape entry as
//! its reference counterpart - same operand handles, same `History` merge, outputs and gradients allocated zeroed at
//! graph-build time - with a node whose body is one call of the C ABI (`node/*.rs`).  Shape rules stay on the host
//! (`cobroadcast`, `conv_out_shape`, `check_conv_args`: `utils.rs:46-55,97-125,207-237,427-497`).
use std::{
    cell::{Cell, RefCell},
    rc::Rc,
};

use ndarray::{Axis, DimMax, Dimension, IntoDimension, Ix0, Ix1, Ix2, Ix3, Ix4, RemoveAxis};

use super::{
    device::Device,
    ffi,
    dp::GradientSync,
    hiparray::HipArray,
    node::{
        Activation, ActivationBackward, Glu, GluBackward,
        AttentionState, BinaryOp, BinaryOperation, BinaryOperationBackwardLeft, BinaryOperationBackwardRight, Chunk, ChunkBackward,
        Convolution, ConvolutionBackwardInput, ConvolutionBackwardKernel, ConvolutionBackwardKernelBias, ConvolutionBackwardPadded, ConvolutionBias,
        ConvolutionBiasPadded, CrossEntropy, CrossEntropyBackward, Dropout, Embedding, EmbeddingBackward,
        AvgPool, AvgPoolBackward, MaxPool, MaxPoolBackward,
        DropoutBackward, Heads, HeadsAttention, HeadsAttentionBackward, BatchNorm, BatchNormBackward, LayerNorm, LayerNormBackward, GroupNorm, GroupNormBackward, RmsNorm, RmsNormBackward, Linear, LinearBackward, LogSoftmax, LogSoftmaxBackward, MatrixMatrixMul, MatrixMatrixMulBackwardLeft,
        MatrixMatrixMulBackwardRight, MatrixMatrixMulT, MatrixMatrixMulTBackwardLeft, MatrixMatrixMulTBackwardRight, Mean, MeanBackward,
        decode_chunk, decode_paged_workspace, decode_window_workspace, decode_workspace, PackedDecodeAttention, PagedDecodeAttention,
        RepeatKv, RepeatKvBackward, RepeatKvGeometry, rope_table, Rope, RopeBackward, RopeGeometry, RopeInPlace, RopeInPlaceBackward,
        sample_stage_limit, Sample, SampleParams,
        quant_linear_rows_rule, QuantLinear, QuantWeight,
        Upsample, UpsampleBackward, UpsampleGeometry, UpsampleMode,
        MultiConcatenate, MultiConcatenateBackward, PackedHeadsAttention, PackedHeadsAttentionBackward, Pad, PadBackward, PadMode, Pair, ReLU,
        ReLUBackward, ReluMask, Softmax, SoftmaxBackward,
        SquaredError, SquaredErrorBackward, Sum, SumBackward, Transpose, TransposeBackward,
    },
};
use crate::{
    autograd::{Backward, Forward},
    gradient::{Gradient, NoGrad},
    history::History,
    utils::{check_conv_args, check_groups_args, cobroadcast, conv_out_shape, Broadcast, Shared},
    Reduction,
};

type Fwd = History<(Rc<dyn Forward>, Cell<bool>)>;
type Bwd = History<(Rc<dyn Backward>, Rc<dyn NoGrad>)>;

/// Host side of the pooling geometry (`nk_pool_out_shape` holds the rules): the per-axis vectors for the C ABI and the output dimension.
/// An empty `stride` means `stride = kernel`.
fn pool_setup<D: Dimension>(dim: &D, kernel: &[usize], stride: &[usize], padding: &[usize]) -> (D, Vec<i32>, Vec<i32>, Vec<i32>) {
    let xs: Vec<i32> = dim.slice().iter().map(|&e| e as i32).collect();
    assert!((3..=5).contains(&xs.len()), "pooling: the input must be (N, C, spatial...) with 1 to 3 spatial axes");
    let nd = xs.len() - 2;
    let stride = if stride.is_empty() { kernel } else { stride };
    assert!(kernel.len() == nd && stride.len() == nd && padding.len() == nd, "pooling: kernel, stride and padding take {} entries each", nd);
    let to_c = |v: &[usize]| v.iter().map(|&e| e as i32).collect::<Vec<i32>>();
    let (k, s, p) = (to_c(kernel), to_c(stride), to_c(padding));
    let mut ys = vec![0i32; xs.len()];
    ffi::check(unsafe { ffi::nk_pool_out_shape(nd as i32, xs.as_ptr(), k.as_ptr(), s.as_ptr(), p.as_ptr(), ys.as_mut_ptr()) });
    let mut out = dim.clone();
    for (o, &y) in out.slice_mut().iter_mut().zip(&ys) {
        *o = y as usize;
    }
    (out, k, s, p)
}

/// Host side of the upsampling geometry (`nk_upsample_fwd` holds the rules): the mode by its torch name, checked against the number of
/// spatial axes, and the output dimension `(N, C, out...)`.
fn upsample_setup<D: Dimension>(dim: &D, out_size: &[usize], mode: &str, align_corners: bool) -> (D, UpsampleGeometry) {
    let nd = dim.ndim().saturating_sub(2);
    assert!((1..=3).contains(&nd), "upsample: the input must be (N, C, spatial...) with 1 to 3 spatial axes");
    assert!(out_size.len() == nd, "upsample: out_size takes {} entries", nd);
    let mode = match (mode, nd) {
        ("nearest", _) => UpsampleMode::Nearest,
        ("linear", 1) | ("bilinear", 2) | ("trilinear", 3) => UpsampleMode::Linear,
        _ => panic!("upsample: mode {:?} does not fit {} spatial axes (nearest, linear, bilinear, trilinear)", mode, nd),
    };
    assert!(mode == UpsampleMode::Linear || !align_corners, "upsample: align_corners has no meaning for the nearest mode");
    assert!(out_size.iter().all(|&e| e >= 1), "upsample: output extents must be >= 1");
    let mut out = dim.clone();
    for (o, &e) in out.slice_mut()[2..].iter_mut().zip(out_size) {
        *o = e;
    }
    (out, UpsampleGeometry { out_size: out_size.iter().map(|&e| e as i32).collect(), mode, align_corners })
}

fn shared<D: Dimension>(dim: D, device: &Device) -> Shared<HipArray<D>> {
    Rc::new(RefCell::new(HipArray::zeroed(dim, device.clone())))
}

/// Seed of the next random node (dropout): the Philox key.  `thread_rng` in the reference (`node/dropout/mod.rs:70`) is
/// non-reproducible by design; a counter-based generator keyed per node keeps masks reproducible and per-rank distinct.
thread_local! {
    static NEXT_SEED: Cell<u64> = Cell::new(0x9E37_79B9_7F4A_7C15);
}

/// Fixes the key of the next random node created on this thread (each node advances it).
pub fn manual_seed(seed: u64) {
    NEXT_SEED.with(|s| s.set(seed));
}

fn next_seed() -> u64 {
    NEXT_SEED.with(|s| {
        let v = s.get();
        s.set(v.wrapping_add(0x9E37_79B9_7F4A_7C15));
        v
    })
}

/// The reference's padding modes (`node/pad/{zero,constant,reflective,replicative}/mod.rs`) as one value type.
#[derive(Clone, Copy, Debug, PartialEq)]
pub enum PaddingMode {
    Zero,
    Constant(f32),
    Reflective,
    Replicative,
}

/// The gate of `glu` (ours: the reference has no gated activation): a value of `enum nk_activation` in `include/neuronika_hip.h`.
/// `Sigmoid` is GLU (torch's `F.glu`), `Gelu` / `GeluTanh` are GeGLU, `Silu` is SwiGLU.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Gate {
    Gelu = 0,
    GeluTanh = 1,
    Silu = 2,
    Sigmoid = 3,
}

impl From<PaddingMode> for PadMode {
    fn from(mode: PaddingMode) -> Self {
        match mode {
            PaddingMode::Zero => PadMode::Constant(0.),
            PaddingMode::Constant(value) => PadMode::Constant(value),
            PaddingMode::Reflective => PadMode::Reflective,
            PaddingMode::Replicative => PadMode::Replicative,
        }
    }
}

/// A non-differentiable variable with data in HBM.  Same fields and tape as `Var<D>` (`var.rs:34-40`) /
/// `CuVar<D>` (`cuda/cuvar.rs:19-46`): only the array type differs.
pub struct HipVar<D>
where
    D: Dimension,
{
    pub(crate) data: Shared<HipArray<D>>,
    pub(crate) history: Fwd,
}

impl<D: Dimension> Clone for HipVar<D> {
    fn clone(&self) -> Self {
        Self { data: self.data.clone(), history: self.history.clone() }
    }
}

impl<D> HipVar<D>
where
    D: 'static + Dimension,
{
    pub(crate) fn leaf(array: HipArray<D>) -> Self {
        Self { data: Rc::new(RefCell::new(array)), history: History::default() }
    }

    /// Uploads a host array (`CuVar::from_ndarray`-style entry; `neuronika::from_ndarray`, `lib.rs`).
    pub fn from_ndarray(array: &ndarray::Array<f32, D>, device: Device) -> Self {
        Self::leaf(HipArray::from_ndarray(array, device))
    }

    pub(crate) fn node(data: Shared<HipArray<D>>, op: Rc<dyn Forward>, mut history: Fwd) -> Self {
        history.insert(Rc::as_ptr(&op) as *const () as usize, (op, Cell::default()));
        Self { data, history }
    }

    fn device(&self) -> Device {
        self.data.borrow().device().clone()
    }

    /// Promotes to a differentiable leaf (`Var::requires_grad`, `var.rs:138-148`).
    pub fn requires_grad(self) -> HipVarDiff<D> {
        let (dim, device) = (self.data.borrow().dimension(), self.device());
        HipVarDiff { var: self, grad: Rc::new(Gradient::hip_zeros(dim, device)), history: History::default(), relu_mask: None }
    }

    /// `Var::forward` (`var.rs:110-128`), verbatim logic: the ops are enqueued on the device's compute stream in
    /// tape order and return immediately; nothing synchronises until the host reads data back.
    pub fn forward(&self) {
        let mut buffer = self.history.buffer_mut();
        if buffer.is_empty() {
            *buffer = self.history.to_vec()
        } else {
            buffer.iter().for_each(|(_, computed)| computed.set(false));
        }
        buffer.iter().filter(|(_, computed)| !computed.get()).for_each(|(op, computed)| {
            op.forward();
            computed.set(true)
        });
    }

    /// Extents of the data, without touching the device.
    pub fn shape(&self) -> Vec<usize> {
        self.data.borrow().dimension().slice().to_vec()
    }

    /// Host copy of the data (synchronises), `Var::data` (`var.rs:131-136`).
    pub fn data(&self) -> ndarray::Array<f32, D> {
        self.data.borrow().as_ndarray()
    }

    /// Broadcast binary (`Addition` ... `Division`): shape rule `cobroadcast` (`utils.rs:97-125`) stays on the host.
    pub(crate) fn binary<E>(mut self, op: BinaryOp, rhs: HipVar<E>) -> HipVar<Broadcast<D, E>>
    where
        D: DimMax<E>,
        E: 'static + Dimension,
    {
        self.history.merge(rhs.history);
        let dim = cobroadcast(self.data.borrow().dimension(), rhs.data.borrow().dimension());
        let data = shared(dim, &self.device());
        let node = Rc::new(BinaryOperation::new(op, self.data, rhs.data, data.clone()));
        HipVar::node(data, node, self.history)
    }

    /// `Var::sum` (`var.rs:201-207`).
    pub fn sum(self) -> HipVar<Ix0> {
        let data = shared(ndarray::Dim(()), &self.device());
        let op = Sum::new(self.data, data.clone());
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// `Var::mean` (`var.rs:209-214`).
    pub fn mean(self) -> HipVar<Ix0> {
        let data = shared(ndarray::Dim(()), &self.device());
        let op = Mean::new(self.data, data.clone());
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// `Var::relu` (`var.rs:243-249`).
    pub fn relu(self) -> HipVar<D> {
        let data = shared(self.data.borrow().dimension(), &self.device());
        let op = ReLU::new(self.data, data.clone());
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// GELU `x Phi(x)` in the erfc form (ours: the reference has none; semantics in `include/neuronika_hip.h`): ONE node.
    pub fn gelu(self) -> HipVar<D> {
        self.activation(Gate::Gelu)
    }

    /// GELU in the tanh form, `0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3)))`: ONE node.
    pub fn gelu_tanh(self) -> HipVar<D> {
        self.activation(Gate::GeluTanh)
    }

    /// SiLU `x sigma(x)`: ONE node.
    pub fn silu(self) -> HipVar<D> {
        self.activation(Gate::Silu)
    }

    fn activation(self, act: Gate) -> HipVar<D> {
        let data = shared(self.data.borrow().dimension(), &self.device());
        let op = Activation::new(self.data, data.clone(), act as i32);
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// `a * gate(b)` over the two halves `(a, b)` of the last axis, which must be even: ONE node (`nk_glu_fwd`).
    pub fn glu(self, gate: Gate) -> HipVar<D> {
        let mut dim = self.data.borrow().dimension();
        let last = dim.ndim().checked_sub(1).expect("glu: a scalar has no last axis");
        assert!(dim[last] % 2 == 0 && dim[last] > 0, "glu: the last axis must have an even extent");
        dim[last] /= 2;
        let half = dim[last];
        let data = shared(dim, &self.device());
        let op = Glu::new(self.data, data.clone(), gate as i32, half);
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// `Var::softmax` (`var.rs:318-330`).
    pub fn softmax(self, axis: usize) -> HipVar<D> {
        let data = shared(self.data.borrow().dimension(), &self.device());
        let op = Softmax::new(self.data, data.clone(), axis);
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// Layer normalisation over the trailing dimensions, which must equal `gamma`'s shape (`beta`'s equals it): ours, the
    /// reference has no normalisation node.  `stats` = the per-row `{mean, rstd}` buffer a backward node will read, `None` for
    /// the no-gradient form (`layer_norm`).
    pub(crate) fn layer_norm_with_stats<E: 'static + Dimension>(mut self, gamma: HipVar<E>, beta: HipVar<E>, eps: f64,
                                                                 stats: Option<Shared<HipArray<Ix2>>>) -> HipVar<D> {
        let (xs, ns) = (self.data.borrow().shape_c(), gamma.data.borrow().shape_c());
        assert!(!ns.is_empty() && ns.len() <= xs.len() && xs[xs.len() - ns.len()..] == ns[..], "layer_norm: gamma must have the shape of the input's trailing dimensions");
        assert!(beta.data.borrow().shape_c() == ns, "layer_norm: beta must have gamma's shape");
        assert!(eps >= 0.0 && eps.is_finite(), "layer_norm: eps must be finite and not negative");
        self.history.merge(gamma.history);
        self.history.merge(beta.history);
        let data = shared(self.data.borrow().dimension(), &self.device());
        let op = LayerNorm::new(self.data, gamma.data, beta.data, data.clone(), stats, eps);
        HipVar::node(data, Rc::new(op), self.history)
    }

    pub fn layer_norm<E: 'static + Dimension>(self, gamma: HipVar<E>, beta: HipVar<E>, eps: f64) -> HipVar<D> {
        self.layer_norm_with_stats(gamma, beta, eps, None)
    }

    /// RMS normalisation over the trailing dimensions, which must equal `gamma`'s shape: ours, the reference has no normalisation
    /// node.  `stats` = the per-row `rstd` buffer a backward node will read, `None` for the no-gradient form (`rms_norm`).
    pub(crate) fn rms_norm_with_stats<E: 'static + Dimension>(mut self, gamma: HipVar<E>, eps: f64, stats: Option<Shared<HipArray<Ix1>>>) -> HipVar<D> {
        let (xs, ns) = (self.data.borrow().shape_c(), gamma.data.borrow().shape_c());
        assert!(!ns.is_empty() && ns.len() <= xs.len() && xs[xs.len() - ns.len()..] == ns[..], "rms_norm: gamma must have the shape of the input's trailing dimensions");
        assert!(eps >= 0.0 && eps.is_finite(), "rms_norm: eps must be finite and not negative");
        self.history.merge(gamma.history);
        let data = shared(self.data.borrow().dimension(), &self.device());
        let op = RmsNorm::new(self.data, gamma.data, data.clone(), stats, eps);
        HipVar::node(data, Rc::new(op), self.history)
    }

    pub fn rms_norm<E: 'static + Dimension>(self, gamma: HipVar<E>, eps: f64) -> HipVar<D> {
        self.rms_norm_with_stats(gamma, eps, None)
    }

    /// Group normalisation of an `(N, C, spatial...)` input over `groups` channel groups, `gamma` / `beta` of shape `(C)`: ours,
    /// the reference has no normalisation node.  `groups == C` is instance normalisation.  `stats` = the `{mean, rstd}` buffer per
    /// `(sample, group)` a backward node will read, `None` for the no-gradient form (`group_norm`).
    pub(crate) fn group_norm_with_stats(mut self, groups: usize, gamma: HipVar<Ix1>, beta: HipVar<Ix1>, eps: f64,
                                        stats: Option<Shared<HipArray<Ix2>>>) -> HipVar<D> {
        let xs = self.data.borrow().shape_c();
        assert!(xs.len() >= 2, "group_norm: the input must have at least two dimensions (N, C, ...)");
        let channels = xs[1] as usize;
        assert!(groups > 0 && channels % groups == 0, "group_norm: the channel count must be a multiple of the group count");
        assert!(gamma.data.borrow().len() == channels && beta.data.borrow().len() == channels, "group_norm: gamma and beta must have shape (C)");
        assert!(eps >= 0.0 && eps.is_finite(), "group_norm: eps must be finite and not negative");
        self.history.merge(gamma.history);
        self.history.merge(beta.history);
        let data = shared(self.data.borrow().dimension(), &self.device());
        let op = GroupNorm::new(self.data, gamma.data, beta.data, data.clone(), stats, groups, eps);
        HipVar::node(data, Rc::new(op), self.history)
    }

    pub fn group_norm(self, groups: usize, gamma: HipVar<Ix1>, beta: HipVar<Ix1>, eps: f64) -> HipVar<D> {
        self.group_norm_with_stats(groups, gamma, beta, eps, None)
    }

    /// Batch normalisation over `(N, spatial...)` for each channel of an `(N, C, spatial...)` input: ours, the reference has no
    /// normalisation node.  `running` = `(running_mean, running_var)`, updated in place by a training forward, or `None` (the
    /// batch statistics then serve in both modes); `status` is the train / eval switch Dropout uses.  `stats` = the per-channel
    /// `{mean, rstd}` buffer a backward node will read with the cell that records the mode of the last run, `None` for the
    /// no-gradient form (`batch_norm`).
    #[allow(clippy::too_many_arguments)]
    pub(crate) fn batch_norm_with_stats(mut self, gamma: HipVar<Ix1>, beta: HipVar<Ix1>, running: Option<(HipVar<Ix1>, HipVar<Ix1>)>, momentum: f64,
                                        eps: f64, status: Rc<Cell<bool>>, stats: Option<(Shared<HipArray<Ix2>>, Rc<Cell<bool>>)>) -> HipVar<D> {
        let xs = self.data.borrow().shape_c();
        assert!(xs.len() >= 2, "batch_norm: the input must have at least two dimensions (N, C, ...)");
        let channels = xs[1] as usize;
        assert!(gamma.data.borrow().len() == channels && beta.data.borrow().len() == channels, "batch_norm: gamma and beta must have shape (C)");
        assert!(eps >= 0.0 && eps.is_finite(), "batch_norm: eps must be finite and not negative");
        assert!((0.0..=1.0).contains(&momentum), "batch_norm: momentum must be in [0, 1]");
        let running = running.map(|(mean, var)| {
            assert!(mean.data.borrow().len() == channels && var.data.borrow().len() == channels, "batch_norm: the running statistics must have shape (C)");
            (mean.data, var.data)
        });
        self.history.merge(gamma.history);
        self.history.merge(beta.history);
        let data = shared(self.data.borrow().dimension(), &self.device());
        let (stats, trained) = match stats {
            Some((s, t)) => (Some(s), t),
            None => (None, Rc::new(Cell::new(true))),
        };
        let op = BatchNorm::new(self.data, gamma.data, beta.data, running, data.clone(), stats, eps, momentum, status, trained);
        HipVar::node(data, Rc::new(op), self.history)
    }

    pub fn batch_norm(self, gamma: HipVar<Ix1>, beta: HipVar<Ix1>, running: Option<(HipVar<Ix1>, HipVar<Ix1>)>, momentum: f64, eps: f64,
                      status: Rc<Cell<bool>>) -> HipVar<D> {
        self.batch_norm_with_stats(gamma, beta, running, momentum, eps, status, None)
    }

    /// Max pooling over the spatial axes (ours, the reference has no pooling; semantics in `include/neuronika_hip.h`).  `indices` = the
    /// offsets buffer a backward node will read, `None` for the no-gradient form (`max_pool`).
    pub(crate) fn max_pool_with_indices(self, kernel: &[usize], stride: &[usize], padding: &[usize], indices: Option<Shared<HipArray<D>>>) -> HipVar<D> {
        let (dim, k, s, p) = pool_setup(&self.data.borrow().dimension(), kernel, stride, padding);
        let data = shared(dim, &self.device());
        let op = MaxPool::new(self.data, data.clone(), indices, k, s, p);
        HipVar::node(data, Rc::new(op), self.history)
    }

    pub fn max_pool(self, kernel: &[usize], stride: &[usize], padding: &[usize]) -> HipVar<D> {
        self.max_pool_with_indices(kernel, stride, padding, None)
    }

    /// Average pooling; `count_include_pad` divides by the window size, otherwise by the number of in-range positions.
    pub fn avg_pool(self, kernel: &[usize], stride: &[usize], padding: &[usize], count_include_pad: bool) -> HipVar<D> {
        let (dim, k, s, p) = pool_setup(&self.data.borrow().dimension(), kernel, stride, padding);
        let data = shared(dim, &self.device());
        let op = AvgPool::new(self.data, data.clone(), k, s, p, count_include_pad);
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// Nearest or linear resampling of the spatial axes to `out_size` (ours, the reference has none; semantics in
    /// `include/neuronika_hip.h`): `mode` is "nearest", or "linear" / "bilinear" / "trilinear" for 1 / 2 / 3 spatial axes.
    pub fn upsample(self, out_size: &[usize], mode: &str, align_corners: bool) -> HipVar<D> {
        let (dim, geometry) = upsample_setup(&self.data.borrow().dimension(), out_size, mode, align_corners);
        let data = shared(dim, &self.device());
        let op = Upsample::new(self.data, data.clone(), geometry);
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// `avg_pool` over the whole spatial extents: `(N, C, 1, ..)`.
    pub fn global_avg_pool(self) -> HipVar<D> {
        let extents: Vec<usize> = self.data.borrow().dimension().slice()[2..].to_vec();
        let zeros = vec![0usize; extents.len()];
        self.avg_pool(&extents, &extents, &zeros, true)
    }

    /// `Var::log_softmax` (`var.rs:332-344`).
    pub fn log_softmax(self, axis: usize) -> HipVar<D> {
        let data = shared(self.data.borrow().dimension(), &self.device());
        let op = LogSoftmax::new(self.data, data.clone(), axis);
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// `Var::t` (`var.rs:346-352`): dimensions reversed.
    pub fn t(self) -> HipVar<D> {
        let mut dim = self.data.borrow().dimension();
        dim.slice_mut().reverse();
        let data = shared(dim, &self.device());
        let op = Transpose::new(self.data, data.clone());
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// `Var::dropout` (`var.rs:375-393`): the noise buffer is shared with the backward node when there is one.
    pub fn dropout(self, p: f64, status: Rc<Cell<bool>>) -> HipVar<D> {
        let noise = shared(self.data.borrow().dimension(), &self.device());
        self.dropout_with_noise(p, noise, status)
    }

    pub(crate) fn dropout_with_noise(self, p: f64, noise: Shared<HipArray<D>>, status: Rc<Cell<bool>>) -> HipVar<D> {
        let data = shared(self.data.borrow().dimension(), &self.device());
        let op = Dropout::new(self.data, data.clone(), p, noise, status, next_seed());
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// `Var::chunks` (`var.rs:401-417`): `exact_chunks(chunk_size)` in row-major chunk order, remainders skipped.
    pub fn chunks<E>(self, chunk_size: E) -> Vec<HipVar<D>>
    where
        E: IntoDimension<Dim = D>,
    {
        let chunk = chunk_size.into_dimension();
        let count: usize = self.data.borrow().dimension().slice().iter().zip(chunk.slice()).map(|(n, c)| n / c).product();
        (0..count)
            .map(|i| {
                let data = shared(chunk.clone(), &self.device());
                let op = Chunk::new(self.data.clone(), data.clone(), i);
                HipVar::node(data, Rc::new(op), self.history.clone())
            })
            .collect()
    }

    /// `Var::cat` (`var.rs:564-584`): `self` followed by `variables` along `axis`.
    pub fn cat(mut self, variables: &[Self], axis: usize) -> HipVar<D> {
        let mut dim = self.data.borrow().dimension();
        let mut operands_data = vec![self.data.clone()];
        variables.iter().cloned().for_each(|variable| {
            dim.slice_mut()[axis] += variable.data.borrow().dimension().slice()[axis];
            self.history.merge(variable.history);
            operands_data.push(variable.data);
        });
        let data = shared(dim, &self.device());
        let op = MultiConcatenate::new(operands_data, data.clone(), axis);
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// `Var::mse` (`var.rs:454-459`).
    pub fn mse(mut self, target: HipVar<D>, reduction: Reduction) -> HipVar<Ix0> {
        self.history.merge(target.history);
        let data = shared(ndarray::Dim(()), &self.device());
        let op = SquaredError::new(self.data, target.data, data.clone(), reduction);
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// `Var::pad` (`var.rs:726-744`) for the four modes of `node/pad/`: `padding[i]` on both sides of spatial axis `i`.
    pub(crate) fn pad_with(self, padding: &[usize], mode: PadMode) -> HipVar<D> {
        let mut dim = self.data.borrow().dimension();
        dim.slice_mut().iter_mut().skip(2).zip(padding).for_each(|(n, p)| *n += 2 * p);
        let data = shared(dim, &self.device());
        let op = Pad::new(self.data, data.clone(), mode, padding.iter().map(|&p| p as i32).collect());
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// Zero padding (`PaddingMode` `Zero`, `node/pad/zero/mod.rs`).
    pub fn pad_zero(self, padding: &[usize]) -> HipVar<D> {
        self.pad_with(padding, PadMode::Constant(0.))
    }
}

impl<D> HipVar<D>
where
    D: 'static + Dimension + RemoveAxis,
{
    /// `Convolution::convolution` for `Var` kernels (`var.rs:1296-1371`): `self` is the KERNEL, as in the reference; checks
    /// and the output shape come from the host-side helpers unchanged.
    pub fn convolution(mut self, input: HipVar<D>, stride: &[usize], dilation: &[usize], groups: usize) -> HipVar<D> {
        self.history.merge(input.history);
        let shape: D = {
            let (x, w) = (input.data.borrow(), self.data.borrow());
            let (xs, ws): (Vec<usize>, Vec<usize>) = (x.dimension().slice().to_vec(), w.dimension().slice().to_vec());
            check_conv_args(&xs, &ws, stride, dilation);
            check_groups_args(&xs, &ws, groups);
            conv_out_shape(&xs, &ws, stride, dilation)
        };
        let data = shared(shape, &self.device());
        let to_i32 = |v: &[usize]| v.iter().map(|&s| s as i32).collect::<Vec<_>>();
        let op = Convolution::new(input.data, self.data, data.clone(), to_i32(stride), to_i32(dilation), groups as i32);
        HipVar::node(data, Rc::new(op), self.history)
    }
}

impl<D> HipVar<D>
where
    D: 'static + Dimension + RemoveAxis,
{
    /// `convolution` followed by the broadcast `+ bias` of the `nn::Conv*` layers as ONE forward node (`nk_conv_bias_fwd`: the
    /// bias in the epilogue that writes the output).  `bias` has the layer's shape `(out_channels, 1, ..)`.
    pub fn convolution_bias<B>(mut self, input: HipVar<D>, bias: HipVar<B>, stride: &[usize], dilation: &[usize], groups: usize) -> HipVar<D>
    where
        B: 'static + Dimension,
    {
        self.history.merge(input.history);
        self.history.merge(bias.history);
        let shape: D = {
            let (x, w) = (input.data.borrow(), self.data.borrow());
            let (xs, ws): (Vec<usize>, Vec<usize>) = (x.dimension().slice().to_vec(), w.dimension().slice().to_vec());
            check_conv_args(&xs, &ws, stride, dilation);
            check_groups_args(&xs, &ws, groups);
            conv_out_shape(&xs, &ws, stride, dilation)
        };
        let data = shared(shape, &self.device());
        let to_i32 = |v: &[usize]| v.iter().map(|&s| s as i32).collect::<Vec<_>>();
        let op = ConvolutionBias::new(input.data, self.data, bias.data, data.clone(), to_i32(stride), to_i32(dilation), groups as i32);
        HipVar::node(data, Rc::new(op), self.history)
    }
}

impl HipVar<Ix2> {
    /// `Var::mm` (`var.rs:1034-1061`).
    pub fn mm(mut self, rhs: HipVar<Ix2>) -> HipVar<Ix2> {
        self.history.merge(rhs.history);
        let (n, o) = (self.data.borrow().dimension()[0], rhs.data.borrow().dimension()[1]);
        let data = shared(ndarray::Dim([n, o]), &self.device());
        let op = MatrixMatrixMul::new(self.data, rhs.data, data.clone());
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// `Var::mm_t` (`var.rs:1065-1094`).
    pub fn mm_t(mut self, rhs: HipVar<Ix2>) -> HipVar<Ix2> {
        self.history.merge(rhs.history);
        let (n, o) = (self.data.borrow().dimension()[0], rhs.data.borrow().dimension()[0]);
        let data = shared(ndarray::Dim([n, o]), &self.device());
        let op = MatrixMatrixMulT::new(self.data, rhs.data, data.clone());
        HipVar::node(data, Rc::new(op), self.history)
    }
}

impl<D> HipVar<D>
where
    D: 'static + Dimension + RemoveAxis,
{
    /// Cross entropy of class logits (ours: the reference stops at `nll`; semantics in `include/neuronika_hip.h`): `self` is
    /// `(minibatch, C, d1..dk)`, `target` `(minibatch, d1..dk)` holds class ids as f32 (read as the NLL targets are).  ONE forward node
    /// (`nk_cross_entropy_fwd`): no log-probability tensor.  Ids `>= C` and ids equal to `ignore_index` are inactive; `Mean` divides by
    /// the number of active positions.
    pub fn cross_entropy(self, target: HipVar<D::Smaller>, reduction: Reduction, ignore_index: Option<usize>, label_smoothing: f64) -> HipVar<Ix0> {
        self.cross_entropy_with_lse(target, reduction, ignore_index, label_smoothing).0
    }

    /// The node and the per-position `lse` it owns (what the backward entry reads).
    pub(crate) fn cross_entropy_with_lse(mut self, target: HipVar<D::Smaller>, reduction: Reduction, ignore_index: Option<usize>,
                                         label_smoothing: f64) -> (HipVar<Ix0>, Shared<HipArray<D::Smaller>>) {
        assert!((0. ..1.).contains(&label_smoothing), "cross_entropy: label_smoothing must be in [0, 1)");
        let dim = self.data.borrow().dimension();
        assert!(dim.ndim() >= 2, "cross_entropy: input of shape (minibatch, C, ...) expected");
        assert!(dim.remove_axis(Axis(1)) == target.data.borrow().dimension(), "cross_entropy: target must have shape (minibatch, d1, ..., dk)");
        self.history.merge(target.history);
        let lse = shared(dim.remove_axis(Axis(1)), &self.device());
        let data = shared(ndarray::Dim(()), &self.device());
        let op = CrossEntropy::new(self.data, target.data, lse.clone(), data.clone(), reduction, ignore_index.map_or(-1, |i| i as i64), label_smoothing);
        (HipVar::node(data, Rc::new(op), self.history), lse)
    }
}

impl HipVar<Ix2> {
    /// Embedding (ours: the reference has none; semantics in `include/neuronika_hip.h`): `self` is the `(V, D)` table, `indices` holds
    /// ids as f32 (read as the NLL targets are) in any dimension `E`; the result has the shape of `indices` plus a last axis `D`.
    pub fn embedding<E: 'static + Dimension>(mut self, indices: HipVar<E>) -> HipVar<E::Larger> {
        self.history.merge(indices.history);
        let d = self.data.borrow().dimension()[1];
        let idim = indices.data.borrow().dimension();
        let mut dim = idim.insert_axis(Axis(idim.ndim()));
        dim.slice_mut()[idim.ndim()] = d;
        let data = shared(dim, &self.device());
        let op = Embedding::new(self.data, indices.data, data.clone());
        HipVar::node(data, Rc::new(op), self.history)
    }
}

/// Device storage of one causal attention layer's keys and values for incremental decoding (ours; layout in
/// `include/neuronika_hip.h`): `(batch, heads, capacity, dh)` each, head-major, plus the scratch of the split-KV kernels, sized
/// for one new row per sample and regrown when a longer slice first arrives.  The lengths are the caller's
/// (`neuronika_nn::hip::KvCache`).  `rolling` (`new_rolling`): a ring for a sliding-window layer - position `p` lives at slot
/// `p % capacity` and the lengths may pass the capacity.
pub struct KvBuffers {
    pub(crate) keys: Shared<HipArray<Ix4>>,
    pub(crate) values: Shared<HipArray<Ix4>>,
    workspace: RefCell<Shared<HipArray<Ix1>>>,
    workspace_rows: Cell<usize>,
    workspace_heads: Cell<usize>, // query heads the scratch is sized for: more than `heads` once a grouped-query layer has used it
    workspace_window: Cell<usize>, // the widest window the scratch is sized for (0: none yet)
    geometry: (usize, usize, usize, usize), // batch, heads (kv heads of a grouped-query layer), capacity, dh
    rolling: bool,
}

impl KvBuffers {
    pub fn new(batch: usize, heads: usize, dh: usize, capacity: usize, device: &Device) -> Self {
        Self::build(batch, heads, dh, capacity, false, device)
    }

    /// `new` as a ring: position `p` at slot `p % capacity`.
    pub fn new_rolling(batch: usize, heads: usize, dh: usize, capacity: usize, device: &Device) -> Self {
        Self::build(batch, heads, dh, capacity, true, device)
    }

    fn build(batch: usize, heads: usize, dh: usize, capacity: usize, rolling: bool, device: &Device) -> Self {
        assert!(batch > 0 && heads > 0 && dh > 0 && capacity > 0, "KvBuffers: batch, heads, dh and capacity must be positive");
        let dim = ndarray::Dim([batch, heads, capacity, dh]);
        Self { keys: shared(dim, device), values: shared(dim, device),
               workspace: RefCell::new(shared(ndarray::Dim([decode_workspace(batch, 1, heads, dh, capacity)]), device)),
               workspace_rows: Cell::new(1), workspace_heads: Cell::new(heads), workspace_window: Cell::new(0),
               geometry: (batch, heads, capacity, dh), rolling }
    }

    pub fn rolling(&self) -> bool {
        self.rolling
    }

    /// `(batch, heads, capacity, dh)`
    pub fn geometry(&self) -> (usize, usize, usize, usize) {
        self.geometry
    }

    /// Keys per partial problem at this head size: where a length crosses into the next chunk.
    pub fn chunk(&self) -> usize {
        decode_chunk(self.geometry.3)
    }

    /// `window > 0`: also at least `nk_attention_decode_window_workspace` floats - a window that straddles one more chunk seam
    /// than the capacity has chunks needs a chunk more than the capacity-sized scratch.
    fn workspace_for(&self, rows: usize, query_heads: usize, window: usize, device: &Device) -> Shared<HipArray<Ix1>> {
        let window = window.min(self.geometry.2);
        if rows > self.workspace_rows.get() || query_heads > self.workspace_heads.get() || window > self.workspace_window.get() {
            let (batch, _, capacity, dh) = self.geometry;
            let (rows, heads) = (rows.max(self.workspace_rows.get()), query_heads.max(self.workspace_heads.get()));
            let window = window.max(self.workspace_window.get());
            let mut floats = decode_workspace(batch, rows, heads, dh, capacity);
            if window > 0 {
                floats = floats.max(decode_window_workspace(batch, rows, heads, dh, window));
            }
            *self.workspace.borrow_mut() = shared(ndarray::Dim([floats]), device);
            self.workspace_rows.set(rows);
            self.workspace_heads.set(heads);
            self.workspace_window.set(window);
        }
        self.workspace.borrow().clone()
    }
}

impl HipVar<Ix2> {
    /// One step of incremental decoding: `self` is the `(batch*rows, 3*heads*dh)` packed projection of the NEW positions; its key
    /// and value blocks are appended to `buffers` at `start[b] + t` and every new row attends to the keys `< start[b] + t + 1` of
    /// its sample (`nk_kv_cache_append`, `nk_attention_decode_fwd`).  `start`: each sample's length before the step, captured
    /// here.  Output `(batch*rows, query_heads*dh)`, no gradient.  `query_heads`: the heads of Q - the buffers' head count for plain
    /// multi-head attention, a multiple of it for a grouped-query layer, whose packed projection is `(rows, (query_heads +
    /// 2*heads)*dh)` and whose step runs `nk_attention_decode_gqa_fwd`.  `window`: 0 = every key below the row's position; `W > 0` =
    /// the keys `max(0, n - W) .. n - 1` through `nk_attention_decode_window_fwd`, on linear buffers or rolling ones
    /// (`KvBuffers::new_rolling`: `nk_kv_cache_append_ring`, `start` may pass the capacity, `W + rows - 1 <= capacity`).
    pub fn packed_decode_attention(self, buffers: &KvBuffers, query_heads: usize, start: &[usize], scale: f32, window: usize) -> HipVar<Ix2> {
        let device = self.device();
        let (batch, heads, capacity, dh) = buffers.geometry();
        let total = self.data.borrow().dimension()[0];
        assert!(start.len() == batch && total % batch == 0 && total > 0, "packed_decode_attention: rows must be a positive multiple of the batch");
        assert!(query_heads >= heads && query_heads % heads == 0, "packed_decode_attention: query_heads must be a multiple of the cache's heads");
        assert!(self.data.borrow().dimension()[1] == (query_heads + 2 * heads) * dh,
                "packed_decode_attention: the input must be (rows, (query_heads + 2 * heads) * dh)");
        let rows = total / batch;
        if buffers.rolling() {
            assert!(window > 0, "packed_decode_attention: rolling buffers keep the last positions only: they need a window");
            assert!(window + rows - 1 <= capacity,
                    "packed_decode_attention: rolling buffers of {} slots cannot hold a window of {} keys and {} new rows (window + rows - 1 <= capacity): chunk the prompt",
                    capacity, window, rows);
            assert!(start.iter().all(|&s| s + rows < (1usize << 31) - 1024), "packed_decode_attention: positions must stay below 2^31 - 1024");
        } else {
            assert!(start.iter().all(|&s| s + rows <= capacity), "packed_decode_attention: the step exceeds the capacity of the cache");
        }
        let cells: Vec<f32> = start.iter().map(|&s| f32::from_bits(s as u32)).collect();
        let start = HipArray::from_slice(&cells, ndarray::Dim([batch]), device.clone());
        let geometry = Heads { batch: batch as i32, seq: rows as i32, heads: heads as i32, dh: dh as i32 };
        let data = shared(ndarray::Dim([total, query_heads * dh]), &device);
        let op = PackedDecodeAttention::new(geometry, query_heads as i32, capacity as i32, window.min(i32::MAX as usize) as i32, buffers.rolling(), self.data,
                                            buffers.keys.clone(), buffers.values.clone(), start,
                                            buffers.workspace_for(rows, query_heads, window, &device), data.clone(), scale);
        HipVar::node(data, Rc::new(op), self.history)
    }
}

/// Device storage of a PAGED key / value cache (layout at `nk_attention_decode_paged_fwd` in `include/neuronika_hip.h`): the two
/// pools `(num_pages, heads, page, dh)`, never initialised, and the decode scratch, regrown when a larger step first arrives.  The
/// table and the lengths are the caller's (`neuronika_nn::hip::PagedKvCache`).
pub struct PagedBuffers {
    pub(crate) keys: Shared<HipArray<Ix4>>,
    pub(crate) values: Shared<HipArray<Ix4>>,
    workspace: RefCell<Option<Shared<HipArray<Ix1>>>>,
    workspace_floats: Cell<usize>,
    geometry: (usize, usize, usize, usize, usize), // num_pages, heads (kv heads), page, dh, max_pages
}

impl PagedBuffers {
    pub fn new(num_pages: usize, page: usize, heads: usize, dh: usize, max_pages: usize, device: &Device) -> Self {
        assert!(num_pages > 0 && heads > 0 && dh > 0 && max_pages > 0, "PagedBuffers: num_pages, heads, dh and max_pages must be positive");
        assert!(page >= 16 && page.is_power_of_two(), "PagedBuffers: page must be a power of two and at least 16");
        assert!(num_pages * heads * page * dh <= i32::MAX as usize, "PagedBuffers: one pool must fit 31 bits of elements");
        let dim = ndarray::Dim([num_pages, heads, page, dh]);
        Self { keys: shared(dim, device), values: shared(dim, device), workspace: RefCell::new(None), workspace_floats: Cell::new(0),
               geometry: (num_pages, heads, page, dh, max_pages) }
    }

    /// `(num_pages, heads, page, dh, max_pages)`
    pub fn geometry(&self) -> (usize, usize, usize, usize, usize) {
        self.geometry
    }

    fn workspace_for(&self, batch: usize, rows: usize, query_heads: usize, window: usize, device: &Device) -> Shared<HipArray<Ix1>> {
        let (_, _, page, dh, max_pages) = self.geometry;
        let floats = decode_paged_workspace(batch, rows, query_heads, dh, max_pages, page, window);
        if floats > self.workspace_floats.get() || self.workspace.borrow().is_none() {
            *self.workspace.borrow_mut() = Some(shared(ndarray::Dim([floats]), device));
            self.workspace_floats.set(floats);
        }
        self.workspace.borrow().as_ref().unwrap().clone()
    }
}

impl HipVar<Ix2> {
    /// `packed_decode_attention` over a paged cache: `start[b]` is sequence b's length before the step, `table` its `max_pages` page
    /// ids per sequence (`-1`: none) AFTER the step's pages were reserved, `copies` the (old, new) page pairs to copy first.  One
    /// upload; `nk_kv_pages_copy`, `nk_kv_pages_append`, `nk_attention_decode_paged_fwd` in the node's forward.
    #[allow(clippy::too_many_arguments)]
    pub fn packed_paged_decode_attention(self, buffers: &PagedBuffers, query_heads: usize, start: &[usize], table: &[i32], copies: &[(usize, usize)],
                                         scale: f32, window: usize) -> HipVar<Ix2> {
        let device = self.device();
        let (num_pages, heads, page, dh, max_pages) = buffers.geometry();
        let batch = start.len();
        let total = self.data.borrow().dimension()[0];
        assert!(batch > 0 && total % batch == 0 && total > 0, "packed_paged_decode_attention: rows must be a positive multiple of the batch");
        assert!(table.len() == batch * max_pages, "packed_paged_decode_attention: one table row of max_pages ids per sequence");
        assert!(query_heads >= heads && query_heads % heads == 0, "packed_paged_decode_attention: query_heads must be a multiple of the cache's heads");
        assert!(self.data.borrow().dimension()[1] == (query_heads + 2 * heads) * dh,
                "packed_paged_decode_attention: the input must be (rows, (query_heads + 2 * heads) * dh)");
        let rows = total / batch;
        assert!(start.iter().all(|&s| s + rows <= max_pages * page), "packed_paged_decode_attention: the step exceeds max_pages * page");
        let mut cells: Vec<f32> = start.iter().map(|&s| f32::from_bits(s as u32)).collect();
        cells.extend(table.iter().map(|&p| f32::from_bits(p as u32)));
        cells.extend(copies.iter().map(|&(old, _)| f32::from_bits(old as u32)));
        cells.extend(copies.iter().map(|&(_, new)| f32::from_bits(new as u32)));
        let image = HipArray::from_slice(&cells, ndarray::Dim([cells.len()]), device.clone());
        let geometry = Heads { batch: batch as i32, seq: rows as i32, heads: heads as i32, dh: dh as i32 };
        let data = shared(ndarray::Dim([total, query_heads * dh]), &device);
        let op = PagedDecodeAttention::new(geometry, query_heads as i32, page as i32, max_pages as i32, num_pages as i32, copies.len() as i32,
                                           window.min(i32::MAX as usize) as i32, self.data, buffers.keys.clone(), buffers.values.clone(), image,
                                           buffers.workspace_for(batch, rows, query_heads, window, &device), data.clone(), scale);
        HipVar::node(data, Rc::new(op), self.history)
    }
}

/// The settings and the offset counter of a token sampler (ours; semantics at `nk_sample_fwd` in `include/neuronika_hip.h`): greedy at
/// `temperature == 0`, else temperature, top-k (`0`: off) and top-p (`1.`: off) and one Philox draw per row at `(seed, offset)`.
/// Every execution of a node built from it advances the shared `offset` (`neuronika_nn::hip::Sampler`).
#[derive(Clone)]
pub struct SamplerState {
    pub temperature: f32,
    pub top_k: usize,
    pub top_p: f32,
    pub seed: u64,
    pub offset: Rc<Cell<u64>>,
}

impl SamplerState {
    pub fn new(temperature: f32, top_k: usize, top_p: f32, seed: u64) -> Self {
        assert!(temperature >= 0. && temperature.is_finite(), "SamplerState: temperature must be finite and not negative");
        assert!(top_p > 0., "SamplerState: top_p must be positive");
        Self { temperature, top_k, top_p, seed, offset: Rc::new(Cell::new(0)) }
    }

    /// The largest vocabulary whose row the kernel keeps in LDS; longer rows are re-read from memory by the later passes.
    pub fn stage_limit() -> usize {
        sample_stage_limit()
    }
}

/// A weight-only quantised `(out, in)` weight with its optional bias (ours; format at `nk_quant_linear_*` in
/// `include/neuronika_hip.h`): what `HipVar::quant_linear` multiplies by.  Built from an f32 weight on the device; the f32 weight
/// is left as it is.  Inference only: no gradient, no parameters for an optimizer, no serde.
#[derive(Clone)]
pub struct QuantLinearState {
    weight: QuantWeight,
    bias: Option<Shared<HipArray<Ix1>>>,
}

impl QuantLinearState {
    /// `bits` 8 or 4; `group` 32, 64, 128 or 0 (one scale per row); `in` a multiple of 32 and of the group.
    pub fn new(weight: &HipVar<Ix2>, bias: Option<&HipVar<Ix1>>, bits: usize, group: usize) -> Self {
        let dim = weight.data.borrow().dimension();
        let (words, scales) = QuantWeight::sizes(dim[0], dim[1], bits as i32, group as i32)
            .expect("QuantLinearState: bits must be 8 or 4, group 32, 64, 128 or 0, and the input extent a multiple of 32 and of the group");
        let device = weight.device();
        let q = QuantWeight { qweight: shared(ndarray::Dim([words]), &device), scales: shared(ndarray::Dim([scales]), &device),
                              out_features: dim[0], in_features: dim[1], bits: bits as i32, group: group as i32 };
        q.pack(&weight.data.borrow());
        if let Some(b) = bias {
            assert!(b.data.borrow().dimension()[0] == dim[0], "QuantLinearState: the bias must have one entry per output");
        }
        Self { weight: q, bias: bias.map(|b| b.data.clone()) }
    }

    /// The `(out, in)` values `float(q) * scale` as a leaf.
    pub fn dequantize(&self) -> HipVar<Ix2> {
        let device = self.weight.qweight.borrow().device().clone();
        let data = shared(ndarray::Dim([self.weight.out_features, self.weight.in_features]), &device);
        self.weight.unpack(&mut data.borrow_mut());
        HipVar { data, history: History::default() }
    }

    /// Rows of `x` up to which the forward takes the rows kernels by rule.
    pub fn rows_rule(&self) -> usize {
        quant_linear_rows_rule(self.weight.bits)
    }
}

impl HipVar<Ix2> {
    /// `(rows, in) -> (rows, out)` on the packed integer weights of `layer`: ONE node (`nk_quant_linear_fwd`), no gradient.
    pub fn quant_linear(self, layer: &QuantLinearState) -> HipVar<Ix2> {
        let dim = self.data.borrow().dimension();
        assert!(dim[1] == layer.weight.in_features, "quant_linear: the input must be (rows, {})", layer.weight.in_features);
        let data = shared(ndarray::Dim([dim[0], layer.weight.out_features]), &self.device());
        let op = QuantLinear::new(layer.weight.clone(), layer.bias.clone(), dim[0], self.data, data.clone());
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// The next token of every sample of `(batch * rows, vocab)` logits: the `(batch,)` ids, as f32, drawn from the LAST row of each
    /// sample - what `embedding` takes.  ONE node (`nk_sample_fwd`), no gradient.
    pub fn sample(self, sampler: &SamplerState, batch: usize) -> HipVar<Ix1> {
        let dim = self.data.borrow().dimension();
        assert!(batch > 0 && dim[0] > 0 && dim[0] % batch == 0, "sample: rows must be a positive multiple of the batch");
        assert!(dim[1] > 0 && dim[1] <= 1 << 20, "sample: the vocabulary must be in [1, 2^20]");
        let data = shared(ndarray::Dim([batch]), &self.device());
        let params = SampleParams { temperature: sampler.temperature, top_k: sampler.top_k.min(i32::MAX as usize) as i32, top_p: sampler.top_p,
                                    seed: sampler.seed };
        let op = Sample::new(params, sampler.offset.clone(), batch as i32, dim[0] / batch, dim[1], self.data, data.clone());
        HipVar::node(data, Rc::new(op), self.history)
    }
}

/// The table of a rotary position embedding (ours; semantics at `nk_rope_fwd` in `include/neuronika_hip.h`): `(max_pos, rot / 2, 2)`
/// f32 `(cos, sin)` of `p * base^(-2j/rot)`, made in f64 by `nk_rope_table` at construction.  The first `rot` columns of every head
/// are rotated (even, `2 <= rot <= head_dim`), pairs `(j, j + rot/2)` or, `interleaved`, `(2j, 2j+1)`.  Nothing trainable; shared by
/// the layers of a model (`neuronika_nn::hip::RotaryEmbedding`).
pub struct RotaryTable {
    table: Shared<HipArray<Ix3>>,
    head_dim: usize,
    max_pos: usize,
    rot: usize,
    interleaved: bool,
}

impl RotaryTable {
    pub fn new(head_dim: usize, max_pos: usize, base: f64, rot: usize, interleaved: bool, device: &Device) -> Self {
        assert!(head_dim > 0 && max_pos > 0, "RotaryTable: head_dim and max_pos must be positive");
        assert!(rot >= 2 && rot <= head_dim && rot % 2 == 0, "RotaryTable: rot must be even and in [2, head_dim]");
        assert!(base > 0. && base.is_finite(), "RotaryTable: base must be positive and finite");
        Self { table: Rc::new(RefCell::new(rope_table(max_pos, rot, base, device))), head_dim, max_pos, rot, interleaved }
    }

    pub fn head_dim(&self) -> usize {
        self.head_dim
    }

    pub fn max_pos(&self) -> usize {
        self.max_pos
    }

    pub fn rot(&self) -> usize {
        self.rot
    }

    pub fn interleaved(&self) -> bool {
        self.interleaved
    }

    /// The launch geometry of `heads` heads per row of stride `ld` over `batch * rows` rows, after the shape checks.
    fn geometry(&self, total: usize, width: usize, batch: usize, heads: usize, ld: usize) -> RopeGeometry {
        assert!(batch > 0 && total > 0 && total % batch == 0, "rope: rows must be a positive multiple of the batch");
        assert!(heads > 0 && heads * self.head_dim <= width && width == ld, "rope: the input must hold heads * head_dim columns");
        RopeGeometry { batch: batch as i32, rows: (total / batch) as i32, heads: heads as i32, dh: self.head_dim as i32, rot: self.rot as i32,
                       max_pos: self.max_pos as i32, interleaved: self.interleaved as i32, ld: ld as i32 }
    }
}

impl HipVar<Ix2> {
    /// Rotary position embedding of a `(batch*rows, heads*head_dim)` value at positions `0 .. rows - 1`: ONE node (`nk_rope_fwd`).
    pub fn rope(self, rotary: &RotaryTable, batch: usize, heads: usize) -> HipVar<Ix2> {
        let dim = self.data.borrow().dimension();
        assert!(dim[1] == heads * rotary.head_dim, "rope: the input must be (batch*rows, heads*head_dim)");
        assert!(dim[0] / batch.max(1) <= rotary.max_pos, "rope: the positions exceed the table");
        let geometry = rotary.geometry(dim[0], dim[1], batch, heads, dim[1]);
        let data = shared(dim, &self.device());
        let op = Rope::new(geometry, rotary.table.clone(), self.data, data.clone());
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// The rotation IN PLACE over the first `heads * head_dim` columns of `self` - `heads = 2 * H` on a `(rows, 3 * H * head_dim)`
    /// packed projection rotates its Q|K blocks and leaves V alone - at positions `start[b] + t` (`None`: `t`).  The result shares
    /// its buffer with `self`; ONE node right behind the one that wrote the buffer.
    pub fn rope_in_place(self, rotary: &RotaryTable, batch: usize, heads: usize, start: Option<&[usize]>) -> HipVar<Ix2> {
        let dim = self.data.borrow().dimension();
        let geometry = rotary.geometry(dim[0], dim[1], batch, heads, dim[1]);
        let device = self.device();
        let start = start.map(|s| {
            assert!(s.len() == batch && s.iter().all(|&l| l + dim[0] / batch <= rotary.max_pos), "rope_in_place: the positions exceed the table");
            let cells: Vec<f32> = s.iter().map(|&l| f32::from_bits(l as u32)).collect();
            HipArray::from_slice(&cells, ndarray::Dim([batch]), device.clone())
        });
        assert!(start.is_some() || dim[0] / batch <= rotary.max_pos, "rope_in_place: the positions exceed the table");
        let data = self.data.clone();
        let op = RopeInPlace::new(geometry, rotary.table.clone(), self.data, start);
        HipVar::node(data, Rc::new(op), self.history)
    }
}

impl HipVarDiff<Ix2> {
    /// `HipVar::rope` with its backward entry (`RopeBackward`: `dx += R^T g`, the same kernel with the sign of the sine flipped).
    pub fn rope(self, rotary: &RotaryTable, batch: usize, heads: usize) -> HipVarDiff<Ix2> {
        let dim = self.var.data.borrow().dimension();
        let geometry = rotary.geometry(dim[0], dim[1], batch, heads, dim[1]);
        let var = self.var.rope(rotary, batch, heads);
        let grad = Rc::new(Gradient::hip_zeros(dim, var.device()));
        let op: Rc<dyn Backward> = Rc::new(RopeBackward::new(geometry, rotary.table.clone(), self.grad, grad.clone()));
        HipVarDiff::node(var, grad.clone(), (op, grad), self.history)
    }

    /// `HipVar::rope_in_place` at positions `0 .. rows - 1` with its backward entry: the inverse rotation in place in the gradient
    /// `self` already owns (`RopeInPlaceBackward`), between the consumer that writes it and the producer's backward that reads it.
    /// The buffer must have ONE consumer.
    pub fn rope_in_place(self, rotary: &RotaryTable, batch: usize, heads: usize) -> HipVarDiff<Ix2> {
        let dim = self.var.data.borrow().dimension();
        let geometry = rotary.geometry(dim[0], dim[1], batch, heads, dim[1]);
        let var = self.var.rope_in_place(rotary, batch, heads, None);
        let grad = self.grad;
        let op: Rc<dyn Backward> = Rc::new(RopeInPlaceBackward::new(geometry, rotary.table.clone(), grad.clone()));
        HipVarDiff::node(var, grad.clone(), (op, grad), self.history)
    }
}

fn repeat_kv_geometry(dim: ndarray::Ix2, groups: usize, head_dim: usize) -> RepeatKvGeometry {
    assert!(groups > 0 && head_dim > 0 && dim[0] > 0 && dim[1] > 0 && dim[1] % head_dim == 0,
            "repeat_kv: the input must be (rows, kv_heads*head_dim)");
    assert!(dim[0] * dim[1] * groups <= i32::MAX as usize, "repeat_kv: the output must fit 31 bits");
    RepeatKvGeometry { rows: dim[0] as i32, kv_heads: (dim[1] / head_dim) as i32, groups: groups as i32, dh: head_dim as i32 }
}

impl HipVar<Ix2> {
    /// Grouped-query attention: every head of a `(rows, kv_heads*head_dim)` value written `groups` times, `(rows,
    /// kv_heads*groups*head_dim)` - what the attention core reads as the keys / values of its query heads.  ONE node
    /// (`nk_repeat_kv_fwd`), a bit-exact copy.
    pub fn repeat_kv(self, groups: usize, head_dim: usize) -> HipVar<Ix2> {
        let dim = self.data.borrow().dimension();
        let geometry = repeat_kv_geometry(dim, groups, head_dim);
        let data = shared(ndarray::Dim([dim[0], dim[1] * groups]), &self.device());
        let op = RepeatKv::new(geometry, self.data, data.clone());
        HipVar::node(data, Rc::new(op), self.history)
    }
}

impl HipVarDiff<Ix2> {
    /// `HipVar::repeat_kv` with its backward entry (`RepeatKvBackward`: the gradients of the copies summed in ascending order).
    pub fn repeat_kv(self, groups: usize, head_dim: usize) -> HipVarDiff<Ix2> {
        let dim = self.var.data.borrow().dimension();
        let geometry = repeat_kv_geometry(dim, groups, head_dim);
        let var = self.var.repeat_kv(groups, head_dim);
        let grad = Rc::new(Gradient::hip_zeros(ndarray::Dim([dim[0], dim[1] * groups]), var.device()));
        let op: Rc<dyn Backward> = Rc::new(RepeatKvBackward::new(geometry, self.grad, grad.clone()));
        HipVarDiff::node(var, grad.clone(), (op, grad), self.history)
    }
}

impl HipVar<Ix2> {
    /// `Var::mm_t(VarDiff)` (`var.rs:1081-1094`): only the right operand is differentiable, so only
    /// `MatrixMatrixMulTBackwardRight` goes on the tape - the input layer of C4, whose input-gradient GEMM the reference never
    /// runs either.
    pub fn mm_t_diff(self, rhs: HipVarDiff<Ix2>) -> HipVarDiff<Ix2> {
        let left_data = self.data.clone();
        let var = self.mm_t(rhs.var);
        let grad = Rc::new(Gradient::hip_zeros(var.data.borrow().dimension(), var.device()));
        let op: Rc<dyn Backward> = Rc::new(MatrixMatrixMulTBackwardRight::new(left_data, rhs.grad.clone(), grad.clone()));
        HipVarDiff::node(var, grad.clone(), (op, grad), rhs.history)
    }
}

impl HipVar<Ix2> {
    /// `nn::Linear::forward` (`neuronika-nn/src/lib.rs:441-447`: `input.mm_t(weight) + bias`) as ONE forward node -
    /// `nk_linear_fwd`, the bias in the GEMM epilogue - and, with `relu`, the `.relu()` that follows it in the reference's
    /// words (`vardiff.rs:282-288`) in the same epilogue (`nk_linear_relu_fwd`).  Bit-identical to the separate nodes.
    pub fn linear(mut self, weight: HipVar<Ix2>, bias: HipVar<Ix1>, relu: bool) -> HipVar<Ix2> {
        self.history.merge(weight.history);
        self.history.merge(bias.history);
        let (n, o) = (self.data.borrow().dimension()[0], weight.data.borrow().dimension()[0]);
        let data = shared(ndarray::Dim([n, o]), &self.device());
        let op = Linear::new(self.data, weight.data, bias.data, data.clone(), relu);
        HipVar::node(data, Rc::new(op), self.history)
    }

    /// The same layer over an input WITHOUT gradient (the first layer of C4: its input-gradient GEMM is never issued, as in
    /// `Var::mm_t(VarDiff)`, `var.rs:1081-1094`).
    pub fn linear_diff(self, weight: HipVarDiff<Ix2>, bias: HipVarDiff<Ix1>, relu: bool) -> HipVarDiff<Ix2> {
        let (input_data, weight_data) = (self.data.clone(), weight.var.data.clone());
        let mut history = weight.history;
        history.merge(bias.history);
        let var = self.linear(weight.var, bias.var, relu);
        let grad = Rc::new(Gradient::hip_zeros(var.data.borrow().dimension(), var.device()));
        let mask = if relu { Some(Rc::new(ReluMask::new(var.data.clone()))) } else { None };
        let op: Rc<dyn Backward> = Rc::new(LinearBackward::new(input_data, weight_data, mask.clone(), None, None, weight.grad.clone(),
                                                               bias.grad.clone(), grad.clone()));
        let mut out = HipVarDiff::node(var, grad.clone(), (op, grad), history);
        out.relu_mask = mask;
        out
    }
}

/// A differentiable variable with data and gradient in HBM (`VarDiff<D>`, `vardiff.rs:35-42`).
pub struct HipVarDiff<D>
where
    D: Dimension,
{
    pub(crate) var: HipVar<D>,
    pub(crate) grad: Rc<Gradient<HipArray<D>, D>>,
    pub(crate) history: Bwd,
    /// Set on the output of a fused Linear+ReLU node (`linear(.., relu = true)`): the mask record a following `linear` hands to
    /// its backward node, so that the input gradient can be written pre-masked (`nk_linear_bwd_input_relu`).
    pub(crate) relu_mask: Option<Rc<ReluMask>>,
}

impl<D: Dimension> Clone for HipVarDiff<D> {
    fn clone(&self) -> Self {
        Self { var: self.var.clone(), grad: self.grad.clone(), history: self.history.clone(), relu_mask: self.relu_mask.clone() }
    }
}

impl<D> HipVarDiff<D>
where
    D: 'static + Dimension,
{
    pub(crate) fn node(var: HipVar<D>, grad: Rc<Gradient<HipArray<D>, D>>, op: (Rc<dyn Backward>, Rc<dyn NoGrad>), mut history: Bwd) -> Self {
        history.insert(Rc::as_ptr(&op.0) as *const () as usize, op);
        Self { var, grad, history, relu_mask: None }
    }

    /// The variable without its gradient: the same data and forward tape (inference paths such as
    /// `nn::MultiheadAttention::forward_step` run a parameter through nodes that keep nothing for a backward pass).
    pub fn detached(&self) -> HipVar<D> {
        self.var.clone()
    }

    fn new_grad<E: Dimension>(&self, dim: E) -> Rc<Gradient<HipArray<E>, E>> {
        Rc::new(Gradient::hip_zeros(dim, self.var.device()))
    }

    pub fn forward(&self) {
        self.var.forward();
    }

    /// `VarDiff::backward` (`vardiff.rs:125-141`): seed the root gradient, run the tape in reverse.  Launches are
    /// asynchronous.  The data-parallel step uses `backward_sync` below (overlapped exchange); calling
    /// `dp::GradientSync::all_reduce` after this plain `backward` is the serialised fallback.
    pub fn backward(&self, seed: f32) {
        debug_assert_eq!(self.var.history.len(), self.var.history.buffer_len(), "Perhaps you forgot to call .forward()?");
        self.grad.borrow_mut().fill(seed);
        let mut buffer = self.history.buffer_mut();
        if buffer.is_empty() {
            *buffer = self.history.to_vec();
        }
        Self::decide_premasking(&buffer);
        buffer.iter().rev().for_each(|(op, _)| op.backward());
    }

    /// Per pass, for every fused Linear+ReLU node on the tape: its output gradient may be stored PRE-MASKED (`(y > 0) *` applied
    /// in the writer's GEMM epilogue, no ReLU-backward kernel) iff every node that accumulates into that gradient can mask
    /// while storing (`Backward::premask_targets`); one plain writer (a second consumer of the activation) and the node masks
    /// a scratch copy instead.  The rule `VarDiff::run_backward` applies in this repository's C++ tape (`host/neuronika.cpp`).
    fn decide_premasking(buffer: &[(Rc<dyn Backward>, Rc<dyn NoGrad>)]) {
        for (op, _) in buffer.iter() {
            if let Some((id, mask)) = op.masked_gradient() {
                let writers = buffer.iter().filter(|(w, _)| w.targets().contains(&id));
                let mut all_mask = true;
                let mut any = false;
                for (w, _) in writers {
                    any = true;
                    all_mask &= w.premask_targets().contains(&id);
                }
                mask.premasked.set(any && all_mask);
            }
        }
    }

    /// The data-parallel form of `backward` (`vardiff.rs:125-141` with the exchange of `hip/dp.rs` inserted): seeds the root
    /// with `seed` (`1 / world` for mean semantics over the global batch), issues the tape in reverse and hands every
    /// registered parameter gradient to `sync` right after the LAST node that accumulates into it has been issued - its
    /// all-reduce then runs on the device's side stream underneath the remaining backward kernels.  Which node is the last
    /// writer is read off `Backward::targets` (`autograd_hip_ext.rs`), exactly as `VarDiff::run_backward` does in the C++
    /// tape of this repository (`host/neuronika.cpp`).  Call `sync.join()` before `Optimizer::step`.
    pub fn backward_sync(&self, seed: f32, sync: &mut GradientSync) {
        debug_assert_eq!(self.var.history.len(), self.var.history.buffer_len(), "Perhaps you forgot to call .forward()?");
        self.grad.borrow_mut().fill(seed);
        let mut buffer = self.history.buffer_mut();
        if buffer.is_empty() {
            *buffer = self.history.to_vec();
        }
        Self::decide_premasking(&buffer);
        // execution order is the reverse of the tape: the LAST writer of a gradient is the entry with the smallest index
        let mut last_writer: std::collections::HashMap<usize, usize> = std::collections::HashMap::new();
        for (index, (op, _)) in buffer.iter().enumerate() {
            for id in op.targets() {
                last_writer.entry(id).or_insert(index);
            }
        }
        for (index, (op, _)) in buffer.iter().enumerate().rev() {
            op.backward();
            let mut finished = op.targets();
            finished.sort_unstable();
            finished.dedup(); // `x * x` names the same gradient twice: one hand-over
            for id in finished {
                if last_writer[&id] == index {
                    if let Some(bucket) = sync.bucket_of(id) {
                        sync.grad_ready(bucket);
                    }
                }
            }
        }
    }

    /// `VarDiff::zero_grad` (`vardiff.rs:100-102`).
    /// Extents of the data, without touching the device.
    pub fn shape(&self) -> Vec<usize> {
        self.var.shape()
    }

    /// A differentiable leaf holding `array` (parameter construction: `zeros(..).requires_grad()` + `init::uniform` in the
    /// reference, `neuronika-nn/src/lib.rs:425-433`; here the values are drawn on the host and uploaded once).
    pub fn parameter(array: &ndarray::Array<f32, D>, device: Device) -> Self {
        HipVar::from_ndarray(array, device).requires_grad()
    }

    /// Registration record of this parameter for `dp::GradientSync::new`.
    pub fn sync_entry(&self) -> super::dp::SyncEntry {
        let mut grad = self.grad.borrow_mut();
        super::dp::SyncEntry { id: super::node::grad_id(&self.grad), ptr: grad.as_mut_ptr(), len: grad.len() }
    }

    pub fn zero_grad(&self) {
        self.grad.borrow_mut().fill(0.);
    }

    /// Host copy of the gradient (synchronises), `VarDiff::grad` (`vardiff.rs:144-150`).
    pub fn grad(&self) -> ndarray::Array<f32, D> {
        self.grad.borrow().as_ndarray()
    }

    /// `VarDiff::sum` (`vardiff.rs:238-245`).
    pub fn sum(self) -> HipVarDiff<Ix0> {
        let grad = self.new_grad(ndarray::Dim(()));
        let op = SumBackward::new(self.grad.clone(), grad.clone());
        let var = self.var.sum();
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }

    /// `VarDiff::mean` (`vardiff.rs:247-253`).
    pub fn mean(self) -> HipVarDiff<Ix0> {
        let grad = self.new_grad(ndarray::Dim(()));
        let op = MeanBackward::new(self.grad.clone(), grad.clone());
        let var = self.var.mean();
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }

    /// `VarDiff::relu` (`vardiff.rs:282-288`).
    pub fn relu(self) -> HipVarDiff<D> {
        let grad = self.new_grad(self.grad.shape());
        let op = ReLUBackward::new(self.grad.clone(), self.var.data.clone(), grad.clone());
        let var = self.var.relu();
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }

    /// GELU in the erfc form: ONE forward node and ONE backward entry, which keeps the input and recomputes from it.
    pub fn gelu(self) -> HipVarDiff<D> {
        self.activation(Gate::Gelu)
    }

    /// GELU in the tanh form: ONE forward node and ONE backward entry.
    pub fn gelu_tanh(self) -> HipVarDiff<D> {
        self.activation(Gate::GeluTanh)
    }

    /// SiLU: ONE forward node and ONE backward entry.
    pub fn silu(self) -> HipVarDiff<D> {
        self.activation(Gate::Silu)
    }

    fn activation(self, act: Gate) -> HipVarDiff<D> {
        let grad = self.new_grad(self.grad.shape());
        let op = ActivationBackward::new(self.grad.clone(), self.var.data.clone(), grad.clone(), act as i32);
        let var = self.var.activation(act);
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }

    /// `a * gate(b)` over the two halves of the last axis: ONE forward node and ONE backward entry (`GluBackward`).
    pub fn glu(self, gate: Gate) -> HipVarDiff<D> {
        let mut dim = self.var.data.borrow().dimension();
        let last = dim.ndim().checked_sub(1).expect("glu: a scalar has no last axis");
        assert!(dim[last] % 2 == 0 && dim[last] > 0, "glu: the last axis must have an even extent");
        dim[last] /= 2;
        let half = dim[last];
        let grad = self.new_grad(dim);
        let op = GluBackward::new(self.grad.clone(), self.var.data.clone(), grad.clone(), gate as i32, half);
        let var = self.var.glu(gate);
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }

    /// `VarDiff::softmax` (`vardiff.rs:359-365`).
    pub fn softmax(self, axis: usize) -> HipVarDiff<D> {
        let grad = self.new_grad(self.grad.shape());
        let var = self.var.softmax(axis);
        let op = SoftmaxBackward::new(self.grad.clone(), var.data.clone(), grad.clone(), axis);
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }

    /// Layer normalisation with differentiable parameters: ONE forward node and ONE backward entry writing the gradients of
    /// `self`, `gamma` and `beta` (`LayerNormBackward`).
    pub fn layer_norm<E: 'static + Dimension>(mut self, gamma: HipVarDiff<E>, beta: HipVarDiff<E>, eps: f64) -> HipVarDiff<D> {
        self.history.merge(gamma.history);
        self.history.merge(beta.history);
        let (input_data, gamma_data) = (self.var.data.clone(), gamma.var.data.clone());
        let rows = input_data.borrow().len() / gamma_data.borrow().len().max(1);
        let stats = shared(Ix2(rows, 2), &self.var.device());
        let grad = self.new_grad(self.grad.shape());
        let var = self.var.layer_norm_with_stats(gamma.var, beta.var, eps, Some(stats.clone()));
        let op: Rc<dyn Backward> = Rc::new(LayerNormBackward::new(input_data, gamma_data, stats, Some(self.grad.clone()), gamma.grad.clone(),
                                                                   beta.grad.clone(), grad.clone()));
        HipVarDiff::node(var, grad.clone(), (op, grad), self.history)
    }

    /// RMS normalisation with a differentiable weight: ONE forward node and ONE backward entry writing the gradients of `self`
    /// and `gamma` (`RmsNormBackward`).
    pub fn rms_norm<E: 'static + Dimension>(mut self, gamma: HipVarDiff<E>, eps: f64) -> HipVarDiff<D> {
        self.history.merge(gamma.history);
        let (input_data, gamma_data) = (self.var.data.clone(), gamma.var.data.clone());
        let rows = input_data.borrow().len() / gamma_data.borrow().len().max(1);
        let stats = shared(Ix1(rows), &self.var.device());
        let grad = self.new_grad(self.grad.shape());
        let var = self.var.rms_norm_with_stats(gamma.var, eps, Some(stats.clone()));
        let op: Rc<dyn Backward> = Rc::new(RmsNormBackward::new(input_data, gamma_data, stats, Some(self.grad.clone()), gamma.grad.clone(), grad.clone()));
        HipVarDiff::node(var, grad.clone(), (op, grad), self.history)
    }

    /// Group normalisation with differentiable parameters: ONE forward node and ONE backward entry writing the gradients of
    /// `self`, `gamma` and `beta` (`GroupNormBackward`).
    pub fn group_norm(mut self, groups: usize, gamma: HipVarDiff<Ix1>, beta: HipVarDiff<Ix1>, eps: f64) -> HipVarDiff<D> {
        self.history.merge(gamma.history);
        self.history.merge(beta.history);
        let (input_data, gamma_data) = (self.var.data.clone(), gamma.var.data.clone());
        let samples = input_data.borrow().shape_c().first().map_or(0, |&n| n as usize);
        let stats = shared(Ix2(samples * groups, 2), &self.var.device());
        let grad = self.new_grad(self.grad.shape());
        let var = self.var.group_norm_with_stats(groups, gamma.var, beta.var, eps, Some(stats.clone()));
        let op: Rc<dyn Backward> = Rc::new(GroupNormBackward::new(input_data, gamma_data, stats, groups, Some(self.grad.clone()), gamma.grad.clone(),
                                                                   beta.grad.clone(), grad.clone()));
        HipVarDiff::node(var, grad.clone(), (op, grad), self.history)
    }

    /// Batch normalisation with differentiable parameters: ONE forward node and ONE backward entry writing the gradients of
    /// `self`, `gamma` and `beta` (`BatchNormBackward`).
    pub fn batch_norm(mut self, gamma: HipVarDiff<Ix1>, beta: HipVarDiff<Ix1>, running: Option<(HipVar<Ix1>, HipVar<Ix1>)>, momentum: f64, eps: f64,
                      status: Rc<Cell<bool>>) -> HipVarDiff<D> {
        self.history.merge(gamma.history);
        self.history.merge(beta.history);
        let (input_data, gamma_data) = (self.var.data.clone(), gamma.var.data.clone());
        let channels = gamma_data.borrow().len();
        let (stats, sums) = (shared(Ix2(channels, 2), &self.var.device()), shared(Ix2(channels, 2), &self.var.device()));
        let trained = Rc::new(Cell::new(true));
        let grad = self.new_grad(self.grad.shape());
        let var = self.var.batch_norm_with_stats(gamma.var, beta.var, running, momentum, eps, status, Some((stats.clone(), trained.clone())));
        let op: Rc<dyn Backward> = Rc::new(BatchNormBackward::new(input_data, gamma_data, stats, sums, trained, Some(self.grad.clone()),
                                                                   gamma.grad.clone(), beta.grad.clone(), grad.clone()));
        HipVarDiff::node(var, grad.clone(), (op, grad), self.history)
    }

    /// Max pooling: the forward node writes the offsets of the selected elements, the backward node gathers through them.
    pub fn max_pool(self, kernel: &[usize], stride: &[usize], padding: &[usize]) -> HipVarDiff<D> {
        let (dim, k, s, p) = pool_setup(&self.var.data.borrow().dimension(), kernel, stride, padding);
        let indices = shared(dim.clone(), &self.var.device());
        let grad = self.new_grad(dim);
        let var = self.var.max_pool_with_indices(kernel, stride, padding, Some(indices.clone()));
        let op = MaxPoolBackward::new(self.grad.clone(), indices, grad.clone(), k, s, p);
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }

    pub fn avg_pool(self, kernel: &[usize], stride: &[usize], padding: &[usize], count_include_pad: bool) -> HipVarDiff<D> {
        let (dim, k, s, p) = pool_setup(&self.var.data.borrow().dimension(), kernel, stride, padding);
        let grad = self.new_grad(dim);
        let var = self.var.avg_pool(kernel, stride, padding, count_include_pad);
        let op = AvgPoolBackward::new(self.grad.clone(), grad.clone(), k, s, p, count_include_pad);
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }

    /// Upsampling: the backward node gathers, per input element, from the outputs that read it (`nk_upsample_bwd`).
    pub fn upsample(self, out_size: &[usize], mode: &str, align_corners: bool) -> HipVarDiff<D> {
        let (dim, geometry) = upsample_setup(&self.var.data.borrow().dimension(), out_size, mode, align_corners);
        let grad = self.new_grad(dim);
        let var = self.var.upsample(out_size, mode, align_corners);
        let op = UpsampleBackward::new(self.grad.clone(), grad.clone(), geometry);
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }

    /// `avg_pool` over the whole spatial extents: `(N, C, 1, ..)`.
    pub fn global_avg_pool(self) -> HipVarDiff<D> {
        let extents: Vec<usize> = self.var.data.borrow().dimension().slice()[2..].to_vec();
        let zeros = vec![0usize; extents.len()];
        self.avg_pool(&extents, &extents, &zeros, true)
    }

    /// `VarDiff::log_softmax` (`vardiff.rs:381-387`).
    pub fn log_softmax(self, axis: usize) -> HipVarDiff<D> {
        let grad = self.new_grad(self.grad.shape());
        let var = self.var.log_softmax(axis);
        let op = LogSoftmaxBackward::new(self.grad.clone(), var.data.clone(), grad.clone(), axis);
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }

    /// `VarDiff::t` (`vardiff.rs:390-396`).
    pub fn t(self) -> HipVarDiff<D> {
        let var = self.var.t();
        let grad = Rc::new(Gradient::hip_zeros(var.data.borrow().dimension(), var.device()));
        let op = TransposeBackward::new(self.grad.clone(), grad.clone());
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }

    /// `VarDiff::dropout` (`vardiff.rs:418-427`): forward and backward node share the noise buffer; the backward node does
    /// NOT divide by `1 - p` (`node/dropout/mod.rs:123-126`, kept).
    pub fn dropout(self, p: f64, status: Rc<Cell<bool>>) -> HipVarDiff<D> {
        let grad = self.new_grad(self.grad.shape());
        let noise = shared(self.grad.shape(), &self.var.device());
        let var = self.var.dropout_with_noise(p, noise.clone(), status.clone());
        let op = DropoutBackward::new(self.grad.clone(), grad.clone(), p, noise, status);
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }

    /// `VarDiff::chunks` (`vardiff.rs:435-452`).
    pub fn chunks<E>(self, chunk_size: E) -> Vec<HipVarDiff<D>>
    where
        E: IntoDimension<Dim = D>,
    {
        self.var
            .chunks(chunk_size)
            .into_iter()
            .enumerate()
            .map(|(i, var)| {
                let grad = Rc::new(Gradient::hip_zeros(var.data.borrow().dimension(), var.device()));
                let op = ChunkBackward::new(self.grad.clone(), grad.clone(), i);
                HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history.clone())
            })
            .collect()
    }

    /// `VarDiff::cat` (`vardiff.rs:627-650`).
    pub fn cat(mut self, vars: &[Self], axis: usize) -> HipVarDiff<D> {
        let mut operands_gradients = vec![self.grad.clone()];
        let mut operands = Vec::with_capacity(vars.len());
        vars.iter().cloned().for_each(|v| {
            self.history.merge(v.history);
            operands_gradients.push(v.grad);
            operands.push(v.var);
        });
        let var = self.var.cat(&operands, axis);
        let grad = Rc::new(Gradient::hip_zeros(var.data.borrow().dimension(), var.device()));
        let op = MultiConcatenateBackward::new(operands_gradients, grad.clone(), axis);
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }

    /// `VarDiff::mse` (`vardiff.rs:495-506`).
    pub fn mse(self, target: HipVar<D>, reduction: Reduction) -> HipVarDiff<Ix0> {
        let grad = self.new_grad(ndarray::Dim(()));
        let op = SquaredErrorBackward::new(self.var.data.clone(), target.data.clone(), self.grad.clone(), grad.clone(), reduction.clone());
        let var = self.var.mse(target, reduction);
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }

    /// `VarDiff::pad` (`vardiff.rs:746-766`), zero mode; `pad_with` takes the other three modes.
    pub fn pad_zero(self, padding: &[usize]) -> HipVarDiff<D> {
        self.pad_with(padding, PadMode::Constant(0.))
    }

    /// `VarDiff::pad(padding, mode)` with the mode as a value (`PaddingMode`: the reference's four marker types `Zero`,
    /// `Constant`, `Reflective`, `Replicative`, `node/pad/`), which is how the `nn` convolution layers store it.
    pub fn pad(self, padding: &[usize], mode: PaddingMode) -> HipVarDiff<D> {
        self.pad_with(padding, mode.into())
    }

    pub(crate) fn pad_with(self, padding: &[usize], mode: PadMode) -> HipVarDiff<D> {
        let var = self.var.pad_with(padding, mode);
        let grad = Rc::new(Gradient::hip_zeros(var.data.borrow().dimension(), var.device()));
        let op = PadBackward::new(self.grad.clone(), grad.clone(), padding.iter().map(|&p| p as i32).collect());
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }

    /// Broadcast binary with two differentiable operands (`vardiff.rs:766-862` and the operator impls): forward node +
    /// the two fused un-broadcast backward nodes as one tape entry.
    pub(crate) fn binary<E>(mut self, op: BinaryOp, rhs: HipVarDiff<E>) -> HipVarDiff<Broadcast<D, E>>
    where
        D: DimMax<E>,
        E: 'static + Dimension,
    {
        self.history.merge(rhs.history);
        let (left_data, right_data) = (self.var.data.clone(), rhs.var.data.clone());
        let var = self.var.binary(op, rhs.var);
        let grad = Rc::new(Gradient::hip_zeros(var.data.borrow().dimension(), var.device()));
        let left = BinaryOperationBackwardLeft::new(op, right_data.clone(), self.grad.clone(), grad.clone());
        let right = BinaryOperationBackwardRight::new(op, left_data, right_data, rhs.grad.clone(), grad.clone());
        let node: Rc<dyn Backward> = Rc::new(Pair(left, right));
        HipVarDiff::node(var, grad.clone(), (node, grad), self.history)
    }
}

impl<D> HipVarDiff<D>
where
    D: 'static + Dimension + RemoveAxis,
{
    /// `Convolution::convolution` for a differentiable kernel and input (`vardiff.rs:1357-1431`): `self` is the KERNEL.
    /// One forward node; `ConvolutionBackwardInput` + `ConvolutionBackwardKernel` as one tape entry (`ConvolutionBackward`,
    /// `node/convolution/mod.rs:357-388`).
    pub fn convolution(mut self, input: HipVarDiff<D>, stride: &[usize], dilation: &[usize], groups: usize) -> HipVarDiff<D> {
        self.history.merge(input.history);
        let (input_data, kernel_data) = (input.var.data.clone(), self.var.data.clone());
        let var = self.var.convolution(input.var, stride, dilation, groups);
        let grad = Rc::new(Gradient::hip_zeros(var.data.borrow().dimension(), var.device()));
        let to_i32 = |v: &[usize]| v.iter().map(|&s| s as i32).collect::<Vec<_>>();
        let bwd_input = ConvolutionBackwardInput::new(kernel_data, input.grad.clone(), grad.clone(), to_i32(stride), to_i32(dilation), groups as i32);
        let bwd_kernel = ConvolutionBackwardKernel::new(input_data, self.grad.clone(), grad.clone(), to_i32(stride), to_i32(dilation), groups as i32);
        let node: Rc<dyn Backward> = Rc::new(Pair(bwd_input, bwd_kernel));
        HipVarDiff::node(var, grad.clone(), (node, grad), self.history)
    }
}

impl<D> HipVarDiff<D>
where
    D: 'static + Dimension + RemoveAxis,
{
    /// `convolution(..) + bias` of the `nn::Conv*` layers with kernel, input and bias differentiable: one forward node
    /// (`HipVar::convolution_bias`), and as one tape entry `ConvolutionBackwardInput` + `ConvolutionBackwardKernelBias` (the bias
    /// gradient summed on the way through the kernel-gradient pass - no second read of the output gradient).
    pub fn convolution_bias<B>(mut self, input: HipVarDiff<D>, bias: HipVarDiff<B>, stride: &[usize], dilation: &[usize],
                               groups: usize) -> HipVarDiff<D>
    where
        B: 'static + Dimension,
    {
        self.history.merge(input.history);
        self.history.merge(bias.history);
        let (input_data, kernel_data) = (input.var.data.clone(), self.var.data.clone());
        let var = self.var.convolution_bias(input.var, bias.var, stride, dilation, groups);
        let grad = Rc::new(Gradient::hip_zeros(var.data.borrow().dimension(), var.device()));
        let to_i32 = |v: &[usize]| v.iter().map(|&s| s as i32).collect::<Vec<_>>();
        let bwd_input = ConvolutionBackwardInput::new(kernel_data, input.grad.clone(), grad.clone(), to_i32(stride), to_i32(dilation), groups as i32);
        let bwd_kernel = ConvolutionBackwardKernelBias::new(input_data, self.grad.clone(), bias.grad.clone(), grad.clone(), to_i32(stride),
                                                            to_i32(dilation), groups as i32);
        let node: Rc<dyn Backward> = Rc::new(Pair(bwd_input, bwd_kernel));
        HipVarDiff::node(var, grad.clone(), (node, grad), self.history)
    }
}

impl<D> HipVarDiff<D>
where
    D: 'static + Dimension + RemoveAxis,
{
    /// Does the library run this module geometry with the Zero padding folded in (`nk_conv_padding_folds`: 3 x 3, stride 1, one group,
    /// padding 0 / 1, 64 | channel counts, even output extents, and sizes the rules give to the Winograd kernels)?  `self` is the KERNEL.
    pub fn padding_folds(&self, input: &HipVarDiff<D>, padding: &[usize], stride: &[usize], dilation: &[usize], groups: usize) -> bool {
        let to_i32 = |v: &[usize]| v.iter().map(|&s| s as i32).collect::<Vec<_>>();
        let (xs, ws) = (input.var.data.borrow().shape_c(), self.var.data.borrow().shape_c());
        let mut folds = 0i32;
        super::ffi::check(unsafe {
            super::ffi::nk_conv_padding_folds(self.var.device().as_raw(), xs.len() as i32 - 2, xs.as_ptr(), to_i32(padding).as_ptr(), ws.as_ptr(),
                                              to_i32(stride).as_ptr(), to_i32(dilation).as_ptr(), groups as i32, &mut folds)
        });
        folds != 0
    }

    /// `pad(padding, Zero) -> convolution -> + bias` of the `nn::Conv*` layers as ONE node pair WITHOUT the Pad node: `input` is the
    /// unpadded variable, forward on `nk_conv_bias_fwd_padded`, backward `nk_conv_bwd_input_padded` + `nk_conv_bwd_kernel_bias_padded`.
    /// Call only after `padding_folds` said yes (the entry points refuse other geometries).
    pub fn convolution_bias_padded<B>(mut self, input: HipVarDiff<D>, bias: HipVarDiff<B>, padding: &[usize], stride: &[usize],
                                      dilation: &[usize], groups: usize) -> HipVarDiff<D>
    where
        B: 'static + Dimension,
    {
        self.history.merge(input.history);
        self.history.merge(bias.history);
        let mut fwd_history = self.var.history;
        fwd_history.merge(input.var.history);
        fwd_history.merge(bias.var.history);
        let to_i32 = |v: &[usize]| v.iter().map(|&s| s as i32).collect::<Vec<_>>();
        let device = self.var.data.borrow().device().clone();
        let shape: D = {
            let (x, w) = (input.var.data.borrow(), self.var.data.borrow());
            let mut xs: Vec<usize> = x.dimension().slice().to_vec();
            for (i, p) in padding.iter().enumerate() {
                xs[2 + i] += 2 * p;
            }
            let ws: Vec<usize> = w.dimension().slice().to_vec();
            check_conv_args(&xs, &ws, stride, dilation);
            check_groups_args(&xs, &ws, groups);
            conv_out_shape(&xs, &ws, stride, dilation)
        };
        let data = shared(shape.clone(), &device);
        let fwd = ConvolutionBiasPadded::new(input.var.data.clone(), self.var.data.clone(), bias.var.data.clone(), data.clone(), to_i32(padding),
                                             to_i32(stride), to_i32(dilation), groups as i32);
        let var = HipVar::node(data, Rc::new(fwd), fwd_history);
        let grad = Rc::new(Gradient::hip_zeros(shape, device));
        let bwd = ConvolutionBackwardPadded::new(input.var.data, self.var.data, input.grad, self.grad, bias.grad, grad.clone(), to_i32(padding),
                                                 to_i32(stride), to_i32(dilation), groups as i32);
        let op: Rc<dyn Backward> = Rc::new(bwd);
        HipVarDiff::node(var, grad.clone(), (op, grad), self.history)
    }
}

impl<D> HipVarDiff<D>
where
    D: 'static + Dimension + RemoveAxis,
{
    /// Cross entropy of differentiable logits: ONE forward node and ONE backward entry (`CrossEntropyBackward`: the softmax
    /// recomputed from the logits and the forward's `lse`).  The targets are data: no gradient flows to them.
    pub fn cross_entropy(self, target: HipVar<D::Smaller>, reduction: Reduction, ignore_index: Option<usize>, label_smoothing: f64) -> HipVarDiff<Ix0> {
        let grad = self.new_grad(ndarray::Dim(()));
        let (input_data, target_data) = (self.var.data.clone(), target.data.clone());
        let (var, lse) = self.var.cross_entropy_with_lse(target, reduction.clone(), ignore_index, label_smoothing);
        let op = CrossEntropyBackward::new(input_data, target_data, lse, self.grad.clone(), grad.clone(), reduction, ignore_index.map_or(-1, |i| i as i64),
                                           label_smoothing);
        HipVarDiff::node(var, grad.clone(), (Rc::new(op), grad), self.history)
    }
}

impl HipVarDiff<Ix2> {
    /// Embedding over a differentiable table: ONE forward node and ONE backward entry (`EmbeddingBackward`: the ordered sum per
    /// table row).  Differentiable in the table only; ids equal to `padding_idx` contribute no gradient.
    pub fn embedding<E: 'static + Dimension>(self, indices: HipVar<E>, padding_idx: Option<usize>) -> HipVarDiff<E::Larger> {
        let rows = self.var.data.borrow().dimension()[0];
        assert!(rows <= 1 << 24, "embedding: at most 2^24 rows (ids are stored as f32)");
        assert!(padding_idx.map_or(true, |p| p < rows), "embedding: padding_idx is not a row of the table");
        let indices_data = indices.data.clone();
        let var = self.var.embedding(indices);
        let grad = Rc::new(Gradient::hip_zeros(var.data.borrow().dimension(), var.device()));
        let op: Rc<dyn Backward> = Rc::new(EmbeddingBackward::new(indices_data, self.grad.clone(), grad.clone(), padding_idx.map_or(-1, |p| p as i64)));
        HipVarDiff::node(var, grad.clone(), (op, grad), self.history)
    }
}

impl HipVarDiff<Ix2> {
    /// `mm` (`vardiff.rs:1073-1106`).
    pub fn mm(mut self, rhs: HipVarDiff<Ix2>) -> HipVarDiff<Ix2> {
        self.history.merge(rhs.history);
        let (left_data, right_data) = (self.var.data.clone(), rhs.var.data.clone());
        let var = self.var.mm(rhs.var);
        let grad = Rc::new(Gradient::hip_zeros(var.data.borrow().dimension(), var.device()));
        let left = MatrixMatrixMulBackwardLeft::new(right_data, self.grad.clone(), grad.clone());
        let right = MatrixMatrixMulBackwardRight::new(left_data, rhs.grad.clone(), grad.clone());
        let op: Rc<dyn Backward> = Rc::new(MatrixMatrixMulBackward::new(left, right));
        HipVarDiff::node(var, grad.clone(), (op, grad), self.history)
    }

    /// `mm_t` (`vardiff.rs:1110-1143`): the node `nn::Linear::forward` is made of (`neuronika-nn/src/lib.rs:443-446`).
    pub fn mm_t(mut self, rhs: HipVarDiff<Ix2>) -> HipVarDiff<Ix2> {
        self.history.merge(rhs.history);
        let (left_data, right_data) = (self.var.data.clone(), rhs.var.data.clone());
        let var = self.var.mm_t(rhs.var);
        let grad = Rc::new(Gradient::hip_zeros(var.data.borrow().dimension(), var.device()));
        let left = MatrixMatrixMulTBackwardLeft::new(right_data, self.grad.clone(), grad.clone());
        let right = MatrixMatrixMulTBackwardRight::new(left_data, rhs.grad.clone(), grad.clone());
        let op: Rc<dyn Backward> = Rc::new(MatrixMatrixMulTBackward::new(left, right));
        HipVarDiff::node(var, grad.clone(), (op, grad), self.history)
    }

    /// `nn::Linear::forward` over a differentiable input: ONE forward node (`HipVar::linear`) and ONE backward entry
    /// (`LinearBackward`: input gradient, bias gradient, weight gradient).  When `self` is itself the output of a
    /// Linear+ReLU node, its mask record travels into the backward node: the input gradient is then written through
    /// `nk_linear_bwd_input_relu` whenever the pass allows (`decide_premasking`) - the C4 graph runs without a single ReLU kernel.
    pub fn linear(mut self, weight: HipVarDiff<Ix2>, bias: HipVarDiff<Ix1>, relu: bool) -> HipVarDiff<Ix2> {
        self.history.merge(weight.history);
        self.history.merge(bias.history);
        let (input_data, weight_data) = (self.var.data.clone(), weight.var.data.clone());
        let var = self.var.linear(weight.var, bias.var, relu);
        let grad = Rc::new(Gradient::hip_zeros(var.data.borrow().dimension(), var.device()));
        let mask = if relu { Some(Rc::new(ReluMask::new(var.data.clone()))) } else { None };
        let op: Rc<dyn Backward> = Rc::new(LinearBackward::new(input_data, weight_data, mask.clone(), self.relu_mask.clone(),
                                                               Some(self.grad.clone()), weight.grad.clone(), bias.grad.clone(), grad.clone()));
        let mut out = HipVarDiff::node(var, grad.clone(), (op, grad), self.history);
        out.relu_mask = mask;
        out
    }

    /// `heads_attention` for PACKED projections: `self` is the `(batch*seq, 3*heads*dh)` output of one `Linear` over the
    /// row-stacked weights `[Wq; Wk; Wv]`; queries, keys and values are read in place as its three column blocks
    /// (`nk_attention_qkv_fwd` / `nk_attention_qkv_bwd`).  Output `(batch*seq, heads*dh)`.
    #[allow(clippy::too_many_arguments)]
    pub fn packed_heads_attention(self, batch: usize, seq: usize, heads: usize, dh: usize, scale: f32, p: f64,
                                  status: Rc<Cell<bool>>) -> HipVarDiff<Ix2> {
        self.packed_attention_node(batch, seq, heads, dh, scale, p, status, false)
    }

    /// `packed_heads_attention` for causal self-attention: query `r` of a sample attends to the keys `<= r` of that sample
    /// (`nk_attention_qkv_causal_fwd` / `_bwd`: the kernels skip the key tiles above the diagonal; the score / dS / Pd tiles there
    /// are neither written nor read).  Same dropout draws and offset advance as the full form.
    #[allow(clippy::too_many_arguments)]
    pub fn packed_heads_attention_causal(self, batch: usize, seq: usize, heads: usize, dh: usize, scale: f32, p: f64,
                                         status: Rc<Cell<bool>>) -> HipVarDiff<Ix2> {
        self.packed_attention_node(batch, seq, heads, dh, scale, p, status, true)
    }

    #[allow(clippy::too_many_arguments)]
    fn packed_attention_node(self, batch: usize, seq: usize, heads: usize, dh: usize, scale: f32, p: f64, status: Rc<Cell<bool>>,
                             causal: bool) -> HipVarDiff<Ix2> {
        let device = self.var.data.borrow().device().clone();
        let geometry = Heads { batch: batch as i32, seq: seq as i32, heads: heads as i32, dh: dh as i32 };
        let sp = (seq + 31) / 32 * 32;
        let big = |last: usize| shared(ndarray::Dim([batch * heads, sp, last]), &device);
        let state = Rc::new(AttentionState { scores: big(sp), stats: big(2), mask_bits: big(sp / 32), calls: Cell::new(0) });
        let dim = ndarray::Dim([batch * seq, heads * dh]);
        let data = shared(dim, &device);
        let fwd = PackedHeadsAttention::new(geometry, self.var.data.clone(), state.clone(), data.clone(), scale, p, status.clone(), next_seed(),
                                            causal);
        let var = HipVar::node(data.clone(), Rc::new(fwd), self.var.history);
        let grad = Rc::new(Gradient::hip_zeros(dim, device));
        let bwd = PackedHeadsAttentionBackward::new(geometry, self.var.data, data, state, big(sp), big(sp), self.grad, grad.clone(), scale, p,
                                                    status, causal);
        let op: Rc<dyn Backward> = Rc::new(bwd);
        HipVarDiff::node(var, grad.clone(), (op, grad), self.history)
    }

    /// The composed multi-head attention's per-(sample, head) chain `mm_t -> * scale -> softmax(1) -> dropout -> mm` as ONE
    /// node on the fused kernels (SURVEY.md 8a note; `self` = queries in the `(batch*seq, heads*dh)` projection layout).
    /// Callers check `ffi::nk_attention_supported` first and compose the five reference nodes on `chunks` otherwise.
    #[allow(clippy::too_many_arguments)]
    pub fn heads_attention(mut self, keys: HipVarDiff<Ix2>, values: HipVarDiff<Ix2>, batch: usize, seq: usize, heads: usize, dh: usize,
                           scale: f32, p: f64, status: Rc<Cell<bool>>) -> HipVarDiff<Ix2> {
        self.history.merge(keys.history);
        self.history.merge(values.history);
        let mut fwd_history = self.var.history;
        fwd_history.merge(keys.var.history);
        fwd_history.merge(values.var.history);
        let device = self.var.data.borrow().device().clone();
        let geometry = Heads { batch: batch as i32, seq: seq as i32, heads: heads as i32, dh: dh as i32 };
        // the scratch tensors are padded to whole 32 x 32 tiles: row count and row stride `sp` (include/neuronika_hip.h)
        let sp = (seq + 31) / 32 * 32;
        let big = |last: usize| shared(ndarray::Dim([batch * heads, sp, last]), &device);
        let state = Rc::new(AttentionState { scores: big(sp), stats: big(2), mask_bits: big(sp / 32), calls: Cell::new(0) });
        let dim = self.var.data.borrow().dimension();
        let data = shared(dim, &device);
        let fwd = HeadsAttention::new(geometry, self.var.data.clone(), keys.var.data.clone(), values.var.data.clone(), state.clone(),
                                      data.clone(), scale, p, status.clone(), next_seed());
        let var = HipVar::node(data.clone(), Rc::new(fwd), fwd_history);
        let grad = Rc::new(Gradient::hip_zeros(dim, device));
        let bwd = HeadsAttentionBackward::new(geometry, self.var.data, keys.var.data, values.var.data, data, state, big(sp), big(sp),
                                              self.grad, keys.grad, values.grad, grad.clone(), scale, p, status);
        let op: Rc<dyn Backward> = Rc::new(bwd);
        HipVarDiff::node(var, grad.clone(), (op, grad), self.history)
    }
}

// Operators: `+ - * /` between device variables (`var.rs:746-838`, `vardiff.rs:766-862` and their `std::ops` impls).
macro_rules! impl_binary {
    ($trait:ident, $fun:ident, $op:expr) => {
        impl<D, E> std::ops::$trait<HipVar<E>> for HipVar<D>
        where
            D: 'static + DimMax<E>,
            E: 'static + Dimension,
        {
            type Output = HipVar<Broadcast<D, E>>;

            fn $fun(self, rhs: HipVar<E>) -> Self::Output {
                self.binary($op, rhs)
            }
        }

        impl<D, E> std::ops::$trait<HipVarDiff<E>> for HipVarDiff<D>
        where
            D: 'static + DimMax<E>,
            E: 'static + Dimension,
        {
            type Output = HipVarDiff<Broadcast<D, E>>;

            fn $fun(self, rhs: HipVarDiff<E>) -> Self::Output {
                self.binary($op, rhs)
            }
        }
    };
}

impl_binary!(Add, add, BinaryOp::Add);
impl_binary!(Sub, sub, BinaryOp::Sub);
impl_binary!(Mul, mul, BinaryOp::Mul);
impl_binary!(Div, div, BinaryOp::Div);

/// The unused-import guard of `Ix3` (attention buffers are `Ix3`, built through `shared`).
#[allow(dead_code)]
type AttentionBuffer = HipArray<Ix3>;
