//! `neuronika_nn::hip` - the module API of `neuronika-nn/src/lib.rs` over the MI355X variables
//! (`neuronika_variable::hip::{HipVar, HipVarDiff}`).  To be added to the reference crate as
//! `#[cfg(feature = "hip")] pub mod hip;` (feature `hip = ["neuronika-variable/hip"]`).
//!
//! Why a twin module and not "nothing above `neuronika-variable` changes": the reference's layers hold CONCRETE CPU types
//! (`pub weight: VarDiff<Ix2>`, `neuronika-nn/src/lib.rs:406-409`; the convolution structs `:630-916`), so a layer whose
//! parameters live in HBM is a different struct.  Everything else is kept: field names, constructor argument order,
//! initialisation law (`U(-k, k)`, `k = 1 / sqrt(fan_in)`, `:428-430,776-778`), `forward` signatures, the train / eval switch
//! of `Dropout` (`ModelStatus`, `:84-137`).  `forward` of the convolution layers is `todo!()` in the reference (`:712-717`);
//! it is defined here as pad -> convolution -> + bias, the composition its fields describe.  `GroupedConv{1,2,3}d`,
//! `MultiheadAttention` and `Dropout` are named by the reference's module index (`src/lib.rs:783-797`) without structs in
//! the snapshot; their shapes follow the same conventions (`groups` after `dilation`).
//!
//! NOT COMPILED in the authoring image (no rustc / cargo); `tests/test_rust_binding.py` checks it structurally (balanced
//! delimiters, every `use` path names an item that exists, every layer calls variable methods that exist with their
//! arity).  The tested host mirror of the same layers is `host/neuronika.hpp` (`nn::*`) in this repository.
use std::{cell::{Cell, RefCell}, rc::Rc};

use ndarray::{Array, Dimension, Ix0, Ix1, Ix2, Ix3, Ix4, Ix5, RemoveAxis};
use neuronika_variable::{
    hip::{Device, Gate, HipVar, HipVarDiff, KvBuffers, PaddingMode, PagedBuffers, RotaryTable, SamplerState},
    Reduction,
};
use rand::distributions::{Distribution, Uniform};

/// `init::uniform` (`neuronika-nn/src/init.rs:177-193`) for a fresh parameter: values from U(low, high), drawn on the host.
fn uniform_parameter<D: Dimension + 'static>(dim: D, low: f32, high: f32, device: &Device) -> HipVarDiff<D> {
    let mut rng = rand::thread_rng();
    let between = Uniform::new(low, high);
    let host = Array::from_shape_simple_fn(dim, || between.sample(&mut rng));
    HipVarDiff::parameter(&host, device.clone())
}

/// Inputs a layer accepts: a device variable with or without gradient (`MatMatMulT<VarDiff<Ix2>>` bounds on
/// `Linear::forward`, `neuronika-nn/src/lib.rs:441-447`).
pub trait LinearInput {
    /// `input.mm_t(weight) + bias` as ONE node on `nk_linear_fwd` (with `relu`: `.relu()` too, `nk_linear_relu_fwd`).
    fn linear_layer(self, weight: HipVarDiff<Ix2>, bias: HipVarDiff<Ix1>, relu: bool) -> HipVarDiff<Ix2>;
}

impl LinearInput for HipVarDiff<Ix2> {
    fn linear_layer(self, weight: HipVarDiff<Ix2>, bias: HipVarDiff<Ix1>, relu: bool) -> HipVarDiff<Ix2> {
        self.linear(weight, bias, relu)
    }
}

impl LinearInput for HipVar<Ix2> {
    fn linear_layer(self, weight: HipVarDiff<Ix2>, bias: HipVarDiff<Ix1>, relu: bool) -> HipVarDiff<Ix2> {
        self.linear_diff(weight, bias, relu)
    }
}

/// `Linear` (`neuronika-nn/src/lib.rs:406-448`): `y = x A^T + b`.
pub struct Linear {
    pub weight: HipVarDiff<Ix2>,
    pub bias: HipVarDiff<Ix1>,
}

impl Linear {
    /// Weight `(out_features, in_features)`, bias `out_features`, both from U(-k, k), `k = (1 / in_features).sqrt()`.
    pub fn new(in_features: usize, out_features: usize, device: &Device) -> Self {
        let k = (1. / (in_features as f32)).sqrt();
        Self {
            weight: uniform_parameter(ndarray::Dim([out_features, in_features]), -k, k, device),
            bias: uniform_parameter(ndarray::Dim([out_features]), -k, k, device),
        }
    }

    /// `input.mm_t(weight) + bias` (`:441-447`) as ONE node: the MFMA GEMM with the bias in its epilogue (`nk_linear_fwd`);
    /// backward one entry (`LinearBackward`: input, bias and weight gradient).  Bit-identical to the two reference nodes.
    pub fn forward<I: LinearInput>(&self, input: I) -> HipVarDiff<Ix2> {
        input.linear_layer(self.weight.clone(), self.bias.clone(), false)
    }

    /// `self.forward(input).relu()` (`vardiff.rs:282-288`) as ONE node (`nk_linear_relu_fwd`); the backward of a following
    /// `Linear` writes this activation's gradient already masked (`nk_linear_bwd_input_relu`).  The explicit form of what the
    /// C++ mirror of this repository also reaches by a graph-build peephole on `forward(x).relu()`; same bits either way.
    pub fn forward_relu<I: LinearInput>(&self, input: I) -> HipVarDiff<Ix2> {
        input.linear_layer(self.weight.clone(), self.bias.clone(), true)
    }
}

/// Batch normalisation over `(N, spatial...)` per channel (the reference has no normalisation layer; semantics in
/// `include/neuronika_hip.h`), torch's `BatchNorm1d` / `2d` / `3d`: training normalises with the batch's mean and biased variance
/// and moves `running_mean` / `running_var` towards them by `momentum` (the running variance takes the unbiased estimate),
/// inference normalises with the running statistics.  `weight` starts as ones, `bias` as zeros, `running_mean` as zeros,
/// `running_var` as ones; the running statistics are plain buffers, not parameters.
macro_rules! batch_norm_layer {
    ($name:ident, $ranks:expr, $doc:expr) => {
        #[doc = $doc]
        pub struct $name {
            pub weight: HipVarDiff<Ix1>,
            pub bias: HipVarDiff<Ix1>,
            pub running_mean: HipVar<Ix1>,
            pub running_var: HipVar<Ix1>,
            pub eps: f64,
            pub momentum: f64,
            pub status: Rc<Cell<bool>>,
        }

        impl $name {
            pub fn new(num_features: usize, eps: f64, momentum: f64, device: &Device) -> Self {
                Self {
                    weight: HipVarDiff::parameter(&Array::ones(num_features), device.clone()),
                    bias: HipVarDiff::parameter(&Array::zeros(num_features), device.clone()),
                    running_mean: HipVar::from_ndarray(&Array::zeros(num_features), device.clone()),
                    running_var: HipVar::from_ndarray(&Array::ones(num_features), device.clone()),
                    eps,
                    momentum,
                    status: Rc::new(Cell::new(true)),
                }
            }

            pub fn train(&self) {
                self.status.set(true)
            }

            pub fn eval(&self) {
                self.status.set(false)
            }

            /// ONE forward node (`nk_batch_norm_fwd` / `nk_batch_norm_infer_fwd`) and ONE backward entry (`nk_batch_norm_bwd_sums`,
            /// `nk_batch_norm_bwd`, `nk_batch_norm_bwd_params`).
            pub fn forward<D: Dimension + 'static>(&self, input: HipVarDiff<D>) -> HipVarDiff<D> {
                let shape = input.shape();
                assert!($ranks.contains(&shape.len()), "{}: an input of {} dimensions", stringify!($name), shape.len());
                assert!(shape[1] == self.weight.shape()[0], "{}: expected {} channels, got {}", stringify!($name), self.weight.shape()[0], shape[1]);
                input.batch_norm(self.weight.clone(), self.bias.clone(), Some((self.running_mean.clone(), self.running_var.clone())), self.momentum,
                                 self.eps, self.status.clone())
            }
        }
    };
}

batch_norm_layer!(BatchNorm1d, [2usize, 3], "Batch normalisation of `(N, C)` or `(N, C, L)` inputs.");
batch_norm_layer!(BatchNorm2d, [4usize], "Batch normalisation of `(N, C, H, W)` inputs.");
batch_norm_layer!(BatchNorm3d, [5usize], "Batch normalisation of `(N, C, D, H, W)` inputs.");

/// Max / average pooling layers (the reference has none; semantics in `include/neuronika_hip.h`), torch's `MaxPool1d / 2d / 3d` and
/// `AvgPool1d / 2d / 3d` in floor mode with dilation 1: no parameters; an empty `stride` means `stride = kernel_size`.
macro_rules! pool_layer {
    ($name:ident, $nd:expr, $average:expr, $doc:expr) => {
        #[doc = $doc]
        pub struct $name {
            pub kernel_size: Vec<usize>,
            pub stride: Vec<usize>,
            pub padding: Vec<usize>,
            pub count_include_pad: bool,
        }

        impl $name {
            pub fn new(kernel_size: &[usize], stride: &[usize], padding: &[usize]) -> Self {
                assert!(kernel_size.len() == $nd, "{}: kernel_size takes {} entries", stringify!($name), $nd);
                let stride = if stride.is_empty() { kernel_size } else { stride };
                let padding = if padding.is_empty() { vec![0; $nd] } else { padding.to_vec() };
                assert!(stride.len() == $nd && padding.len() == $nd, "{}: stride and padding take {} entries", stringify!($name), $nd);
                Self { kernel_size: kernel_size.to_vec(), stride: stride.to_vec(), padding, count_include_pad: true }
            }

            /// ONE forward node and ONE backward entry (`nk_max_pool_fwd` / `nk_max_pool_bwd`, `nk_avg_pool_fwd` / `nk_avg_pool_bwd`).
            pub fn forward<D: Dimension + 'static>(&self, input: HipVarDiff<D>) -> HipVarDiff<D> {
                assert!(input.shape().len() == $nd + 2, "{}: an input of {} dimensions", stringify!($name), input.shape().len());
                if $average {
                    input.avg_pool(&self.kernel_size, &self.stride, &self.padding, self.count_include_pad)
                } else {
                    input.max_pool(&self.kernel_size, &self.stride, &self.padding)
                }
            }
        }
    };
}

pool_layer!(MaxPool1d, 1usize, false, "Max pooling of `(N, C, L)` inputs.");
pool_layer!(MaxPool2d, 2usize, false, "Max pooling of `(N, C, H, W)` inputs.");
pool_layer!(MaxPool3d, 3usize, false, "Max pooling of `(N, C, D, H, W)` inputs.");
pool_layer!(AvgPool1d, 1usize, true, "Average pooling of `(N, C, L)` inputs (`count_include_pad` is a public field, `true` after `new`).");
pool_layer!(AvgPool2d, 2usize, true, "Average pooling of `(N, C, H, W)` inputs (`count_include_pad` is a public field, `true` after `new`).");
pool_layer!(AvgPool3d, 3usize, true, "Average pooling of `(N, C, D, H, W)` inputs (`count_include_pad` is a public field, `true` after `new`).");

/// torch's `nn.Upsample` (the reference has none; semantics in `include/neuronika_hip.h`): either `size` (one entry per spatial axis)
/// or `scale_factor` (one value, or one per axis; `out_i = floor(in_i * scale_i)` in f64, after which the index arithmetic sees `in_i`
/// and `out_i` alone), never both.  `mode` is "nearest", or "linear" / "bilinear" / "trilinear" for 1 / 2 / 3 spatial axes, checked
/// against the input's rank at `forward`.  No parameters.
pub struct Upsample {
    pub size: Vec<usize>,
    pub scale_factor: Vec<f64>,
    pub mode: String,
    pub align_corners: bool,
}

impl Upsample {
    pub fn new(size: &[usize], scale_factor: &[f64], mode: &str, align_corners: bool) -> Self {
        assert!(size.is_empty() != scale_factor.is_empty(), "Upsample: give either size or scale_factor, not both and not neither");
        assert!(["nearest", "linear", "bilinear", "trilinear"].contains(&mode), "Upsample: unknown mode {:?}", mode);
        assert!(mode != "nearest" || !align_corners, "Upsample: align_corners has no meaning for the nearest mode");
        assert!(scale_factor.iter().all(|s| s.is_finite() && *s > 0.0), "Upsample: scale_factor entries must be finite and positive");
        Self { size: size.to_vec(), scale_factor: scale_factor.to_vec(), mode: mode.to_string(), align_corners }
    }

    /// The output extents for an input of this shape (what `nk_upsample_out_size` computes).
    pub fn output_size(&self, input_shape: &[usize]) -> Vec<usize> {
        let nd = input_shape.len().saturating_sub(2);
        if !self.size.is_empty() {
            assert!(self.size.len() == nd, "Upsample: size takes {} entries", nd);
            return self.size.clone();
        }
        assert!(self.scale_factor.len() == 1 || self.scale_factor.len() == nd, "Upsample: scale_factor takes one entry, or {}", nd);
        (0..nd).map(|i| (input_shape[2 + i] as f64 * self.scale_factor[if self.scale_factor.len() == 1 { 0 } else { i }]).floor() as usize).collect()
    }

    /// ONE forward node and ONE backward entry (`nk_upsample_fwd` / `nk_upsample_bwd`).
    pub fn forward<D: Dimension + 'static>(&self, input: HipVarDiff<D>) -> HipVarDiff<D> {
        let out = self.output_size(&input.shape());
        input.upsample(&out, &self.mode, self.align_corners)
    }
}

/// Layer normalisation over the trailing dimensions `normalized_shape` of the input (the reference has no normalisation layer;
/// semantics in `include/neuronika_hip.h`): `y = (x - mean) / sqrt(var + eps) * weight + bias` per row, biased variance.
/// `weight` starts as ones, `bias` as zeros, both of `normalized_shape` (dimension `E`).
pub struct LayerNorm<E: Dimension> {
    pub weight: HipVarDiff<E>,
    pub bias: HipVarDiff<E>,
    pub eps: f64,
}

impl<E: Dimension + 'static> LayerNorm<E> {
    pub fn new(normalized_shape: E, eps: f64, device: &Device) -> Self {
        Self {
            weight: HipVarDiff::parameter(&Array::ones(normalized_shape.clone()), device.clone()),
            bias: HipVarDiff::parameter(&Array::zeros(normalized_shape), device.clone()),
            eps,
        }
    }

    /// ONE forward node (`nk_layer_norm_fwd`) and ONE backward entry (`nk_layer_norm_bwd`, `nk_layer_norm_bwd_params`).
    pub fn forward<D: Dimension + 'static>(&self, input: HipVarDiff<D>) -> HipVarDiff<D> {
        input.layer_norm(self.weight.clone(), self.bias.clone(), self.eps)
    }
}

/// Group normalisation (the reference has no normalisation layer; semantics in `include/neuronika_hip.h`), torch's `GroupNorm`:
/// the channels of an `(N, C, spatial...)` input are cut into `num_groups` groups, each `(sample, group)` is normalised over its
/// channels and positions and then scaled and shifted per channel.  `weight` starts as ones, `bias` as zeros, both of shape `(C)`.
pub struct GroupNorm {
    pub weight: HipVarDiff<Ix1>,
    pub bias: HipVarDiff<Ix1>,
    pub num_groups: usize,
    pub eps: f64,
}

impl GroupNorm {
    pub fn new(num_groups: usize, num_channels: usize, eps: f64, device: &Device) -> Self {
        assert!(num_groups > 0 && num_channels % num_groups == 0, "GroupNorm: num_channels must be a multiple of num_groups");
        Self {
            weight: HipVarDiff::parameter(&Array::ones(num_channels), device.clone()),
            bias: HipVarDiff::parameter(&Array::zeros(num_channels), device.clone()),
            num_groups,
            eps,
        }
    }

    /// ONE forward node (`nk_group_norm_fwd`) and ONE backward entry (`nk_group_norm_bwd`, `nk_group_norm_bwd_params`).
    pub fn forward<D: Dimension + 'static>(&self, input: HipVarDiff<D>) -> HipVarDiff<D> {
        input.group_norm(self.num_groups, self.weight.clone(), self.bias.clone(), self.eps)
    }
}

/// Instance normalisation, torch's `InstanceNorm1d / 2d / 3d` with `affine = true`: group normalisation with one channel per group.
/// Running statistics (`track_running_stats`) are not built: the statistics are always the input's own.
macro_rules! instance_norm_layer {
    ($name:ident, $rank:expr, $doc:expr) => {
        #[doc = $doc]
        pub struct $name {
            pub weight: HipVarDiff<Ix1>,
            pub bias: HipVarDiff<Ix1>,
            pub num_features: usize,
            pub eps: f64,
        }

        impl $name {
            pub fn new(num_features: usize, eps: f64, device: &Device) -> Self {
                Self {
                    weight: HipVarDiff::parameter(&Array::ones(num_features), device.clone()),
                    bias: HipVarDiff::parameter(&Array::zeros(num_features), device.clone()),
                    num_features,
                    eps,
                }
            }

            pub fn forward<D: Dimension + 'static>(&self, input: HipVarDiff<D>) -> HipVarDiff<D> {
                assert!(input.shape().len() == $rank, "{}: an input of {} dimensions", stringify!($name), input.shape().len());
                input.group_norm(self.num_features, self.weight.clone(), self.bias.clone(), self.eps)
            }
        }
    };
}

instance_norm_layer!(InstanceNorm1d, 3usize, "Instance normalisation of `(N, C, L)` inputs.");
instance_norm_layer!(InstanceNorm2d, 4usize, "Instance normalisation of `(N, C, H, W)` inputs.");
instance_norm_layer!(InstanceNorm3d, 5usize, "Instance normalisation of `(N, C, D, H, W)` inputs.");

/// RMS normalisation over the trailing dimensions `normalized_shape` of the input (the reference has no normalisation layer;
/// semantics in `include/neuronika_hip.h`): `y = x / sqrt(mean(x^2) + eps) * weight` per row, no centring and no bias, the
/// normalisation of LLaMA-style decoders (`eps` = 1e-6 there).  `weight` starts as ones of `normalized_shape` (dimension `E`).
pub struct RMSNorm<E: Dimension> {
    pub weight: HipVarDiff<E>,
    pub eps: f64,
}

impl<E: Dimension + 'static> RMSNorm<E> {
    pub fn new(normalized_shape: E, eps: f64, device: &Device) -> Self {
        Self { weight: HipVarDiff::parameter(&Array::ones(normalized_shape), device.clone()), eps }
    }

    /// ONE forward node (`nk_rms_norm_fwd`) and ONE backward entry (`nk_rms_norm_bwd`, `nk_rms_norm_bwd_gamma`).
    pub fn forward<D: Dimension + 'static>(&self, input: HipVarDiff<D>) -> HipVarDiff<D> {
        input.rms_norm(self.weight.clone(), self.eps)
    }
}

/// Embedding table (the reference has no such layer; semantics in `include/neuronika_hip.h`): `forward(indices)` = the rows of
/// `weight` `(num_embeddings, embedding_dim)` selected by the ids of `indices` (f32, any dimension), with one more axis of extent
/// `embedding_dim`.  `weight` ~ N(0, 1) (`init::normal`, `neuronika-nn/src/init.rs:195-201`), the row `padding_idx` zeroed; that row
/// receives no gradient.
pub struct Embedding {
    pub weight: HipVarDiff<Ix2>,
    pub padding_idx: Option<usize>,
}

impl Embedding {
    pub fn new(num_embeddings: usize, embedding_dim: usize, padding_idx: Option<usize>, device: &Device) -> Self {
        assert!(padding_idx.map_or(true, |p| p < num_embeddings), "Embedding: padding_idx is not a row of the table");
        let mut rng = rand::thread_rng();
        let normal = rand_distr::Normal::new(0f32, 1f32).unwrap();
        let mut host = Array::from_shape_simple_fn((num_embeddings, embedding_dim), || normal.sample(&mut rng));
        if let Some(p) = padding_idx {
            host.row_mut(p).fill(0.);
        }
        Self { weight: HipVarDiff::parameter(&host, device.clone()), padding_idx }
    }

    /// ONE forward node (`nk_embedding_fwd`) and ONE backward entry (`nk_embedding_bwd`).
    pub fn forward<E: Dimension + 'static>(&self, indices: HipVar<E>) -> HipVarDiff<E::Larger> {
        self.weight.clone().embedding(indices, self.padding_idx)
    }
}

/// GELU (the reference has no such layer; semantics in `include/neuronika_hip.h`): `x Phi(x)`, or its tanh form when
/// `approximate_tanh` is set.  No parameters; ONE forward node and ONE backward entry.
pub struct GELU {
    pub approximate_tanh: bool,
}

impl GELU {
    pub fn new(approximate_tanh: bool) -> Self {
        Self { approximate_tanh }
    }

    pub fn forward<D: Dimension + 'static>(&self, input: HipVarDiff<D>) -> HipVarDiff<D> {
        if self.approximate_tanh {
            input.gelu_tanh()
        } else {
            input.gelu()
        }
    }
}

/// SiLU `x sigma(x)` (the reference has no such layer).  No parameters.
pub struct SiLU;

impl SiLU {
    pub fn forward<D: Dimension + 'static>(&self, input: HipVarDiff<D>) -> HipVarDiff<D> {
        input.silu()
    }
}

/// Gated linear unit (the reference has no such layer): `a * gate(b)` over the two halves of the input's last axis.
/// `Gate::Sigmoid` is GLU, `Gate::Gelu` GeGLU, `Gate::Silu` SwiGLU.  No parameters.
pub struct GLU {
    pub gate: Gate,
}

impl GLU {
    pub fn new(gate: Gate) -> Self {
        Self { gate }
    }

    pub fn forward<D: Dimension + 'static>(&self, input: HipVarDiff<D>) -> HipVarDiff<D> {
        input.glu(self.gate)
    }
}

/// Cross entropy criterion (the reference has no such layer; semantics in `include/neuronika_hip.h`): `forward(logits, target)` =
/// `logits.cross_entropy(target, reduction, ignore_index, label_smoothing)`, log-softmax and NLL in one node.  No parameters.
pub struct CrossEntropyLoss {
    pub reduction: Reduction,
    pub ignore_index: Option<usize>,
    pub label_smoothing: f64,
}

impl CrossEntropyLoss {
    pub fn new(reduction: Reduction, ignore_index: Option<usize>, label_smoothing: f64) -> Self {
        assert!((0. ..1.).contains(&label_smoothing), "CrossEntropyLoss: label_smoothing must be in [0, 1)");
        Self { reduction, ignore_index, label_smoothing }
    }

    /// ONE forward node (`nk_cross_entropy_fwd`) and ONE backward entry (`nk_cross_entropy_bwd`).
    pub fn forward<D: Dimension + RemoveAxis + 'static>(&self, logits: HipVarDiff<D>, target: HipVar<D::Smaller>) -> HipVarDiff<Ix0> {
        logits.cross_entropy(target, self.reduction.clone(), self.ignore_index, self.label_smoothing)
    }
}

/// `ModelStatus`-style switch shared with the dropout nodes (`neuronika-nn/src/lib.rs:84-137`, `node/dropout/mod.rs:27`).
pub struct Dropout {
    pub p: f64,
    pub status: Rc<Cell<bool>>,
}

impl Dropout {
    /// # Panics
    /// As `Dropout::new` of the node (`node/dropout/mod.rs:31-50`) when `p` is outside `[0, 1]`.
    pub fn new(p: f64) -> Self {
        if !(0. ..=1.).contains(&p) {
            panic!("Dropout probability has to be between 0 and 1, but got {}.", p);
        }
        Self { p, status: Rc::new(Cell::new(true)) }
    }

    pub fn train(&self) {
        self.status.set(true)
    }

    pub fn eval(&self) {
        self.status.set(false)
    }

    pub fn forward<D: Dimension + 'static>(&self, input: HipVarDiff<D>) -> HipVarDiff<D> {
        input.dropout(self.p, self.status.clone())
    }
}

macro_rules! conv_layer {
    ($name:ident, $grouped:ident, $dim:ty, $bias_dim:ty, $size:ty, $doc:literal, $kernel_dim:expr, $bias_shape:expr, $volume:expr, $list:expr) => {
        #[doc = $doc]
        pub struct $name {
            pub padding: $size,
            pub padding_mode: PaddingMode,
            pub stride: $size,
            pub dilation: $size,
            pub weight: HipVarDiff<$dim>,
            pub bias: HipVarDiff<$bias_dim>,
        }

        impl $name {
            /// Argument order of the reference's `new` (`neuronika-nn/src/lib.rs:671-679,762-770,857-865`) plus the device.
            /// Weight and bias from U(-k, k), `k = (1 / (in_channels * kernel volume)).sqrt()`.
            #[allow(clippy::too_many_arguments)]
            pub fn new(in_channels: usize, out_channels: usize, kernel_size: $size, padding: $size, padding_mode: PaddingMode,
                       stride: $size, dilation: $size, device: &Device) -> Self {
                let k = (1. / ((in_channels * $volume(kernel_size)) as f32)).sqrt();
                Self {
                    padding,
                    padding_mode,
                    stride,
                    dilation,
                    weight: uniform_parameter($kernel_dim(out_channels, in_channels, kernel_size), -k, k, device),
                    bias: uniform_parameter($bias_shape(out_channels), -k, k, device),
                }
            }

            /// pad -> convolution + bias as ONE node (`nk_conv_bias_fwd`: implicit GEMM or Winograd F(2x2, 3x3) on the MFMA core,
            /// the bias in the epilogue; backward `nk_conv_bwd_input` and `nk_conv_bwd_kernel_bias`).  The reference leaves the
            /// body as `todo!()` (`:712-717`).
            pub fn forward(&self, input: HipVarDiff<$dim>) -> HipVarDiff<$dim> {
                // Zero padding the library's kernels can read through (the Winograd geometries): no Pad node, no padded copy
                if matches!(self.padding_mode, PaddingMode::Zero)
                    && self.weight.padding_folds(&input, &$list(self.padding), &$list(self.stride), &$list(self.dilation), 1)
                {
                    return self.weight.clone().convolution_bias_padded(input, self.bias.clone(), &$list(self.padding), &$list(self.stride),
                                                                       &$list(self.dilation), 1);
                }
                let padded = input.pad(&$list(self.padding), self.padding_mode);
                self.weight.clone().convolution_bias(padded, self.bias.clone(), &$list(self.stride), &$list(self.dilation), 1)
            }
        }

        /// The grouped twin (named by `src/lib.rs:783-797`): `groups` after `dilation`, weight `(out, in / groups, k..)`.
        pub struct $grouped {
            pub padding: $size,
            pub padding_mode: PaddingMode,
            pub stride: $size,
            pub dilation: $size,
            pub groups: usize,
            pub weight: HipVarDiff<$dim>,
            pub bias: HipVarDiff<$bias_dim>,
        }

        impl $grouped {
            #[allow(clippy::too_many_arguments)]
            pub fn new(in_channels: usize, out_channels: usize, kernel_size: $size, padding: $size, padding_mode: PaddingMode,
                       stride: $size, dilation: $size, groups: usize, device: &Device) -> Self {
                assert!(groups > 0 && in_channels % groups == 0 && out_channels % groups == 0, "channels must be divisible by groups");
                let k = (1. / ((in_channels / groups * $volume(kernel_size)) as f32)).sqrt();
                Self {
                    padding,
                    padding_mode,
                    stride,
                    dilation,
                    groups,
                    weight: uniform_parameter($kernel_dim(out_channels, in_channels / groups, kernel_size), -k, k, device),
                    bias: uniform_parameter($bias_shape(out_channels), -k, k, device),
                }
            }

            pub fn forward(&self, input: HipVarDiff<$dim>) -> HipVarDiff<$dim> {
                let padded = input.pad(&$list(self.padding), self.padding_mode);
                self.weight.clone().convolution_bias(padded, self.bias.clone(), &$list(self.stride), &$list(self.dilation), self.groups)
            }
        }
    };
}

conv_layer!(Conv1d, GroupedConv1d, Ix3, Ix2, usize,
            "`Conv1d` (`neuronika-nn/src/lib.rs:630-718`): input `(N, Cin, L)`, kernel `(Cout, Cin, Lk)`, bias `(Cout, 1)`.",
            |o, i, k: usize| ndarray::Dim([o, i, k]), |o| ndarray::Dim([o, 1]), |k: usize| k, |v: usize| [v]);
conv_layer!(Conv2d, GroupedConv2d, Ix4, Ix3, (usize, usize),
            "`Conv2d` (`neuronika-nn/src/lib.rs:724-812`): input `(N, Cin, H, W)`, kernel `(Cout, Cin, Hk, Wk)`, bias `(Cout, 1, 1)`.",
            |o, i, k: (usize, usize)| ndarray::Dim([o, i, k.0, k.1]), |o| ndarray::Dim([o, 1, 1]), |k: (usize, usize)| k.0 * k.1,
            |v: (usize, usize)| [v.0, v.1]);
conv_layer!(Conv3d, GroupedConv3d, Ix5, Ix4, (usize, usize, usize),
            "`Conv3d` (`neuronika-nn/src/lib.rs:818-916`): input `(N, Cin, D, H, W)`, kernel `(Cout, Cin, Dk, Hk, Wk)`, bias `(Cout, 1, 1, 1)`.",
            |o, i, k: (usize, usize, usize)| ndarray::Dim([o, i, k.0, k.1, k.2]), |o| ndarray::Dim([o, 1, 1, 1]),
            |k: (usize, usize, usize)| k.0 * k.1 * k.2, |v: (usize, usize, usize)| [v.0, v.1, v.2]);

/// The keys and values of one causal attention layer between the steps of incremental decoding (ours; the tested mirror is
/// `nn::KvCache` in `host/neuronika.hpp`): device buffers `(batch, heads, capacity, head_dim)` and the per-sample lengths on the
/// host.  `MultiheadAttention::forward_step` advances the lengths when it builds its node.
/// `new_rolling`: a ring for a sliding-window layer (`MultiheadAttention::window`) - position `p` lives at slot `p % capacity`, the
/// lengths grow past the capacity, and `high_water` keeps the largest length every sample has reached since the last `reset`: the
/// slots hold the positions `[high_water - capacity, high_water)`.
pub struct KvCache {
    pub buffers: KvBuffers,
    lens: RefCell<Vec<usize>>,
    high: RefCell<Vec<usize>>,
    window: Cell<usize>, // of the layer that last stepped the cache (0: none yet)
}

impl KvCache {
    pub fn new(batch: usize, heads: usize, head_dim: usize, capacity: usize, device: &Device) -> Self {
        Self { buffers: KvBuffers::new(batch, heads, head_dim, capacity, device), lens: RefCell::new(vec![0; batch]),
               high: RefCell::new(vec![0; batch]), window: Cell::new(0) }
    }

    pub fn new_rolling(batch: usize, heads: usize, head_dim: usize, capacity: usize, device: &Device) -> Self {
        Self { buffers: KvBuffers::new_rolling(batch, heads, head_dim, capacity, device), lens: RefCell::new(vec![0; batch]),
               high: RefCell::new(vec![0; batch]), window: Cell::new(0) }
    }

    pub fn rolling(&self) -> bool {
        self.buffers.rolling()
    }

    /// The largest length every sample has reached since the last `reset`.
    pub fn high_water(&self) -> Vec<usize> {
        self.high.borrow().clone()
    }

    pub fn capacity(&self) -> usize {
        self.buffers.geometry().2
    }

    /// Positions held per sample.
    pub fn lens(&self) -> Vec<usize> {
        self.lens.borrow().clone()
    }

    /// Every length back to 0; the buffers are kept.
    pub fn reset(&self) {
        self.lens.borrow_mut().iter_mut().for_each(|l| *l = 0);
        self.high.borrow_mut().iter_mut().for_each(|l| *l = 0);
    }

    /// Every sample to a length no longer than its current one: ragged prompts after a right-padded prefill (under the causal
    /// rule the padding never influenced the real positions), and roll-back.  On a rolling cache the next query's window must
    /// still lie in the ring: `max(0, l - W) >= high_water - capacity`, `W` the window of the layer that last stepped the cache
    /// (remembered by `forward_step`; the capacity before any step).
    pub fn truncate(&self, lens: &[usize]) {
        let mut mine = self.lens.borrow_mut();
        assert!(lens.len() == mine.len(), "KvCache::truncate: one length per sample");
        assert!(lens.iter().zip(mine.iter()).all(|(new, old)| new <= old), "KvCache::truncate: a sample cannot grow");
        if self.rolling() {
            let capacity = self.capacity();
            let w = if self.window.get() > 0 { self.window.get() } else { capacity };
            assert!(lens.iter().zip(self.high.borrow().iter()).all(|(&l, &h)| l.saturating_sub(w) + capacity >= h),
                    "KvCache::truncate: the window of the next query would read positions that were overwritten");
        }
        mine.copy_from_slice(lens);
    }

    fn advance(&self, rows: usize) {
        self.lens.borrow_mut().iter_mut().for_each(|l| *l += rows);
        self.high.borrow_mut().iter_mut().zip(self.lens.borrow().iter()).for_each(|(h, &l)| *h = (*h).max(l));
    }
}

/// Rotary position embedding (ours; the tested mirror is `nn::RotaryEmbedding` in `host/neuronika.hpp`): owns the table of
/// `(cos, sin)` of `p * base^(-2j/rot)`, no parameters.  Shared between the layers of a model through `Rc`:
/// `MultiheadAttention::rope`, `HipVar / HipVarDiff::rope`.
pub struct RotaryEmbedding {
    pub table: RotaryTable,
}

impl RotaryEmbedding {
    /// `rot`: the rotated columns of every head (even, at most `head_dim`); `interleaved`: pairs `(2j, 2j+1)` instead of
    /// `(j, j + rot/2)`.
    pub fn new(head_dim: usize, max_pos: usize, base: f64, rot: usize, interleaved: bool, device: &Device) -> Self {
        Self { table: RotaryTable::new(head_dim, max_pos, base, rot, interleaved, device) }
    }

    /// `input`: `(batch * seq, heads * head_dim)` at positions `0 .. seq - 1`.
    pub fn forward(&self, input: HipVarDiff<Ix2>, batch: usize, heads: usize) -> HipVarDiff<Ix2> {
        input.rope(&self.table, batch, heads)
    }
}

/// Token sampling on the device (ours; the tested mirror is `nn::Sampler` in `host/neuronika.hpp`): greedy at `temperature == 0`, else
/// temperature, top-k (`0`: off), top-p (`1.`: off) and one Philox draw per row.  The ids come back as f32 on the device, the form
/// `Embedding::forward` takes: a generation loop never leaves the device.  No parameters, no gradient.
pub struct Sampler {
    pub state: SamplerState,
}

impl Sampler {
    pub fn new(temperature: f32, top_k: usize, top_p: f32, seed: u64) -> Self {
        Self { state: SamplerState::new(temperature, top_k, top_p, seed) }
    }

    /// `logits`: `(batch * seq, vocab)`; the `(batch,)` ids of the last position of every sample.  A differentiable input enters
    /// through `HipVarDiff::detached`.
    pub fn forward(&self, logits: HipVar<Ix2>, batch: usize) -> HipVar<Ix1> {
        logits.sample(&self.state, batch)
    }
}

/// Multi-head self-attention composed from reference operations (module named by `src/lib.rs:783-797`; SURVEY.md 8a note):
/// `Q, K, V = x.mm_t(W) + b`; per (sample, head): `P = dropout(softmax(Q K^T / sqrt(dh)))`, `O = P V`; `out = O.mm_t(Wo) + bo`.
/// Input rows are `(batch * seq, d_model)`.
///
/// The three input projections are PACKED: `qkv` is one `Linear(d_model, 3 * d_model)` whose weight rows are `[Wq; Wk; Wv]`
/// (`q_weight()` / `k_weight()` / `v_weight()` name the row blocks for initialisation from separate matrices) - one GEMM with
/// N = 3 d forward and one with K = 3 d for the input gradient instead of three each - and the per-head chain is one node
/// reading queries, keys and values in place as the column blocks of that projection (`HipVarDiff::packed_heads_attention`:
/// `nk_attention_qkv_fwd` / `nk_attention_qkv_bwd`, or their `_causal_` counterparts when `causal` is set).  Head sizes the fused core does not cover
/// (`ffi::nk_attention_supported`: dh in {32, 64, 128}) are rejected at construction.
pub struct MultiheadAttention {
    pub qkv: Linear,
    pub o: Linear,
    pub d_model: usize,
    pub heads: usize,
    /// Grouped-query attention (the tested mirror is `nn::MultiheadAttention::kv_heads` in `host/neuronika.hpp`): key / value heads, a
    /// divisor of `heads`; `heads` after `new`.  With fewer, `qkv` is `Linear(d_model, d_model + 2 * kv_heads * dh)`, rows
    /// `[Wq; Wk; Wv]`, `forward_step` appends `kv_heads` heads to a `KvCache` built with `kv_heads` and attends through
    /// `nk_attention_decode_gqa_fwd`.  The TRAINING forward of a grouped layer is not mirrored here: it is composed from separate
    /// projections, `HipVarDiff::repeat_kv` on K and V and `heads_attention`, as `host/neuronika.cpp` composes it.
    pub kv_heads: usize,
    pub dropout: Dropout,
    /// Causal self-attention: query `r` of a sample attends to the keys `<= r` of that sample (`P = dropout(softmax(scores * scale +
    /// M))`, `M` = 0 on and below the diagonal, -inf above).  Read by `forward` when it builds the graph; `false` after `new`.
    pub causal: bool,
    /// Rotary position embedding of the queries and keys: `None` after `new`, and then every graph is the one built without it.
    /// Read by `forward` / `forward_step` when they build their nodes: the Q|K blocks of the packed projection are rotated in place
    /// right behind the projection (one launch, `2 * heads` heads, stride `3 * d_model`), at `lens[b] + t` in `forward_step`, so the
    /// cache holds rotated keys; the backward applies the inverse in place to `[dQ | dK]` in front of the projection's products.
    pub rope: Option<Rc<RotaryEmbedding>>,
    /// Sliding-window attention (the tested mirror is `nn::MultiheadAttention::window` in `host/neuronika.hpp`): query position `i`
    /// attends to the keys `max(0, i - window + 1) ..= i`.  `0` after `new`: off.  Read by `forward_step`, which then runs
    /// `nk_attention_decode_window_fwd` over a linear `KvCache` or a rolling one (`KvCache::new_rolling`).  The TRAINING forward with
    /// a window shorter than the sequence is not mirrored here (the packed node runs the fused core, which has no window): `forward`
    /// panics for it.
    pub window: usize,
}

impl MultiheadAttention {
    pub fn new(d_model: usize, heads: usize, p: f64, device: &Device) -> Self {
        assert!(heads > 0 && d_model % heads == 0, "d_model must be divisible by heads");
        assert!(matches!(d_model / heads, 32 | 64 | 128), "MultiheadAttention: head size must be 32, 64 or 128");
        // each of the three row blocks is initialised as its own Linear(d_model, d_model): U(-k, k), k = 1 / sqrt(d_model) -
        // the fan-in of the packed layer is d_model too, so one draw over (3 d, d) follows the same law
        Self { qkv: Linear::new(d_model, 3 * d_model, device), o: Linear::new(d_model, d_model, device), d_model, heads, dropout: Dropout::new(p),
               kv_heads: heads, causal: false, rope: None, window: 0 }
    }

    /// `new` with `kv_heads < heads` key / value heads shared by `heads / kv_heads` query heads each.
    pub fn new_grouped(d_model: usize, heads: usize, kv_heads: usize, p: f64, device: &Device) -> Self {
        assert!(kv_heads > 0 && kv_heads <= heads && heads % kv_heads == 0, "MultiheadAttention: kv_heads must be positive and divide heads");
        let mut layer = Self::new(d_model, heads, p, device);
        layer.qkv = Linear::new(d_model, d_model + 2 * (d_model / heads) * kv_heads, device);
        layer.kv_heads = kv_heads;
        layer
    }

    fn dkv(&self) -> usize {
        self.d_model / self.heads * self.kv_heads
    }

    /// Row range of the packed weight (and element range of the packed bias) holding the query / key / value projection.
    pub fn q_rows(&self) -> std::ops::Range<usize> {
        0..self.d_model
    }

    pub fn k_rows(&self) -> std::ops::Range<usize> {
        self.d_model..self.d_model + self.dkv()
    }

    pub fn v_rows(&self) -> std::ops::Range<usize> {
        self.d_model + self.dkv()..self.d_model + 2 * self.dkv()
    }

    /// `input`: `(batch * seq, d_model)`, rows of a sample contiguous.
    pub fn forward(&self, input: HipVarDiff<Ix2>, batch: usize) -> HipVarDiff<Ix2> {
        let rows = input.shape()[0];
        assert!(batch > 0 && rows % batch == 0, "MultiheadAttention: rows must be a multiple of batch");
        assert!(self.kv_heads == self.heads, "MultiheadAttention::forward: the packed node takes kv_heads == heads (see `kv_heads`)");
        let (seq, dh) = (rows / batch, self.d_model / self.heads);
        assert!(self.window == 0 || self.causal, "MultiheadAttention: a sliding window is a band of the causal triangle: set causal");
        assert!(self.window == 0 || seq <= self.window, "MultiheadAttention::forward: the packed node has no window shorter than the sequence (see `window`)");
        let scale = 1. / (dh as f32).sqrt();
        let packed = self.qkv.forward(input);
        let packed = match &self.rope {
            Some(r) => {
                assert!(r.table.head_dim() == dh && seq <= r.table.max_pos(), "MultiheadAttention: rope does not fit the head size or the sequence");
                packed.rope_in_place(&r.table, batch, 2 * self.heads)
            }
            None => packed,
        };
        let context = if self.causal {
            packed.packed_heads_attention_causal(batch, seq, self.heads, dh, scale, self.dropout.p, self.dropout.status.clone())
        } else {
            packed.packed_heads_attention(batch, seq, self.heads, dh, scale, self.dropout.p, self.dropout.status.clone())
        };
        self.o.forward(context)
    }

    /// Incremental decoding: the causal forward one slice of positions at a time, in inference.  `input` holds the NEW positions
    /// only, `(batch * rows, d_model)`; the packed projection, the append to `cache`, the single-query attention over the cached
    /// keys and the output projection run without keeping anything for a backward pass.  The cache's lengths advance here, when
    /// the graph is built.  Panics unless `causal` is set and dropout is inactive, or when the step exceeds the capacity.
    /// Unlike the C++ mirror (`host/neuronika.cpp`), which sends a fresh prefill of two or more rows through the causal core in
    /// its inference form, this method ALWAYS runs the append and the decode kernels, prefill included: the same values up to
    /// summation order, one kernel per (sample, head, row) instead of the tiled core.
    pub fn forward_step(&self, input: HipVar<Ix2>, batch: usize, cache: &KvCache) -> HipVar<Ix2> {
        assert!(self.causal, "MultiheadAttention::forward_step is the incremental form of the causal forward");
        assert!(!self.dropout.status.get() || self.dropout.p == 0., "MultiheadAttention::forward_step: dropout is active, call eval() first");
        let rows = input.shape()[0];
        assert!(batch > 0 && rows > 0 && rows % batch == 0, "MultiheadAttention: rows must be a multiple of batch");
        let dh = self.d_model / self.heads;
        let (cb, ch, capacity, cd) = cache.buffers.geometry();
        assert!((cb, ch, cd) == (batch, self.kv_heads, dh),
                "MultiheadAttention::forward_step: the cache holds {} heads, the layer has {} kv heads (of {} query heads)", ch, self.kv_heads, self.heads);
        let start = cache.lens();
        if cache.rolling() {
            assert!(self.window > 0, "MultiheadAttention::forward_step: a rolling cache keeps the last positions only: it needs a layer with window > 0");
            assert!(self.window + rows / batch - 1 <= capacity,
                    "MultiheadAttention::forward_step: window + T - 1 <= capacity on a rolling cache: chunk the prompt");
        } else {
            assert!(start.iter().all(|&l| l + rows / batch <= capacity), "MultiheadAttention::forward_step: the step exceeds the capacity");
        }
        let scale = 1. / (dh as f32).sqrt();
        let packed = input.linear(self.qkv.weight.detached(), self.qkv.bias.detached(), false);
        let packed = match &self.rope {
            Some(r) => {
                // a rolling cache's positions keep growing: they, not the capacity, must stay inside the table
                let fits = if cache.rolling() { start.iter().all(|&l| l + rows / batch <= r.table.max_pos()) } else { capacity <= r.table.max_pos() };
                assert!(r.table.head_dim() == dh && fits, "MultiheadAttention::forward_step: rope does not fit the head size or the capacity");
                packed.rope_in_place(&r.table, batch, self.heads + self.kv_heads, Some(&start))
            }
            None => packed,
        };
        let context = packed.packed_decode_attention(&cache.buffers, self.heads, &start, scale, self.window);
        if self.window > 0 {
            cache.window.set(self.window);
        }
        cache.advance(rows / batch);
        context.linear(self.o.weight.detached(), self.o.bias.detached(), false)
    }
}

/// The page table of a paged key / value cache, on the host (ours; the tested mirror is `nn::PageTable` in `host/neuronika.hpp`):
/// per sequence a length, a row of `max_pages` page ids (`-1`: none) and `behind`, the first position still held; per page a
/// reference count.  Every operation that can fail panics before it changes any state.
pub struct PageTable {
    pub num_pages: usize,
    pub page: usize,
    pub max_seqs: usize,
    pub max_pages: usize,
    lens: Vec<usize>,
    behind: Vec<usize>,
    rows: Vec<i32>,
    refs: Vec<usize>,
    free: std::collections::BTreeSet<usize>,
}

impl PageTable {
    pub fn new(num_pages: usize, page: usize, max_seqs: usize, max_pages: usize) -> Self {
        assert!(num_pages > 0 && max_seqs > 0 && max_pages > 0, "PageTable: num_pages, max_seqs and max_pages must be positive");
        assert!(page >= 16 && page.is_power_of_two(), "PageTable: page must be a power of two and at least 16");
        assert!(max_pages * page < (1usize << 31) - 1024, "PageTable: max_pages * page must stay below 2^31 - 1024");
        Self { num_pages, page, max_seqs, max_pages, lens: vec![0; max_seqs], behind: vec![0; max_seqs], rows: vec![-1; max_seqs * max_pages],
               refs: vec![0; num_pages], free: (0..num_pages).collect() }
    }

    pub fn lens(&self) -> &[usize] {
        &self.lens
    }

    /// `max_pages` ids, `-1` where the sequence owns nothing.
    pub fn row(&self, seq: usize) -> &[i32] {
        &self.rows[seq * self.max_pages..(seq + 1) * self.max_pages]
    }

    pub fn pages(&self, seq: usize) -> Vec<usize> {
        self.row(seq).iter().filter(|&&p| p >= 0).map(|&p| p as usize).collect()
    }

    pub fn refcount(&self, page: usize) -> usize {
        self.refs[page]
    }

    pub fn free_pages(&self) -> Vec<usize> {
        self.free.iter().copied().collect()
    }

    pub fn behind(&self, seq: usize) -> usize {
        self.behind[seq]
    }

    fn unref(&mut self, page: usize) {
        self.refs[page] -= 1;
        if self.refs[page] == 0 {
            self.free.insert(page);
        }
    }

    fn take(&mut self) -> usize {
        let page = *self.free.iter().next().expect("PageTable: a free page");
        self.free.remove(&page);
        self.refs[page] = 1;
        page
    }

    /// Grows every listed sequence by `rows` positions, in the order of `seqs`, lowest free page first.  A partial last page with
    /// another owner is replaced by a page of the sequence's own; the `(old, new)` pairs are the copies to make before the append.
    pub fn reserve(&mut self, seqs: &[usize], rows: usize) -> Vec<(usize, usize)> {
        assert!(rows > 0, "PageTable::reserve: rows must be positive");
        let mut left = std::collections::HashMap::<usize, usize>::new();
        let mut need = 0;
        for (i, &s) in seqs.iter().enumerate() {
            assert!(s < self.max_seqs, "PageTable::reserve: sequence id {} is outside [0, {})", s, self.max_seqs);
            assert!(!seqs[..i].contains(&s), "PageTable::reserve: sequence {} is listed twice", s);
            let (have, want) = ((self.lens[s] + self.page - 1) / self.page, (self.lens[s] + rows + self.page - 1) / self.page);
            assert!(want <= self.max_pages, "PageTable::reserve: sequence {} would exceed max_pages = {}", s, self.max_pages);
            need += want - have;
            if self.lens[s] % self.page != 0 {
                let last = self.rows[s * self.max_pages + have - 1] as usize;
                let gone = left.entry(last).or_insert(0);
                if self.refs[last] - *gone > 1 {
                    *gone += 1;
                    need += 1;
                }
            }
        }
        assert!(need <= self.free.len(), "PageTable::reserve: {} pages needed, {} are free", need, self.free.len());
        let mut copies = Vec::new();
        for &s in seqs {
            let (have, want) = ((self.lens[s] + self.page - 1) / self.page, (self.lens[s] + rows + self.page - 1) / self.page);
            if self.lens[s] % self.page != 0 {
                let old = self.rows[s * self.max_pages + have - 1] as usize;
                if self.refs[old] > 1 {
                    self.refs[old] -= 1;
                    let new = self.take();
                    self.rows[s * self.max_pages + have - 1] = new as i32;
                    copies.push((old, new));
                }
            }
            for i in have..want {
                self.rows[s * self.max_pages + i] = self.take() as i32;
            }
            self.lens[s] += rows;
        }
        copies
    }

    /// Releases the pages wholly past `len`.
    pub fn truncate(&mut self, seq: usize, len: usize) {
        assert!(seq < self.max_seqs && len <= self.lens[seq] && len >= self.behind[seq], "PageTable::truncate: sequence {} to length {}", seq, len);
        for i in (len + self.page - 1) / self.page..(self.lens[seq] + self.page - 1) / self.page {
            let p = self.rows[seq * self.max_pages + i];
            if p >= 0 {
                self.unref(p as usize);
                self.rows[seq * self.max_pages + i] = -1;
            }
        }
        self.lens[seq] = len;
    }

    pub fn release(&mut self, seq: usize) {
        assert!(seq < self.max_seqs, "PageTable::release: sequence id {}", seq);
        for i in 0..self.max_pages {
            let p = self.rows[seq * self.max_pages + i];
            if p >= 0 {
                self.unref(p as usize);
                self.rows[seq * self.max_pages + i] = -1;
            }
        }
        self.lens[seq] = 0;
        self.behind[seq] = 0;
    }

    /// `dst` must be empty: it shares every page of `src` by reference count and takes its length.
    pub fn fork(&mut self, src: usize, dst: usize) {
        assert!(src < self.max_seqs && dst < self.max_seqs && src != dst, "PageTable::fork: sequence ids {} -> {}", src, dst);
        assert!(self.lens[dst] == 0 && self.behind[dst] == 0, "PageTable::fork: sequence {} is not empty", dst);
        for i in 0..self.max_pages {
            let p = self.rows[src * self.max_pages + i];
            self.rows[dst * self.max_pages + i] = p;
            if p >= 0 {
                self.refs[p as usize] += 1;
            }
        }
        self.lens[dst] = self.lens[src];
        self.behind[dst] = self.behind[src];
    }

    /// Releases the pages wholly below `pos`: how a windowed layer bounds its memory.
    pub fn release_behind(&mut self, seq: usize, pos: usize) {
        assert!(seq < self.max_seqs && pos <= self.lens[seq], "PageTable::release_behind: sequence {} below {}", seq, pos);
        for i in 0..pos / self.page {
            let p = self.rows[seq * self.max_pages + i];
            if p >= 0 {
                self.unref(p as usize);
                self.rows[seq * self.max_pages + i] = -1;
            }
        }
        self.behind[seq] = self.behind[seq].max(pos / self.page * self.page);
    }

    pub fn reset(&mut self) {
        *self = Self::new(self.num_pages, self.page, self.max_seqs, self.max_pages);
    }
}

/// A paged key / value cache (ours; the tested mirror is `nn::PagedKvCache` in `host/neuronika.hpp`): the pools, a `PageTable`
/// and the decode scratch.
pub struct PagedKvCache {
    pub buffers: PagedBuffers,
    pub table: RefCell<PageTable>,
}

impl PagedKvCache {
    pub fn new(num_pages: usize, page: usize, kv_heads: usize, head_dim: usize, max_seqs: usize, max_pages: usize, device: &Device) -> Self {
        Self { buffers: PagedBuffers::new(num_pages, page, kv_heads, head_dim, max_pages, device),
               table: RefCell::new(PageTable::new(num_pages, page, max_seqs, max_pages)) }
    }

    pub fn lens(&self) -> Vec<usize> {
        self.table.borrow().lens().to_vec()
    }
}

impl MultiheadAttention {
    /// `forward_step` over a paged cache: the batch is `seqs.len()`, any subset of the cache's sequences in any order.  The pages
    /// of the step are reserved here, when the graph is built; the node's forward runs the page copies, the append and
    /// `nk_attention_decode_paged_fwd` with the layer's `window`.  Like `forward_step`, always on the decode kernels.
    pub fn forward_step_paged(&self, input: HipVar<Ix2>, seqs: &[usize], cache: &PagedKvCache) -> HipVar<Ix2> {
        assert!(self.causal, "MultiheadAttention::forward_step is the incremental form of the causal forward");
        assert!(!self.dropout.status.get() || self.dropout.p == 0., "MultiheadAttention::forward_step: dropout is active, call eval() first");
        let (rows, batch) = (input.shape()[0], seqs.len());
        assert!(batch > 0 && rows > 0 && rows % batch == 0, "MultiheadAttention: rows must be a multiple of the number of sequences");
        let dh = self.d_model / self.heads;
        let (_, ch, _, cd, max_pages) = cache.buffers.geometry();
        assert!((ch, cd) == (self.kv_heads, dh), "MultiheadAttention::forward_step: the cache holds {} heads, the layer has {} kv heads", ch, self.kv_heads);
        let mut table = cache.table.borrow_mut();
        assert!(seqs.iter().all(|&s| s < table.max_seqs), "MultiheadAttention::forward_step: a sequence id is out of range");
        let start: Vec<usize> = seqs.iter().map(|&s| table.lens()[s]).collect();
        for (&s, &l) in seqs.iter().zip(start.iter()) {
            let behind = table.behind(s);
            assert!(behind == 0 || (self.window > 0 && (l + 1).saturating_sub(self.window) >= behind),
                    "MultiheadAttention::forward_step: sequence {} released the pages below {}: the window must stay above them", s, behind);
        }
        if let Some(r) = &self.rope {
            assert!(r.table.head_dim() == dh && start.iter().all(|&l| l + rows / batch <= r.table.max_pos()),
                    "MultiheadAttention::forward_step: rope does not fit the head size or the positions");
        }
        let copies = table.reserve(seqs, rows / batch);
        let image: Vec<i32> = seqs.iter().flat_map(|&s| table.row(s).to_vec()).collect();
        debug_assert!(image.len() == batch * max_pages);
        let scale = 1. / (dh as f32).sqrt();
        let packed = input.linear(self.qkv.weight.detached(), self.qkv.bias.detached(), false);
        let packed = match &self.rope {
            Some(r) => packed.rope_in_place(&r.table, batch, self.heads + self.kv_heads, Some(&start)),
            None => packed,
        };
        let context = packed.packed_paged_decode_attention(&cache.buffers, self.heads, &start, &image, &copies, scale, self.window);
        context.linear(self.o.weight.detached(), self.o.bias.detached(), false)
    }
}
