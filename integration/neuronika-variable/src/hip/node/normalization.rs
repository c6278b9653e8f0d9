use super::grad_id;
use std::{cell::Cell, rc::Rc};

use ndarray::{Dimension, Ix1, Ix2};

use crate::{
    autograd::{Backward, Forward},
    gradient::Gradient,
    hip::{ffi, hiparray::HipArray},
    utils::Shared,
};

/// Layer normalisation over the trailing dimensions (`nk_layer_norm_fwd`; the reference has no such node): the input of
/// dimension `D` is read as `(rows, dim)`, `dim` the element count of `gamma` / `beta` (dimension `E`, the normalised shape).
/// `stats` keeps `{mean, rstd}` per row for the backward node; the no-gradient form passes none.
pub(crate) struct LayerNorm<D: Dimension, E: Dimension> {
    operand_data: Shared<HipArray<D>>,
    gamma: Shared<HipArray<E>>,
    beta: Shared<HipArray<E>>,
    data: Shared<HipArray<D>>,
    stats: Option<Shared<HipArray<Ix2>>>,
    eps: f64,
}

impl<D: Dimension, E: Dimension> LayerNorm<D, E> {
    pub(crate) fn new(operand_data: Shared<HipArray<D>>, gamma: Shared<HipArray<E>>, beta: Shared<HipArray<E>>, data: Shared<HipArray<D>>,
                      stats: Option<Shared<HipArray<Ix2>>>, eps: f64) -> Self {
        Self { operand_data, gamma, beta, data, stats, eps }
    }
}

impl<D: Dimension, E: Dimension> Forward for LayerNorm<D, E> {
    fn forward(&self) {
        let (x, gamma, beta) = (self.operand_data.borrow(), self.gamma.borrow(), self.beta.borrow());
        let mut y = self.data.borrow_mut();
        let dim = gamma.len();
        let rows = x.len() / dim;
        let stats = match &self.stats {
            Some(s) => s.borrow_mut().as_mut_ptr(),
            None => std::ptr::null_mut(),
        };
        ffi::check(unsafe {
            ffi::nk_layer_norm_fwd(x.device().as_raw(), x.as_ptr(), gamma.as_ptr(), beta.as_ptr(), y.as_mut_ptr(), stats, rows as i64, dim as i32, self.eps)
        });
    }
}

/// ONE backward entry for the three operands: `dgamma += sum_rows g * xhat` and `dbeta += sum_rows g` leave one pass together
/// (`nk_layer_norm_bwd_params`), `dx += rstd * (gh - mean(gh) - xhat * mean(gh * xhat))` its own (`nk_layer_norm_bwd`).  The input
/// gradient is absent when the input is not differentiable.  (This tape zeroes gradients eagerly, `+=` everywhere: the `_assign`
/// twins of the C ABI serve the C++ tape's lazily zeroed gradients.)
pub(crate) struct LayerNormBackward<D: Dimension, E: Dimension> {
    operand_data: Shared<HipArray<D>>,
    gamma: Shared<HipArray<E>>,
    stats: Shared<HipArray<Ix2>>,
    operand_gradient: Option<Rc<Gradient<HipArray<D>, D>>>,
    gamma_gradient: Rc<Gradient<HipArray<E>, E>>,
    beta_gradient: Rc<Gradient<HipArray<E>, E>>,
    gradient: Rc<Gradient<HipArray<D>, D>>,
}

impl<D: Dimension, E: Dimension> LayerNormBackward<D, E> {
    #[allow(clippy::too_many_arguments)]
    pub(crate) fn new(operand_data: Shared<HipArray<D>>, gamma: Shared<HipArray<E>>, stats: Shared<HipArray<Ix2>>,
                      operand_gradient: Option<Rc<Gradient<HipArray<D>, D>>>, gamma_gradient: Rc<Gradient<HipArray<E>, E>>,
                      beta_gradient: Rc<Gradient<HipArray<E>, E>>, gradient: Rc<Gradient<HipArray<D>, D>>) -> Self {
        Self { operand_data, gamma, stats, operand_gradient, gamma_gradient, beta_gradient, gradient }
    }
}

impl<D: Dimension, E: Dimension> Backward for LayerNormBackward<D, E> {
    fn backward(&self) {
        let (g, x, gamma, stats) = (self.gradient.borrow(), self.operand_data.borrow(), self.gamma.borrow(), self.stats.borrow());
        let dev = g.device().as_raw();
        let dim = gamma.len();
        let rows = x.len() / dim;
        {
            let (mut dgamma, mut dbeta) = (self.gamma_gradient.borrow_mut(), self.beta_gradient.borrow_mut());
            ffi::check(unsafe {
                ffi::nk_layer_norm_bwd_params(dev, dgamma.as_mut_ptr(), dbeta.as_mut_ptr(), g.as_ptr(), x.as_ptr(), stats.as_ptr(), rows as i64, dim as i32)
            });
        }
        if let Some(operand_gradient) = &self.operand_gradient {
            let mut dx = operand_gradient.borrow_mut();
            ffi::check(unsafe {
                ffi::nk_layer_norm_bwd(dev, dx.as_mut_ptr(), g.as_ptr(), x.as_ptr(), gamma.as_ptr(), stats.as_ptr(), rows as i64, dim as i32)
            });
        }
    }

    /// The gradients this node accumulates into (`autograd.rs` extension: the last-writer rule of `backward_sync`).
    fn targets(&self) -> Vec<usize> {
        let mut t = vec![grad_id(&self.gamma_gradient), grad_id(&self.beta_gradient)];
        if let Some(operand_gradient) = &self.operand_gradient {
            t.push(grad_id(operand_gradient));
        }
        t
    }
}

/// `(N, C, L)` of a batch-normalised input: `L` the product of the extents behind the channel axis.
fn batch_norm_geometry<D: Dimension>(x: &HipArray<D>) -> (i32, i32, i32) {
    let s = x.shape_c();
    assert!(s.len() >= 2, "batch_norm: the input must have at least two dimensions (N, C, ...)");
    (s[0] as i32, s[1] as i32, s[2..].iter().map(|&e| e as i32).product())
}

/// Batch normalisation over `(N, spatial...)` for each channel of an `(N, C, spatial...)` input (`nk_batch_norm_fwd` /
/// `nk_batch_norm_infer_fwd`; the reference has no such node).  `status` is read each time the node runs, as Dropout's is: `true`
/// normalises with the batch statistics and moves the running ones (when there are any) towards them in place, `false` normalises
/// with the running ones.  Without running statistics the batch's serve in both modes.  `stats` keeps `{mean, rstd}` per channel
/// for the backward node, `trained` the mode of the last run.
pub(crate) struct BatchNorm<D: Dimension> {
    operand_data: Shared<HipArray<D>>,
    gamma: Shared<HipArray<Ix1>>,
    beta: Shared<HipArray<Ix1>>,
    running: Option<(Shared<HipArray<Ix1>>, Shared<HipArray<Ix1>>)>,
    data: Shared<HipArray<D>>,
    stats: Option<Shared<HipArray<Ix2>>>,
    eps: f64,
    momentum: f64,
    status: Rc<Cell<bool>>,
    trained: Rc<Cell<bool>>,
}

impl<D: Dimension> BatchNorm<D> {
    #[allow(clippy::too_many_arguments)]
    pub(crate) fn new(operand_data: Shared<HipArray<D>>, gamma: Shared<HipArray<Ix1>>, beta: Shared<HipArray<Ix1>>,
                      running: Option<(Shared<HipArray<Ix1>>, Shared<HipArray<Ix1>>)>, data: Shared<HipArray<D>>,
                      stats: Option<Shared<HipArray<Ix2>>>, eps: f64, momentum: f64, status: Rc<Cell<bool>>, trained: Rc<Cell<bool>>) -> Self {
        Self { operand_data, gamma, beta, running, data, stats, eps, momentum, status, trained }
    }
}

impl<D: Dimension> Forward for BatchNorm<D> {
    fn forward(&self) {
        let (x, gamma, beta) = (self.operand_data.borrow(), self.gamma.borrow(), self.beta.borrow());
        let mut y = self.data.borrow_mut();
        let (n, c, l) = batch_norm_geometry(&x);
        let stats = match &self.stats {
            Some(s) => s.borrow_mut().as_mut_ptr(),
            None => std::ptr::null_mut(),
        };
        let train = self.status.get() || self.running.is_none();
        self.trained.set(train);
        let dev = x.device().as_raw();
        match (&self.running, train) {
            (Some((mean, var)), true) => {
                let (mut mean, mut var) = (mean.borrow_mut(), var.borrow_mut());
                ffi::check(unsafe {
                    ffi::nk_batch_norm_fwd(dev, x.as_ptr(), gamma.as_ptr(), beta.as_ptr(), y.as_mut_ptr(), stats, mean.as_mut_ptr(), var.as_mut_ptr(), n, c, l, self.eps, self.momentum)
                });
            }
            (Some((mean, var)), false) => {
                let (mean, var) = (mean.borrow(), var.borrow());
                ffi::check(unsafe {
                    ffi::nk_batch_norm_infer_fwd(dev, x.as_ptr(), gamma.as_ptr(), beta.as_ptr(), mean.as_ptr(), var.as_ptr(), y.as_mut_ptr(), stats, n, c, l, self.eps)
                });
            }
            (None, _) => ffi::check(unsafe {
                ffi::nk_batch_norm_fwd(dev, x.as_ptr(), gamma.as_ptr(), beta.as_ptr(), y.as_mut_ptr(), stats, std::ptr::null_mut(), std::ptr::null_mut(), n, c, l, self.eps, self.momentum)
            }),
        }
    }
}

/// ONE backward entry for the three operands: one reduction pass (`nk_batch_norm_bwd_sums`) leaves `{sum g, sum g * xhat}` per
/// channel in `sums`, which both parameter gradients (`nk_batch_norm_bwd_params`) and, in training, the input gradient
/// (`nk_batch_norm_bwd`; without `sums` its inference form) read.  The input gradient is absent when the input is not
/// differentiable.  (`+=` everywhere, as in `LayerNormBackward`.)
pub(crate) struct BatchNormBackward<D: Dimension> {
    operand_data: Shared<HipArray<D>>,
    gamma: Shared<HipArray<Ix1>>,
    stats: Shared<HipArray<Ix2>>,
    sums: Shared<HipArray<Ix2>>,
    trained: Rc<Cell<bool>>,
    operand_gradient: Option<Rc<Gradient<HipArray<D>, D>>>,
    gamma_gradient: Rc<Gradient<HipArray<Ix1>, Ix1>>,
    beta_gradient: Rc<Gradient<HipArray<Ix1>, Ix1>>,
    gradient: Rc<Gradient<HipArray<D>, D>>,
}

impl<D: Dimension> BatchNormBackward<D> {
    #[allow(clippy::too_many_arguments)]
    pub(crate) fn new(operand_data: Shared<HipArray<D>>, gamma: Shared<HipArray<Ix1>>, stats: Shared<HipArray<Ix2>>, sums: Shared<HipArray<Ix2>>,
                      trained: Rc<Cell<bool>>, operand_gradient: Option<Rc<Gradient<HipArray<D>, D>>>,
                      gamma_gradient: Rc<Gradient<HipArray<Ix1>, Ix1>>, beta_gradient: Rc<Gradient<HipArray<Ix1>, Ix1>>,
                      gradient: Rc<Gradient<HipArray<D>, D>>) -> Self {
        Self { operand_data, gamma, stats, sums, trained, operand_gradient, gamma_gradient, beta_gradient, gradient }
    }
}

impl<D: Dimension> Backward for BatchNormBackward<D> {
    fn backward(&self) {
        let (g, x, gamma, stats) = (self.gradient.borrow(), self.operand_data.borrow(), self.gamma.borrow(), self.stats.borrow());
        let dev = g.device().as_raw();
        let (n, c, l) = batch_norm_geometry(&x);
        let mut sums = self.sums.borrow_mut();
        ffi::check(unsafe { ffi::nk_batch_norm_bwd_sums(dev, sums.as_mut_ptr(), g.as_ptr(), x.as_ptr(), stats.as_ptr(), n, c, l) });
        {
            let (mut dgamma, mut dbeta) = (self.gamma_gradient.borrow_mut(), self.beta_gradient.borrow_mut());
            ffi::check(unsafe { ffi::nk_batch_norm_bwd_params(dev, dgamma.as_mut_ptr(), dbeta.as_mut_ptr(), sums.as_ptr(), c) });
        }
        if let Some(operand_gradient) = &self.operand_gradient {
            let mut dx = operand_gradient.borrow_mut();
            let sums_ptr = if self.trained.get() { sums.as_ptr() } else { std::ptr::null() };
            ffi::check(unsafe {
                ffi::nk_batch_norm_bwd(dev, dx.as_mut_ptr(), g.as_ptr(), x.as_ptr(), gamma.as_ptr(), stats.as_ptr(), sums_ptr, n, c, l)
            });
        }
    }

    /// The gradients this node accumulates into (`autograd.rs` extension: the last-writer rule of `backward_sync`).
    fn targets(&self) -> Vec<usize> {
        let mut t = vec![grad_id(&self.gamma_gradient), grad_id(&self.beta_gradient)];
        if let Some(operand_gradient) = &self.operand_gradient {
            t.push(grad_id(operand_gradient));
        }
        t
    }
}
