use super::grad_id;
use std::rc::Rc;

use ndarray::{Dimension, Ix1};

use crate::{
    autograd::{Backward, Forward},
    gradient::Gradient,
    hip::{ffi, hiparray::HipArray},
    utils::Shared,
};

/// RMS normalisation over the trailing dimensions (`nk_rms_norm_fwd`; the reference has no such node): the input of dimension
/// `D` is read as `(rows, dim)`, `dim` the element count of `gamma` (dimension `E`, the normalised shape).  No centring and no
/// bias: `y = x * rstd * gamma`, `rstd = 1 / sqrt(sum(x * x) / dim + eps)`.  `stats` keeps `rstd` per row for the backward node;
/// the no-gradient form passes none.
pub(crate) struct RmsNorm<D: Dimension, E: Dimension> {
    operand_data: Shared<HipArray<D>>,
    gamma: Shared<HipArray<E>>,
    data: Shared<HipArray<D>>,
    stats: Option<Shared<HipArray<Ix1>>>,
    eps: f64,
}

impl<D: Dimension, E: Dimension> RmsNorm<D, E> {
    pub(crate) fn new(operand_data: Shared<HipArray<D>>, gamma: Shared<HipArray<E>>, data: Shared<HipArray<D>>,
                      stats: Option<Shared<HipArray<Ix1>>>, eps: f64) -> Self {
        Self { operand_data, gamma, data, stats, eps }
    }
}

impl<D: Dimension, E: Dimension> Forward for RmsNorm<D, E> {
    fn forward(&self) {
        let (x, gamma) = (self.operand_data.borrow(), self.gamma.borrow());
        let mut y = self.data.borrow_mut();
        let dim = gamma.len();
        let rows = x.len() / dim;
        let stats = match &self.stats {
            Some(s) => s.borrow_mut().as_mut_ptr(),
            None => std::ptr::null_mut(),
        };
        ffi::check(unsafe { ffi::nk_rms_norm_fwd(x.device().as_raw(), x.as_ptr(), gamma.as_ptr(), y.as_mut_ptr(), stats, rows as i64, dim as i32, self.eps) });
    }
}

/// ONE backward entry for the two operands: `dgamma += sum_rows g * xhat` (`nk_rms_norm_bwd_gamma`, no atomics) and
/// `dx += rstd * (gh - xhat * mean(gh * xhat))` (`nk_rms_norm_bwd`).  The input gradient is absent when the input is not
/// differentiable.  (This tape zeroes gradients eagerly, `+=` everywhere: the `_assign` twins of the C ABI serve the C++ tape's
/// lazily zeroed gradients.)
pub(crate) struct RmsNormBackward<D: Dimension, E: Dimension> {
    operand_data: Shared<HipArray<D>>,
    gamma: Shared<HipArray<E>>,
    stats: Shared<HipArray<Ix1>>,
    operand_gradient: Option<Rc<Gradient<HipArray<D>, D>>>,
    gamma_gradient: Rc<Gradient<HipArray<E>, E>>,
    gradient: Rc<Gradient<HipArray<D>, D>>,
}

impl<D: Dimension, E: Dimension> RmsNormBackward<D, E> {
    pub(crate) fn new(operand_data: Shared<HipArray<D>>, gamma: Shared<HipArray<E>>, stats: Shared<HipArray<Ix1>>,
                      operand_gradient: Option<Rc<Gradient<HipArray<D>, D>>>, gamma_gradient: Rc<Gradient<HipArray<E>, E>>,
                      gradient: Rc<Gradient<HipArray<D>, D>>) -> Self {
        Self { operand_data, gamma, stats, operand_gradient, gamma_gradient, gradient }
    }
}

impl<D: Dimension, E: Dimension> Backward for RmsNormBackward<D, E> {
    fn backward(&self) {
        let (g, x, gamma, stats) = (self.gradient.borrow(), self.operand_data.borrow(), self.gamma.borrow(), self.stats.borrow());
        let dev = g.device().as_raw();
        let dim = gamma.len();
        let rows = x.len() / dim;
        {
            let mut dgamma = self.gamma_gradient.borrow_mut();
            ffi::check(unsafe { ffi::nk_rms_norm_bwd_gamma(dev, dgamma.as_mut_ptr(), g.as_ptr(), x.as_ptr(), stats.as_ptr(), rows as i64, dim as i32) });
        }
        if let Some(operand_gradient) = &self.operand_gradient {
            let mut dx = operand_gradient.borrow_mut();
            ffi::check(unsafe {
                ffi::nk_rms_norm_bwd(dev, dx.as_mut_ptr(), g.as_ptr(), x.as_ptr(), gamma.as_ptr(), stats.as_ptr(), rows as i64, dim as i32)
            });
        }
    }

    /// The gradients this node accumulates into (`autograd.rs` extension: the last-writer rule of `backward_sync`).
    fn targets(&self) -> Vec<usize> {
        let mut t = vec![grad_id(&self.gamma_gradient)];
        if let Some(operand_gradient) = &self.operand_gradient {
            t.push(grad_id(operand_gradient));
        }
        t
    }
}
