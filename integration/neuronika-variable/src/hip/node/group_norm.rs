use super::grad_id;
use std::rc::Rc;

use ndarray::{Dimension, Ix1, Ix2};

use crate::{
    autograd::{Backward, Forward},
    gradient::Gradient,
    hip::{ffi, hiparray::HipArray},
    utils::Shared,
};

/// `(N, C, L)` of a group-normalised input: `L` the product of the extents behind the channel axis.
fn group_norm_geometry<D: Dimension>(x: &HipArray<D>) -> (i64, i32, i64) {
    let s = x.shape_c();
    assert!(s.len() >= 2, "group_norm: the input must have at least two dimensions (N, C, ...)");
    (s[0] as i64, s[1] as i32, s[2..].iter().map(|&e| e as i64).product())
}

/// Group normalisation of an `(N, C, spatial...)` input over `groups` channel groups (`nk_group_norm_fwd`; the reference has no
/// such node): each `(sample, group)` is normalised over its `C / groups` channels and all positions, then scaled and shifted per
/// channel by `gamma` / `beta` of shape `(C)`.  `groups == C` is instance normalisation.  `stats` keeps `{mean, rstd}` per
/// `(sample, group)` for the backward node; the no-gradient form passes none.
pub(crate) struct GroupNorm<D: Dimension> {
    operand_data: Shared<HipArray<D>>,
    gamma: Shared<HipArray<Ix1>>,
    beta: Shared<HipArray<Ix1>>,
    data: Shared<HipArray<D>>,
    stats: Option<Shared<HipArray<Ix2>>>,
    groups: usize,
    eps: f64,
}

impl<D: Dimension> GroupNorm<D> {
    #[allow(clippy::too_many_arguments)]
    pub(crate) fn new(operand_data: Shared<HipArray<D>>, gamma: Shared<HipArray<Ix1>>, beta: Shared<HipArray<Ix1>>, data: Shared<HipArray<D>>,
                      stats: Option<Shared<HipArray<Ix2>>>, groups: usize, eps: f64) -> Self {
        Self { operand_data, gamma, beta, data, stats, groups, eps }
    }
}

impl<D: Dimension> Forward for GroupNorm<D> {
    fn forward(&self) {
        let (x, gamma, beta) = (self.operand_data.borrow(), self.gamma.borrow(), self.beta.borrow());
        let mut y = self.data.borrow_mut();
        let (n, c, l) = group_norm_geometry(&x);
        let stats = match &self.stats {
            Some(s) => s.borrow_mut().as_mut_ptr(),
            None => std::ptr::null_mut(),
        };
        ffi::check(unsafe {
            ffi::nk_group_norm_fwd(x.device().as_raw(), x.as_ptr(), gamma.as_ptr(), beta.as_ptr(), y.as_mut_ptr(), stats, n, c, l, self.groups as i32, self.eps)
        });
    }
}

/// ONE backward entry for the three operands: `dgamma[c] += sum_{n, l} g * xhat` and `dbeta[c] += sum_{n, l} g` leave one pass
/// together (`nk_group_norm_bwd_params`, no atomics), `dx += rstd * (gh - mean(gh) - xhat * mean(gh * xhat))` its own
/// (`nk_group_norm_bwd`).  The input gradient is absent when the input is not differentiable.  (`+=` everywhere, as in
/// `LayerNormBackward`.)
pub(crate) struct GroupNormBackward<D: Dimension> {
    operand_data: Shared<HipArray<D>>,
    gamma: Shared<HipArray<Ix1>>,
    stats: Shared<HipArray<Ix2>>,
    groups: usize,
    operand_gradient: Option<Rc<Gradient<HipArray<D>, D>>>,
    gamma_gradient: Rc<Gradient<HipArray<Ix1>, Ix1>>,
    beta_gradient: Rc<Gradient<HipArray<Ix1>, Ix1>>,
    gradient: Rc<Gradient<HipArray<D>, D>>,
}

impl<D: Dimension> GroupNormBackward<D> {
    #[allow(clippy::too_many_arguments)]
    pub(crate) fn new(operand_data: Shared<HipArray<D>>, gamma: Shared<HipArray<Ix1>>, stats: Shared<HipArray<Ix2>>, groups: usize,
                      operand_gradient: Option<Rc<Gradient<HipArray<D>, D>>>, gamma_gradient: Rc<Gradient<HipArray<Ix1>, Ix1>>,
                      beta_gradient: Rc<Gradient<HipArray<Ix1>, Ix1>>, gradient: Rc<Gradient<HipArray<D>, D>>) -> Self {
        Self { operand_data, gamma, stats, groups, operand_gradient, gamma_gradient, beta_gradient, gradient }
    }
}

impl<D: Dimension> Backward for GroupNormBackward<D> {
    fn backward(&self) {
        let (g, x, gamma, stats) = (self.gradient.borrow(), self.operand_data.borrow(), self.gamma.borrow(), self.stats.borrow());
        let dev = g.device().as_raw();
        let (n, c, l) = group_norm_geometry(&x);
        let groups = self.groups as i32;
        {
            let (mut dgamma, mut dbeta) = (self.gamma_gradient.borrow_mut(), self.beta_gradient.borrow_mut());
            ffi::check(unsafe {
                ffi::nk_group_norm_bwd_params(dev, dgamma.as_mut_ptr(), dbeta.as_mut_ptr(), g.as_ptr(), x.as_ptr(), stats.as_ptr(), n, c, l, groups)
            });
        }
        if let Some(operand_gradient) = &self.operand_gradient {
            let mut dx = operand_gradient.borrow_mut();
            ffi::check(unsafe { ffi::nk_group_norm_bwd(dev, dx.as_mut_ptr(), g.as_ptr(), x.as_ptr(), gamma.as_ptr(), stats.as_ptr(), n, c, l, groups) });
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
