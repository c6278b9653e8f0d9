use super::grad_id;
use std::rc::Rc;

use ndarray::Dimension;

use crate::{
    autograd::{Backward, Forward},
    gradient::Gradient,
    hip::{ffi, hiparray::HipArray},
    utils::Shared,
};

/// A smooth activation over every element (`nk_activation_fwd`; the reference has no such node; semantics in
/// `include/neuronika_hip.h`): `act` is a value of `enum nk_activation` - GELU (erfc form), GELU (tanh form), SiLU or sigmoid.
pub(crate) struct Activation<D: Dimension> {
    operand_data: Shared<HipArray<D>>,
    data: Shared<HipArray<D>>,
    act: i32,
}

impl<D: Dimension> Activation<D> {
    pub(crate) fn new(operand_data: Shared<HipArray<D>>, data: Shared<HipArray<D>>, act: i32) -> Self {
        Self { operand_data, data, act }
    }
}

impl<D: Dimension> Forward for Activation<D> {
    fn forward(&self) {
        let x = self.operand_data.borrow();
        let mut y = self.data.borrow_mut();
        ffi::check(unsafe { ffi::nk_activation_fwd(x.device().as_raw(), self.act, x.as_ptr(), y.as_mut_ptr(), x.len()) });
    }
}

/// `dx += g * act'(x)` (`nk_activation_bwd`): the node keeps its INPUT and the derivative is recomputed from it.  (This tape zeroes
/// gradients eagerly, `+=` everywhere: the `_assign` twin of the C ABI serves the C++ tape's lazily zeroed gradients.)
pub(crate) struct ActivationBackward<D: Dimension> {
    operand_data: Shared<HipArray<D>>,
    operand_gradient: Rc<Gradient<HipArray<D>, D>>,
    gradient: Rc<Gradient<HipArray<D>, D>>,
    act: i32,
}

impl<D: Dimension> ActivationBackward<D> {
    pub(crate) fn new(operand_gradient: Rc<Gradient<HipArray<D>, D>>, operand_data: Shared<HipArray<D>>, gradient: Rc<Gradient<HipArray<D>, D>>,
                      act: i32) -> Self {
        Self { operand_data, operand_gradient, gradient, act }
    }
}

impl<D: Dimension> Backward for ActivationBackward<D> {
    fn backward(&self) {
        let (g, x) = (self.gradient.borrow(), self.operand_data.borrow());
        let mut dx = self.operand_gradient.borrow_mut();
        ffi::check(unsafe { ffi::nk_activation_bwd(g.device().as_raw(), self.act, dx.as_mut_ptr(), g.as_ptr(), x.as_ptr(), x.len()) });
    }

    /// The gradient this node accumulates into (`autograd.rs` extension: the last-writer rule of `backward_sync`).
    fn targets(&self) -> Vec<usize> {
        vec![grad_id(&self.operand_gradient)]
    }
}

/// The gated form over the two halves of the last axis (`nk_glu_fwd`): `y[r, j] = x[r, j] * act(x[r, H + j])`, `x` of `(rows, 2 H)`,
/// `y` of `(rows, H)`.  Sigmoid is GLU, GELU is GeGLU, SiLU is SwiGLU.
pub(crate) struct Glu<D: Dimension> {
    operand_data: Shared<HipArray<D>>,
    data: Shared<HipArray<D>>,
    act: i32,
    half: usize,
}

impl<D: Dimension> Glu<D> {
    pub(crate) fn new(operand_data: Shared<HipArray<D>>, data: Shared<HipArray<D>>, act: i32, half: usize) -> Self {
        Self { operand_data, data, act, half }
    }
}

impl<D: Dimension> Forward for Glu<D> {
    fn forward(&self) {
        let x = self.operand_data.borrow();
        let mut y = self.data.borrow_mut();
        let rows = (y.len() / self.half) as i64;
        ffi::check(unsafe { ffi::nk_glu_fwd(x.device().as_raw(), self.act, x.as_ptr(), y.as_mut_ptr(), rows, self.half as i32) });
    }
}

/// `dx[r, j] += g * act(b)`, `dx[r, H + j] += g * a * act'(b)` (`nk_glu_bwd`), recomputed from the node's INPUT.
pub(crate) struct GluBackward<D: Dimension> {
    operand_data: Shared<HipArray<D>>,
    operand_gradient: Rc<Gradient<HipArray<D>, D>>,
    gradient: Rc<Gradient<HipArray<D>, D>>,
    act: i32,
    half: usize,
}

impl<D: Dimension> GluBackward<D> {
    pub(crate) fn new(operand_gradient: Rc<Gradient<HipArray<D>, D>>, operand_data: Shared<HipArray<D>>, gradient: Rc<Gradient<HipArray<D>, D>>,
                      act: i32, half: usize) -> Self {
        Self { operand_data, operand_gradient, gradient, act, half }
    }
}

impl<D: Dimension> Backward for GluBackward<D> {
    fn backward(&self) {
        let (g, x) = (self.gradient.borrow(), self.operand_data.borrow());
        let mut dx = self.operand_gradient.borrow_mut();
        let rows = (g.len() / self.half) as i64;
        ffi::check(unsafe { ffi::nk_glu_bwd(g.device().as_raw(), self.act, dx.as_mut_ptr(), g.as_ptr(), x.as_ptr(), rows, self.half as i32) });
    }

    /// The gradient this node accumulates into (`autograd.rs` extension: the last-writer rule of `backward_sync`).
    fn targets(&self) -> Vec<usize> {
        vec![grad_id(&self.operand_gradient)]
    }
}
