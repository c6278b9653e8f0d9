use super::grad_id;
use std::rc::Rc;

use ndarray::{Dimension, Ix0, RemoveAxis};

use crate::{
    autograd::{Backward, Forward},
    gradient::Gradient,
    hip::{ffi, hiparray::HipArray},
    utils::Shared,
    Reduction,
};

/// Cross entropy of the class logits `(N, C, d1..dk)` against the ids of `target` `(N, d1..dk)`, f32 read as the NLL targets are
/// (`nk_cross_entropy_fwd`; the reference stops at `nll`; semantics in `include/neuronika_hip.h`): log-softmax and NLL in one pass
/// over the logits.  The node owns `lse`, one float per position, which is all the backward needs besides the logits.
pub(crate) struct CrossEntropy<D: Dimension + RemoveAxis> {
    input_data: Shared<HipArray<D>>,
    target_data: Shared<HipArray<D::Smaller>>,
    lse: Shared<HipArray<D::Smaller>>,
    data: Shared<HipArray<Ix0>>,
    reduction: Reduction,
    ignore_index: i64,
    label_smoothing: f64,
}

impl<D: Dimension + RemoveAxis> CrossEntropy<D> {
    pub(crate) fn new(input_data: Shared<HipArray<D>>, target_data: Shared<HipArray<D::Smaller>>, lse: Shared<HipArray<D::Smaller>>,
                      data: Shared<HipArray<Ix0>>, reduction: Reduction, ignore_index: i64, label_smoothing: f64) -> Self {
        Self { input_data, target_data, lse, data, reduction, ignore_index, label_smoothing }
    }
}

impl<D: Dimension + RemoveAxis> Forward for CrossEntropy<D> {
    fn forward(&self) {
        let (x, t) = (self.input_data.borrow(), self.target_data.borrow());
        let (mut lse, mut out) = (self.lse.borrow_mut(), self.data.borrow_mut());
        let s = x.shape_c();
        let red = matches!(self.reduction, Reduction::Mean) as i32;
        ffi::check(unsafe {
            ffi::nk_cross_entropy_fwd(x.device().as_raw(), x.as_ptr(), t.as_ptr(), s.as_ptr(), s.len() as i32, red, self.ignore_index, self.label_smoothing, lse.as_mut_ptr(), out.as_mut_ptr())
        });
    }
}

/// `dx += g w (softmax(x) - (1 - e) onehot(target) - e / C)` per active position, `w` = 1 or 1 / active count
/// (`nk_cross_entropy_bwd`): the softmax is recomputed as `exp(x - lse)`; inactive positions are not touched.  (This tape zeroes
/// gradients eagerly, `+=` everywhere: the `_assign` twin of the C ABI serves the C++ tape's lazily zeroed gradients.)
pub(crate) struct CrossEntropyBackward<D: Dimension + RemoveAxis> {
    input_data: Shared<HipArray<D>>,
    target_data: Shared<HipArray<D::Smaller>>,
    lse: Shared<HipArray<D::Smaller>>,
    input_gradient: Rc<Gradient<HipArray<D>, D>>,
    gradient: Rc<Gradient<HipArray<Ix0>, Ix0>>,
    reduction: Reduction,
    ignore_index: i64,
    label_smoothing: f64,
}

impl<D: Dimension + RemoveAxis> CrossEntropyBackward<D> {
    pub(crate) fn new(input_data: Shared<HipArray<D>>, target_data: Shared<HipArray<D::Smaller>>, lse: Shared<HipArray<D::Smaller>>,
                      input_gradient: Rc<Gradient<HipArray<D>, D>>, gradient: Rc<Gradient<HipArray<Ix0>, Ix0>>, reduction: Reduction,
                      ignore_index: i64, label_smoothing: f64) -> Self {
        Self { input_data, target_data, lse, input_gradient, gradient, reduction, ignore_index, label_smoothing }
    }
}

impl<D: Dimension + RemoveAxis> Backward for CrossEntropyBackward<D> {
    fn backward(&self) {
        let (g, x, t, lse) = (self.gradient.borrow(), self.input_data.borrow(), self.target_data.borrow(), self.lse.borrow());
        let mut dx = self.input_gradient.borrow_mut();
        let s = x.shape_c();
        let red = matches!(self.reduction, Reduction::Mean) as i32;
        ffi::check(unsafe {
            ffi::nk_cross_entropy_bwd(g.device().as_raw(), dx.as_mut_ptr(), g.as_ptr(), x.as_ptr(), t.as_ptr(), lse.as_ptr(), s.as_ptr(), s.len() as i32, red, self.ignore_index, self.label_smoothing)
        });
    }

    /// The gradient this node accumulates into (`autograd.rs` extension: the last-writer rule of `backward_sync`).
    fn targets(&self) -> Vec<usize> {
        vec![grad_id(&self.input_gradient)]
    }
}
