use super::grad_id;
use std::rc::Rc;

use ndarray::{Dimension, Ix2};

use crate::{
    autograd::{Backward, Forward},
    gradient::Gradient,
    hip::{ffi, hiparray::HipArray},
    utils::Shared,
};

/// Rows of the `(V, D)` table selected by the ids of `indices` (`nk_embedding_fwd`; the reference has no such node; semantics in
/// `include/neuronika_hip.h`).  The ids are f32, read as the NLL targets are, in an array of any dimension `E`; the output has one
/// more axis, of extent `D`.  An id beyond the table yields a zero row.
pub(crate) struct Embedding<E: Dimension> {
    weight: Shared<HipArray<Ix2>>,
    indices: Shared<HipArray<E>>,
    data: Shared<HipArray<E::Larger>>,
}

impl<E: Dimension> Embedding<E> {
    pub(crate) fn new(weight: Shared<HipArray<Ix2>>, indices: Shared<HipArray<E>>, data: Shared<HipArray<E::Larger>>) -> Self {
        Self { weight, indices, data }
    }
}

impl<E: Dimension> Forward for Embedding<E> {
    fn forward(&self) {
        let (w, idx) = (self.weight.borrow(), self.indices.borrow());
        let mut y = self.data.borrow_mut();
        let s = w.shape_c();
        ffi::check(unsafe { ffi::nk_embedding_fwd(w.device().as_raw(), w.as_ptr(), idx.as_ptr(), y.as_mut_ptr(), idx.len() as i64, s[0] as i32, s[1] as i32) });
    }
}

/// `dweight[v, :] += ` the sum of the gradient rows of the tokens that selected row `v`, in ascending token order
/// (`nk_embedding_bwd`: an inverted index and one owner per table row, no atomics, bit-reproducible).  Ids equal to `padding_idx`
/// (negative: none) contribute nothing.  The ids are data: no gradient flows to them.  (This tape zeroes gradients eagerly, `+=`
/// everywhere: the `_assign` twin of the C ABI serves the C++ tape's lazily zeroed gradients.)
pub(crate) struct EmbeddingBackward<E: Dimension> {
    indices: Shared<HipArray<E>>,
    weight_gradient: Rc<Gradient<HipArray<Ix2>, Ix2>>,
    gradient: Rc<Gradient<HipArray<E::Larger>, E::Larger>>,
    padding_idx: i64,
}

impl<E: Dimension> EmbeddingBackward<E> {
    pub(crate) fn new(indices: Shared<HipArray<E>>, weight_gradient: Rc<Gradient<HipArray<Ix2>, Ix2>>,
                      gradient: Rc<Gradient<HipArray<E::Larger>, E::Larger>>, padding_idx: i64) -> Self {
        Self { indices, weight_gradient, gradient, padding_idx }
    }
}

impl<E: Dimension> Backward for EmbeddingBackward<E> {
    fn backward(&self) {
        let (g, idx) = (self.gradient.borrow(), self.indices.borrow());
        let mut dw = self.weight_gradient.borrow_mut();
        let s = dw.shape_c();
        ffi::check(unsafe {
            ffi::nk_embedding_bwd(g.device().as_raw(), dw.as_mut_ptr(), g.as_ptr(), idx.as_ptr(), idx.len() as i64, s[0] as i32, s[1] as i32, self.padding_idx)
        });
    }

    /// The gradient this node accumulates into (`autograd.rs` extension: the last-writer rule of `backward_sync`).
    fn targets(&self) -> Vec<usize> {
        vec![grad_id(&self.weight_gradient)]
    }
}
