use super::grad_id;
use std::rc::Rc;

use ndarray::Dimension;

use crate::{
    autograd::{Backward, Forward},
    gradient::Gradient,
    hip::{ffi, hiparray::HipArray},
    utils::Shared,
};

/// `(nd, x_shape)` of a pooled input `(N, C, spatial...)` for the C ABI.
fn pool_geometry<D: Dimension>(x: &HipArray<D>) -> (i32, Vec<i32>) {
    let s: Vec<i32> = x.shape_c().iter().map(|&e| e as i32).collect();
    assert!((3..=5).contains(&s.len()), "pooling: the input must be (N, C, spatial...) with 1 to 3 spatial axes");
    ((s.len() - 2) as i32, s)
}

/// Max pooling over the spatial axes of an `(N, C, spatial...)` input (`nk_max_pool_fwd`; the reference has no pooling; semantics in
/// `include/neuronika_hip.h`).  `indices` keeps, per output, the int32 offset of the selected element inside its own plane for the
/// backward node (the same four bytes per element as the f32 arrays of the tape); the no-gradient form passes none.
pub(crate) struct MaxPool<D: Dimension> {
    operand_data: Shared<HipArray<D>>,
    data: Shared<HipArray<D>>,
    indices: Option<Shared<HipArray<D>>>,
    kernel: Vec<i32>,
    stride: Vec<i32>,
    padding: Vec<i32>,
}

impl<D: Dimension> MaxPool<D> {
    pub(crate) fn new(operand_data: Shared<HipArray<D>>, data: Shared<HipArray<D>>, indices: Option<Shared<HipArray<D>>>, kernel: Vec<i32>,
                      stride: Vec<i32>, padding: Vec<i32>) -> Self {
        Self { operand_data, data, indices, kernel, stride, padding }
    }
}

impl<D: Dimension> Forward for MaxPool<D> {
    fn forward(&self) {
        let x = self.operand_data.borrow();
        let mut y = self.data.borrow_mut();
        let (nd, shape) = pool_geometry(&x);
        let idx = match &self.indices {
            Some(i) => i.borrow_mut().as_mut_ptr() as *mut i32,
            None => std::ptr::null_mut(),
        };
        ffi::check(unsafe {
            ffi::nk_max_pool_fwd(x.device().as_raw(), nd, x.as_ptr(), shape.as_ptr(), y.as_mut_ptr(), idx, self.kernel.as_ptr(), self.stride.as_ptr(), self.padding.as_ptr())
        });
    }
}

/// `dx[idx[o]] += g[o]` as a gather over the covering outputs (`nk_max_pool_bwd`): no atomics, bit-reproducible.
pub(crate) struct MaxPoolBackward<D: Dimension> {
    operand_gradient: Rc<Gradient<HipArray<D>, D>>,
    indices: Shared<HipArray<D>>,
    gradient: Rc<Gradient<HipArray<D>, D>>,
    kernel: Vec<i32>,
    stride: Vec<i32>,
    padding: Vec<i32>,
}

impl<D: Dimension> MaxPoolBackward<D> {
    pub(crate) fn new(operand_gradient: Rc<Gradient<HipArray<D>, D>>, indices: Shared<HipArray<D>>, gradient: Rc<Gradient<HipArray<D>, D>>,
                      kernel: Vec<i32>, stride: Vec<i32>, padding: Vec<i32>) -> Self {
        Self { operand_gradient, indices, gradient, kernel, stride, padding }
    }
}

impl<D: Dimension> Backward for MaxPoolBackward<D> {
    fn backward(&self) {
        let (g, idx) = (self.gradient.borrow(), self.indices.borrow());
        let mut dx = self.operand_gradient.borrow_mut();
        let (nd, shape) = pool_geometry(&dx);
        ffi::check(unsafe {
            ffi::nk_max_pool_bwd(g.device().as_raw(), nd, dx.as_mut_ptr(), shape.as_ptr(), g.as_ptr(), idx.as_ptr() as *const i32, self.kernel.as_ptr(), self.stride.as_ptr(), self.padding.as_ptr())
        });
    }

    fn targets(&self) -> Vec<usize> {
        vec![grad_id(&self.operand_gradient)]
    }
}

/// Average pooling (`nk_avg_pool_fwd`): the row-major f32 sum of the in-range positions over `prod k_i` (`count_include_pad`) or over
/// their number.  Global average pooling is this node with `kernel = stride =` the spatial extents.
pub(crate) struct AvgPool<D: Dimension> {
    operand_data: Shared<HipArray<D>>,
    data: Shared<HipArray<D>>,
    kernel: Vec<i32>,
    stride: Vec<i32>,
    padding: Vec<i32>,
    count_include_pad: bool,
}

impl<D: Dimension> AvgPool<D> {
    pub(crate) fn new(operand_data: Shared<HipArray<D>>, data: Shared<HipArray<D>>, kernel: Vec<i32>, stride: Vec<i32>, padding: Vec<i32>,
                      count_include_pad: bool) -> Self {
        Self { operand_data, data, kernel, stride, padding, count_include_pad }
    }
}

impl<D: Dimension> Forward for AvgPool<D> {
    fn forward(&self) {
        let x = self.operand_data.borrow();
        let mut y = self.data.borrow_mut();
        let (nd, shape) = pool_geometry(&x);
        ffi::check(unsafe {
            ffi::nk_avg_pool_fwd(x.device().as_raw(), nd, x.as_ptr(), shape.as_ptr(), y.as_mut_ptr(), self.kernel.as_ptr(), self.stride.as_ptr(), self.padding.as_ptr(), self.count_include_pad as i32)
        });
    }
}

/// `dx[i] += sum over the windows holding i of g[o] / divisor(o)` (`nk_avg_pool_bwd`).
pub(crate) struct AvgPoolBackward<D: Dimension> {
    operand_gradient: Rc<Gradient<HipArray<D>, D>>,
    gradient: Rc<Gradient<HipArray<D>, D>>,
    kernel: Vec<i32>,
    stride: Vec<i32>,
    padding: Vec<i32>,
    count_include_pad: bool,
}

impl<D: Dimension> AvgPoolBackward<D> {
    pub(crate) fn new(operand_gradient: Rc<Gradient<HipArray<D>, D>>, gradient: Rc<Gradient<HipArray<D>, D>>, kernel: Vec<i32>, stride: Vec<i32>,
                      padding: Vec<i32>, count_include_pad: bool) -> Self {
        Self { operand_gradient, gradient, kernel, stride, padding, count_include_pad }
    }
}

impl<D: Dimension> Backward for AvgPoolBackward<D> {
    fn backward(&self) {
        let g = self.gradient.borrow();
        let mut dx = self.operand_gradient.borrow_mut();
        let (nd, shape) = pool_geometry(&dx);
        ffi::check(unsafe {
            ffi::nk_avg_pool_bwd(g.device().as_raw(), nd, dx.as_mut_ptr(), shape.as_ptr(), g.as_ptr(), self.kernel.as_ptr(), self.stride.as_ptr(), self.padding.as_ptr(), self.count_include_pad as i32)
        });
    }

    fn targets(&self) -> Vec<usize> {
        vec![grad_id(&self.operand_gradient)]
    }
}
