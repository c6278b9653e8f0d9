use super::grad_id;
use std::rc::Rc;

use ndarray::Dimension;

use crate::{
    autograd::{Backward, Forward},
    gradient::Gradient,
    hip::{ffi, hiparray::HipArray},
    utils::Shared,
};

/// The resampling rule of `nk_upsample_*` (`enum { NK_UPSAMPLE_NEAREST, NK_UPSAMPLE_LINEAR }` of the header; the generated `ffi.rs`
/// carries prototypes and `#define`s only).  `Linear` is bilinear over two spatial axes and trilinear over three.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub(crate) enum UpsampleMode {
    Nearest = 0,
    Linear = 1,
}

/// What both nodes pass to the C ABI besides the pointers: the output extents, the mode and `align_corners` (linear only).
#[derive(Clone, Debug)]
pub(crate) struct UpsampleGeometry {
    pub(crate) out_size: Vec<i32>,
    pub(crate) mode: UpsampleMode,
    pub(crate) align_corners: bool,
}

/// `(nd, x_shape)` of a resampled input `(N, C, spatial...)` for the C ABI.
fn upsample_input<D: Dimension>(x: &HipArray<D>) -> (i32, Vec<i32>) {
    let s: Vec<i32> = x.shape_c().iter().map(|&e| e as i32).collect();
    assert!((3..=5).contains(&s.len()), "upsample: the input must be (N, C, spatial...) with 1 to 3 spatial axes");
    ((s.len() - 2) as i32, s)
}

/// Nearest or linear resampling of the spatial axes of an `(N, C, spatial...)` input (`nk_upsample_fwd`; the reference has no such
/// node; semantics in `include/neuronika_hip.h`).
pub(crate) struct Upsample<D: Dimension> {
    operand_data: Shared<HipArray<D>>,
    data: Shared<HipArray<D>>,
    geometry: UpsampleGeometry,
}

impl<D: Dimension> Upsample<D> {
    pub(crate) fn new(operand_data: Shared<HipArray<D>>, data: Shared<HipArray<D>>, geometry: UpsampleGeometry) -> Self {
        Self { operand_data, data, geometry }
    }
}

impl<D: Dimension> Forward for Upsample<D> {
    fn forward(&self) {
        let x = self.operand_data.borrow();
        let mut y = self.data.borrow_mut();
        let (nd, shape) = upsample_input(&x);
        let q = &self.geometry;
        ffi::check(unsafe {
            ffi::nk_upsample_fwd(x.device().as_raw(), nd, q.mode as i32, q.align_corners as i32, x.as_ptr(), shape.as_ptr(), y.as_mut_ptr(), q.out_size.as_ptr())
        });
    }
}

/// `dx[i] += sum of w * g[o]` over the outputs that read `i`, as a gather in ascending order of `o` (`nk_upsample_bwd`): no atomics,
/// bit-reproducible, the weights those of the forward to the bit.
pub(crate) struct UpsampleBackward<D: Dimension> {
    operand_gradient: Rc<Gradient<HipArray<D>, D>>,
    gradient: Rc<Gradient<HipArray<D>, D>>,
    geometry: UpsampleGeometry,
}

impl<D: Dimension> UpsampleBackward<D> {
    pub(crate) fn new(operand_gradient: Rc<Gradient<HipArray<D>, D>>, gradient: Rc<Gradient<HipArray<D>, D>>, geometry: UpsampleGeometry) -> Self {
        Self { operand_gradient, gradient, geometry }
    }
}

impl<D: Dimension> Backward for UpsampleBackward<D> {
    fn backward(&self) {
        let g = self.gradient.borrow();
        let mut dx = self.operand_gradient.borrow_mut();
        let (nd, shape) = upsample_input(&dx);
        let q = &self.geometry;
        ffi::check(unsafe {
            ffi::nk_upsample_bwd(g.device().as_raw(), nd, q.mode as i32, q.align_corners as i32, dx.as_mut_ptr(), shape.as_ptr(), g.as_ptr(), q.out_size.as_ptr())
        });
    }

    fn targets(&self) -> Vec<usize> {
        vec![grad_id(&self.operand_gradient)]
    }
}
