use super::grad_id;
use std::rc::Rc;

use ndarray::Ix2;

use crate::{
    autograd::{Backward, Forward},
    gradient::Gradient,
    hip::{ffi, hiparray::HipArray},
    utils::Shared,
};

/// The geometry of one `nk_repeat_kv_*` launch (semantics in `include/neuronika_hip.h`): `rows` rows, `kv_heads` heads of `dh` floats
/// each written `groups` times - head `k` becomes heads `k * groups .. k * groups + groups - 1`.  Both operands are contiguous here:
/// the row strides are `kv_heads * dh` and `kv_heads * groups * dh`.
#[derive(Clone, Copy)]
pub(crate) struct RepeatKvGeometry {
    pub(crate) rows: i32,
    pub(crate) kv_heads: i32,
    pub(crate) groups: i32,
    pub(crate) dh: i32,
}

/// Grouped-query attention, the training / prefill side (`nk_repeat_kv_fwd`; ours: the reference has one head count): the keys or
/// values of `kv_heads` heads repeated for the `kv_heads * groups` query heads the attention core runs on.  A bit-exact copy.
pub(crate) struct RepeatKv {
    geometry: RepeatKvGeometry,
    operand_data: Shared<HipArray<Ix2>>,
    data: Shared<HipArray<Ix2>>,
}

impl RepeatKv {
    pub(crate) fn new(geometry: RepeatKvGeometry, operand_data: Shared<HipArray<Ix2>>, data: Shared<HipArray<Ix2>>) -> Self {
        Self { geometry, operand_data, data }
    }
}

impl Forward for RepeatKv {
    fn forward(&self) {
        let x = self.operand_data.borrow();
        let mut y = self.data.borrow_mut();
        let g = self.geometry;
        ffi::check(unsafe {
            ffi::nk_repeat_kv_fwd(x.device().as_raw(), x.as_ptr(), g.kv_heads * g.dh, y.as_mut_ptr(), g.kv_heads * g.groups * g.dh, g.rows,
                                  g.kv_heads, g.groups, g.dh)
        });
    }
}

/// `dx += ((g_0 + g_1) + g_2) + ...` over the copies in ascending order (`nk_repeat_kv_bwd`): the node keeps the geometry and nothing
/// of its input.
pub(crate) struct RepeatKvBackward {
    geometry: RepeatKvGeometry,
    operand_gradient: Rc<Gradient<HipArray<Ix2>, Ix2>>,
    gradient: Rc<Gradient<HipArray<Ix2>, Ix2>>,
}

impl RepeatKvBackward {
    pub(crate) fn new(geometry: RepeatKvGeometry, operand_gradient: Rc<Gradient<HipArray<Ix2>, Ix2>>, gradient: Rc<Gradient<HipArray<Ix2>, Ix2>>) -> Self {
        Self { geometry, operand_gradient, gradient }
    }
}

impl Backward for RepeatKvBackward {
    fn backward(&self) {
        let gr = self.gradient.borrow();
        let mut dx = self.operand_gradient.borrow_mut();
        let g = self.geometry;
        ffi::check(unsafe {
            ffi::nk_repeat_kv_bwd(gr.device().as_raw(), dx.as_mut_ptr(), g.kv_heads * g.dh, gr.as_ptr(), g.kv_heads * g.groups * g.dh, g.rows,
                                  g.kv_heads, g.groups, g.dh)
        });
    }

    /// The gradient this node accumulates into (`autograd.rs` extension: the last-writer rule of `backward_sync`).
    fn targets(&self) -> Vec<usize> {
        vec![grad_id(&self.operand_gradient)]
    }
}
