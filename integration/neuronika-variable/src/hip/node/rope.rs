use super::grad_id;
use std::rc::Rc;

use ndarray::{Ix1, Ix2, Ix3};

use crate::{
    autograd::{Backward, Forward},
    gradient::Gradient,
    hip::{device::Device, ffi, hiparray::HipArray},
    utils::Shared,
};

/// The geometry of one rotary launch (`nk_rope_*`; semantics in `include/neuronika_hip.h`): `batch * rows` rows of row stride `ld`
/// floats, `heads` heads of `dh` floats from column 0, the first `rot` columns of each rotated.  `heads = 2 * H`, `ld = 3 * H * dh`
/// addresses the Q|K blocks of a packed projection output.
#[derive(Clone, Copy)]
pub(crate) struct RopeGeometry {
    pub(crate) batch: i32,
    pub(crate) rows: i32,
    pub(crate) heads: i32,
    pub(crate) dh: i32,
    pub(crate) rot: i32,
    pub(crate) max_pos: i32,
    pub(crate) interleaved: i32,
    pub(crate) ld: i32,
}

/// The `(max_pos, rot / 2, 2)` table of `(cos, sin)` of `p * base^(-2j/rot)` (`nk_rope_table`: f64 on the host, rounded once).
pub(crate) fn rope_table(max_pos: usize, rot: usize, base: f64, device: &Device) -> HipArray<Ix3> {
    let mut table = HipArray::zeroed(ndarray::Dim([max_pos, rot / 2, 2]), device.clone());
    ffi::check(unsafe { ffi::nk_rope_table(device.as_raw(), table.as_mut_ptr(), max_pos as i32, rot as i32, base) });
    table
}

/// Rotary position embedding of a `(batch*rows, heads*dh)` value at positions `0 .. rows - 1`, out of place (`nk_rope_fwd`; ours: the
/// reference has no position encoding).
pub(crate) struct Rope {
    geometry: RopeGeometry,
    table: Shared<HipArray<Ix3>>,
    operand_data: Shared<HipArray<Ix2>>,
    data: Shared<HipArray<Ix2>>,
}

impl Rope {
    pub(crate) fn new(geometry: RopeGeometry, table: Shared<HipArray<Ix3>>, operand_data: Shared<HipArray<Ix2>>, data: Shared<HipArray<Ix2>>) -> Self {
        Self { geometry, table, operand_data, data }
    }
}

impl Forward for Rope {
    fn forward(&self) {
        let (x, t) = (self.operand_data.borrow(), self.table.borrow());
        let mut y = self.data.borrow_mut();
        let g = self.geometry;
        ffi::check(unsafe {
            ffi::nk_rope_fwd(x.device().as_raw(), x.as_ptr(), g.ld, y.as_mut_ptr(), g.ld, t.as_ptr(), std::ptr::null(), g.batch, g.rows, g.heads,
                             g.dh, g.rot, g.max_pos, g.interleaved)
        });
    }
}

/// `dx += R^T g` (`nk_rope_bwd`): the rotation is orthogonal, so the node keeps the table and the geometry and nothing of its input.
pub(crate) struct RopeBackward {
    geometry: RopeGeometry,
    table: Shared<HipArray<Ix3>>,
    operand_gradient: Rc<Gradient<HipArray<Ix2>, Ix2>>,
    gradient: Rc<Gradient<HipArray<Ix2>, Ix2>>,
}

impl RopeBackward {
    pub(crate) fn new(geometry: RopeGeometry, table: Shared<HipArray<Ix3>>, operand_gradient: Rc<Gradient<HipArray<Ix2>, Ix2>>,
                      gradient: Rc<Gradient<HipArray<Ix2>, Ix2>>) -> Self {
        Self { geometry, table, operand_gradient, gradient }
    }
}

impl Backward for RopeBackward {
    fn backward(&self) {
        let (gr, t) = (self.gradient.borrow(), self.table.borrow());
        let mut dx = self.operand_gradient.borrow_mut();
        let g = self.geometry;
        ffi::check(unsafe {
            ffi::nk_rope_bwd(gr.device().as_raw(), dx.as_mut_ptr(), g.ld, gr.as_ptr(), g.ld, t.as_ptr(), std::ptr::null(), g.batch, g.rows, g.heads,
                             g.dh, g.rot, g.max_pos, g.interleaved)
        });
    }

    /// The gradient this node accumulates into (`autograd.rs` extension: the last-writer rule of `backward_sync`).
    fn targets(&self) -> Vec<usize> {
        vec![grad_id(&self.operand_gradient)]
    }
}

/// The rotation IN PLACE in the buffer another node has just written - the Q|K blocks of a packed projection output - at positions
/// `start[b] + t` (`start`: `batch` int32 lengths in f32 cells, as `nk_kv_cache_append` takes them) or `t`.  The node's output IS
/// its operand: it sits on the tape right behind the projection.
pub(crate) struct RopeInPlace {
    geometry: RopeGeometry,
    table: Shared<HipArray<Ix3>>,
    data: Shared<HipArray<Ix2>>,
    start: Option<HipArray<Ix1>>,
}

impl RopeInPlace {
    pub(crate) fn new(geometry: RopeGeometry, table: Shared<HipArray<Ix3>>, data: Shared<HipArray<Ix2>>, start: Option<HipArray<Ix1>>) -> Self {
        Self { geometry, table, data, start }
    }
}

impl Forward for RopeInPlace {
    fn forward(&self) {
        let t = self.table.borrow();
        let mut x = self.data.borrow_mut();
        let g = self.geometry;
        let start = self.start.as_ref().map_or(std::ptr::null(), |s| s.as_ptr() as *const i32);
        let p = x.as_mut_ptr();
        ffi::check(unsafe {
            ffi::nk_rope_fwd(x.device().as_raw(), p as *const f32, g.ld, p, g.ld, t.as_ptr(), start, g.batch, g.rows, g.heads, g.dh, g.rot,
                             g.max_pos, g.interleaved)
        });
    }
}

/// The inverse rotation in place in the gradient of that buffer (`nk_rope_bwd_assign` with `dx == g`): it runs after the attention
/// node has written `[dQ | dK | dV]` and before the projection's products read it.
pub(crate) struct RopeInPlaceBackward {
    geometry: RopeGeometry,
    table: Shared<HipArray<Ix3>>,
    gradient: Rc<Gradient<HipArray<Ix2>, Ix2>>,
}

impl RopeInPlaceBackward {
    pub(crate) fn new(geometry: RopeGeometry, table: Shared<HipArray<Ix3>>, gradient: Rc<Gradient<HipArray<Ix2>, Ix2>>) -> Self {
        Self { geometry, table, gradient }
    }
}

impl Backward for RopeInPlaceBackward {
    fn backward(&self) {
        let t = self.table.borrow();
        let mut dx = self.gradient.borrow_mut();
        let g = self.geometry;
        let p = dx.as_mut_ptr();
        ffi::check(unsafe {
            ffi::nk_rope_bwd_assign(dx.device().as_raw(), p, g.ld, p as *const f32, g.ld, t.as_ptr(), std::ptr::null(), g.batch, g.rows, g.heads,
                                    g.dh, g.rot, g.max_pos, g.interleaved)
        });
    }

    /// The gradient this node rewrites (`autograd.rs` extension: the last-writer rule of `backward_sync`).
    fn targets(&self) -> Vec<usize> {
        vec![grad_id(&self.gradient)]
    }
}
