use ndarray::{Ix1, Ix2};

use crate::{
    autograd::Forward,
    hip::{ffi, hiparray::HipArray},
    utils::Shared,
};

/// The MXFP4 image of an `(out, in)` weight (format at `nk_quant_mx_*` in `include/neuronika_hip.h`): E2M1 codes, two to a byte, and
/// one E8M0 scale byte per 32 consecutive inputs of a row, both as opaque f32 words.
#[derive(Clone)]
pub(crate) struct MxWeight {
    pub(crate) qweight: Shared<HipArray<Ix1>>,
    pub(crate) scales: Shared<HipArray<Ix1>>,
    pub(crate) out_features: usize,
    pub(crate) in_features: usize,
}

impl MxWeight {
    /// Floats of the codes and of the scale bytes; `None` for a geometry the entry points refuse (`in` not a multiple of 32).
    pub(crate) fn sizes(out_features: usize, in_features: usize) -> Option<(usize, usize)> {
        let words = unsafe { ffi::nk_quant_mx_words(out_features as i32, in_features as i32) };
        let scales = unsafe { ffi::nk_quant_mx_scales(out_features as i32, in_features as i32) };
        if words == 0 || scales == 0 { None } else { Some((words, scales)) }
    }

    /// Quantise `weight` on the device into `self` (`nk_quant_mx_pack`).
    pub(crate) fn pack(&self, weight: &HipArray<Ix2>) {
        let mut q = self.qweight.borrow_mut();
        let mut s = self.scales.borrow_mut();
        ffi::check(unsafe {
            ffi::nk_quant_mx_pack(weight.device().as_raw(), weight.as_ptr(), self.in_features as i32, q.as_mut_ptr(), s.as_mut_ptr(),
                                  self.out_features as i32, self.in_features as i32)
        });
    }

    /// The values `element * 2^(e - 127)` the forward multiplies by, into an `(out, in)` array (`nk_quant_mx_unpack`).
    pub(crate) fn unpack(&self, weight: &mut HipArray<Ix2>) {
        let q = self.qweight.borrow();
        let s = self.scales.borrow();
        ffi::check(unsafe {
            ffi::nk_quant_mx_unpack(q.device().as_raw(), q.as_ptr(), s.as_ptr(), weight.as_mut_ptr(), self.in_features as i32,
                                    self.out_features as i32, self.in_features as i32)
        });
    }
}

/// Microscaling Linear (ours: the reference has no such layer): `(rows, in) -> (rows, out)` on the MXFP4 weights, the rows of `x`
/// quantised to MXFP8 on the fly, on the block-scaled matrix instruction (`nk_quant_mx_linear_fwd`).  Inference only: there is no
/// backward node.
pub(crate) struct MxLinear {
    weight: MxWeight,
    bias: Option<Shared<HipArray<Ix1>>>,
    rows: usize,
    input: Shared<HipArray<Ix2>>,
    data: Shared<HipArray<Ix2>>,
}

impl MxLinear {
    pub(crate) fn new(weight: MxWeight, bias: Option<Shared<HipArray<Ix1>>>, rows: usize, input: Shared<HipArray<Ix2>>,
                      data: Shared<HipArray<Ix2>>) -> Self {
        Self { weight, bias, rows, input, data }
    }
}

impl Forward for MxLinear {
    fn forward(&self) {
        let x = self.input.borrow();
        let mut y = self.data.borrow_mut();
        let (q, s) = (self.weight.qweight.borrow(), self.weight.scales.borrow());
        let bias = self.bias.as_ref().map(|b| b.borrow());
        let (n, k) = (self.weight.out_features as i32, self.weight.in_features as i32);
        let b = bias.as_ref().map_or(std::ptr::null(), |b| b.as_ptr());
        ffi::check(unsafe {
            ffi::nk_quant_mx_linear_fwd(x.device().as_raw(), x.as_ptr(), k, q.as_ptr(), s.as_ptr(), b, y.as_mut_ptr(), n, self.rows as i32, n, k)
        });
    }
}
