use ndarray::{Ix1, Ix2};

use crate::{
    autograd::Forward,
    hip::{ffi, hiparray::HipArray},
    utils::Shared,
};

/// `L(bits)`: `nk_quant_linear_fwd` takes its rows kernels for up to this many rows of `x` by rule (`nk_quant_linear_rows_rule`).
pub(crate) fn quant_linear_rows_rule(bits: i32) -> usize {
    (unsafe { ffi::nk_quant_linear_rows_rule(bits) }) as usize
}

/// The packed image of an `(out, in)` weight (format at `nk_quant_linear_*` in `include/neuronika_hip.h`): int8 / int4 rows as opaque
/// f32 words and the per-group f32 scales, `group` in {32, 64, 128} or 0 for one group per row.
#[derive(Clone)]
pub(crate) struct QuantWeight {
    pub(crate) qweight: Shared<HipArray<Ix1>>,
    pub(crate) scales: Shared<HipArray<Ix1>>,
    pub(crate) out_features: usize,
    pub(crate) in_features: usize,
    pub(crate) bits: i32,
    pub(crate) group: i32,
}

impl QuantWeight {
    /// Floats of the packed weight and of its scales; `None` for a geometry the entry points refuse.
    pub(crate) fn sizes(out_features: usize, in_features: usize, bits: i32, group: i32) -> Option<(usize, usize)> {
        let words = unsafe { ffi::nk_quant_linear_words(out_features as i32, in_features as i32, bits) };
        let scales = unsafe { ffi::nk_quant_linear_scales(out_features as i32, in_features as i32, group) };
        if words == 0 || scales == 0 { None } else { Some((words, scales)) }
    }

    /// Quantise `weight` on the device into `self` (`nk_quant_linear_pack`).
    pub(crate) fn pack(&self, weight: &HipArray<Ix2>) {
        let mut q = self.qweight.borrow_mut();
        let mut s = self.scales.borrow_mut();
        ffi::check(unsafe {
            ffi::nk_quant_linear_pack(weight.device().as_raw(), weight.as_ptr(), self.in_features as i32, q.as_mut_ptr(), s.as_mut_ptr(),
                                      self.out_features as i32, self.in_features as i32, self.bits, self.group)
        });
    }

    /// The values `float(q) * s` the forward multiplies by, into an `(out, in)` array (`nk_quant_linear_unpack`).
    pub(crate) fn unpack(&self, weight: &mut HipArray<Ix2>) {
        let q = self.qweight.borrow();
        let s = self.scales.borrow();
        ffi::check(unsafe {
            ffi::nk_quant_linear_unpack(q.device().as_raw(), q.as_ptr(), s.as_ptr(), weight.as_mut_ptr(), self.in_features as i32,
                                        self.out_features as i32, self.in_features as i32, self.bits, self.group)
        });
    }
}

/// Weight-only quantised Linear (ours: the reference has no such layer): `(rows, in) -> (rows, out)` on the packed integer weights,
/// f32 activations and accumulation (`nk_quant_linear_fwd`).  Inference only: there is no backward node.
pub(crate) struct QuantLinear {
    weight: QuantWeight,
    bias: Option<Shared<HipArray<Ix1>>>,
    rows: usize,
    input: Shared<HipArray<Ix2>>,
    data: Shared<HipArray<Ix2>>,
}

impl QuantLinear {
    pub(crate) fn new(weight: QuantWeight, bias: Option<Shared<HipArray<Ix1>>>, rows: usize, input: Shared<HipArray<Ix2>>,
                      data: Shared<HipArray<Ix2>>) -> Self {
        Self { weight, bias, rows, input, data }
    }
}

impl Forward for QuantLinear {
    fn forward(&self) {
        let x = self.input.borrow();
        let mut y = self.data.borrow_mut();
        let (q, s) = (self.weight.qweight.borrow(), self.weight.scales.borrow());
        let bias = self.bias.as_ref().map(|b| b.borrow());
        let (n, k) = (self.weight.out_features as i32, self.weight.in_features as i32);
        ffi::check(unsafe {
            ffi::nk_quant_linear_fwd(x.device().as_raw(), x.as_ptr(), k, q.as_ptr(), s.as_ptr(), bias.as_ref().map_or(std::ptr::null(), |b| b.as_ptr()),
                                     y.as_mut_ptr(), n, self.rows as i32, n, k, self.weight.bits, self.weight.group)
        });
    }
}
