use std::{cell::Cell, rc::Rc};

use ndarray::{Ix1, Ix2};

use crate::{
    autograd::Forward,
    hip::{ffi, hiparray::HipArray},
    utils::Shared,
};

/// The largest vocabulary whose row the sampling kernel keeps in LDS (`nk_sample_stage_limit`): a constant of the library.
pub(crate) fn sample_stage_limit() -> usize {
    (unsafe { ffi::nk_sample_stage_limit() }) as usize
}

/// What one sampling launch draws with (semantics at `nk_sample_fwd` in `include/neuronika_hip.h`): greedy at `temperature == 0`,
/// else temperature, top-k (`0`: off) and top-p (`1`: off) in that order and one Philox draw per row at `(seed, offset)`.
#[derive(Clone, Copy)]
pub(crate) struct SampleParams {
    pub(crate) temperature: f32,
    pub(crate) top_k: i32,
    pub(crate) top_p: f32,
    pub(crate) seed: u64,
}

/// Token sampling on the device (ours: the reference has no generation loop): the ids, as f32, of the LAST of `rows` positions of
/// every sample of `(batch * rows, vocab)` logits - `logits + (rows - 1) * vocab` with row stride `rows * vocab`.  Every forward
/// that was issued consumes one offset of the counter its sampler shares with it.  Inference only: there is no backward node.
pub(crate) struct Sample {
    params: SampleParams,
    offset: Rc<Cell<u64>>,
    batch: i32,
    rows: usize,
    vocab: usize,
    logits: Shared<HipArray<Ix2>>,
    data: Shared<HipArray<Ix1>>,
}

impl Sample {
    pub(crate) fn new(params: SampleParams, offset: Rc<Cell<u64>>, batch: i32, rows: usize, vocab: usize, logits: Shared<HipArray<Ix2>>,
                      data: Shared<HipArray<Ix1>>) -> Self {
        Self { params, offset, batch, rows, vocab, logits, data }
    }
}

impl Forward for Sample {
    fn forward(&self) {
        let x = self.logits.borrow();
        let mut ids = self.data.borrow_mut();
        let p = self.params;
        ffi::check(unsafe {
            ffi::nk_sample_fwd(x.device().as_raw(), x.as_ptr().add((self.rows - 1) * self.vocab), (self.rows * self.vocab) as i64, self.batch,
                               self.vocab as i32, ids.as_mut_ptr(), p.temperature, p.top_k, p.top_p, p.seed, self.offset.get())
        });
        self.offset.set(self.offset.get() + 1);
    }
}
