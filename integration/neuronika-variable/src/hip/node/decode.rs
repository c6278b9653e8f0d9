use ndarray::{Ix1, Ix2, Ix4};

use super::attention::Heads;
use crate::{
    autograd::Forward,
    hip::{ffi, hiparray::HipArray},
    utils::Shared,
};

/// Keys one partial problem of the split-KV decode kernel covers (`nk_attention_decode_chunk`): a constant of the library per
/// head size, never a function of the device or the batch.
pub(crate) fn decode_chunk(dh: usize) -> usize {
    (unsafe { ffi::nk_attention_decode_chunk(dh as i32) }) as usize
}

/// Floats of scratch `nk_attention_decode_fwd` needs for `rows` new positions per sample (`nk_attention_decode_workspace`).
pub(crate) fn decode_workspace(batch: usize, rows: usize, heads: usize, dh: usize, capacity: usize) -> usize {
    unsafe { ffi::nk_attention_decode_workspace(batch as i32, rows as i32, heads as i32, dh as i32, capacity as i32) }
}

/// Floats of scratch `nk_attention_decode_window_fwd` needs (`nk_attention_decode_window_workspace`): a function of the window,
/// never of the capacity.
pub(crate) fn decode_window_workspace(batch: usize, rows: usize, heads: usize, dh: usize, window: usize) -> usize {
    unsafe { ffi::nk_attention_decode_window_workspace(batch as i32, rows as i32, heads as i32, dh as i32, window as i32) }
}

/// One step of incremental decoding over PACKED projections (ours: the reference has no such node; semantics in
/// `include/neuronika_hip.h`): `packed` is the `(batch*rows, 3*heads*dh)` output of one `Linear` over `[Wq; Wk; Wv]` for the NEW
/// positions only - `(batch*rows, (query_heads + 2*heads)*dh)` for a grouped-query layer, where `geometry.heads` counts the kv heads
/// the caches hold and `query_heads` (a multiple of it) the heads of Q and of the output.  The forward appends its key and value blocks to the `(batch, heads, capacity, dh)` caches at
/// `start[b] + t` (`nk_kv_cache_append`) and lets every new row attend to the keys `< start[b] + t + 1` of its sample
/// (`nk_attention_decode_fwd`: split-KV partials merged in chunk order, no atomics; `nk_attention_decode_gqa_fwd` when
/// `query_heads > heads`: the query heads of a group share one read of their keys and values).  `start` is fixed when the node is built,
/// so a second `forward()` writes the same rows to the same places.  Inference only: there is no backward node.
/// Sliding window (`window > 0`): every new row attends to the keys `max(0, n - window) .. n - 1`, `n = start[b] + t + 1`, through
/// `nk_attention_decode_window_fwd` - at most `window` keys per kv head whatever the length.  `ring`: the caches are rolling, position
/// `p` lives at slot `p % capacity` (`nk_kv_cache_append_ring`; `window + rows - 1 <= capacity`, checked where the node is built).
pub(crate) struct PackedDecodeAttention {
    geometry: Heads, // `seq` = new rows per sample, `heads` = kv heads
    query_heads: i32,
    capacity: i32,
    window: i32, // 0: off
    ring: bool,
    packed: Shared<HipArray<Ix2>>,
    keys: Shared<HipArray<Ix4>>,
    values: Shared<HipArray<Ix4>>,
    start: HipArray<Ix1>, // `batch` int32 lengths in f32 cells
    workspace: Shared<HipArray<Ix1>>,
    data: Shared<HipArray<Ix2>>,
    scale: f32,
}

impl PackedDecodeAttention {
    #[allow(clippy::too_many_arguments)]
    pub(crate) fn new(geometry: Heads, query_heads: i32, capacity: i32, window: i32, ring: bool, packed: Shared<HipArray<Ix2>>,
                      keys: Shared<HipArray<Ix4>>, values: Shared<HipArray<Ix4>>, start: HipArray<Ix1>, workspace: Shared<HipArray<Ix1>>,
                      data: Shared<HipArray<Ix2>>, scale: f32) -> Self {
        Self { geometry, query_heads, capacity, window, ring, packed, keys, values, start, workspace, data, scale }
    }
}

impl Forward for PackedDecodeAttention {
    fn forward(&self) {
        let qkv = self.packed.borrow();
        let (mut kc, mut vc) = (self.keys.borrow_mut(), self.values.borrow_mut());
        let mut ws = self.workspace.borrow_mut();
        let mut out = self.data.borrow_mut();
        let h = self.geometry;
        let (d, dkv) = ((self.query_heads * h.dh) as usize, (h.heads * h.dh) as usize);
        let ld = (d + 2 * dkv) as i32;
        let start = self.start.as_ptr() as *const i32;
        let dev = qkv.device().as_raw();
        if self.ring {
            ffi::check(unsafe {
                ffi::nk_kv_cache_append_ring(dev, kc.as_mut_ptr(), vc.as_mut_ptr(), qkv.as_ptr().add(d), qkv.as_ptr().add(d + dkv), ld, start,
                                             h.batch, h.seq, h.heads, h.dh, self.capacity)
            });
        } else {
            ffi::check(unsafe {
                ffi::nk_kv_cache_append(dev, kc.as_mut_ptr(), vc.as_mut_ptr(), qkv.as_ptr().add(d), qkv.as_ptr().add(d + dkv), ld, start,
                                        h.batch, h.seq, h.heads, h.dh, self.capacity)
            });
        }
        if self.window > 0 {
            ffi::check(unsafe {
                ffi::nk_attention_decode_window_fwd(dev, qkv.as_ptr(), ld, kc.as_ptr(), vc.as_ptr(), start, out.as_mut_ptr(), ws.as_mut_ptr(),
                                                    h.batch, h.seq, self.query_heads, h.heads, h.dh, self.capacity, self.window,
                                                    self.ring as i32, self.scale)
            });
        } else if self.query_heads == h.heads {
            ffi::check(unsafe {
                ffi::nk_attention_decode_fwd(dev, qkv.as_ptr(), ld, kc.as_ptr(), vc.as_ptr(), start, out.as_mut_ptr(), ws.as_mut_ptr(),
                                             h.batch, h.seq, h.heads, h.dh, self.capacity, self.scale)
            });
        } else {
            ffi::check(unsafe {
                ffi::nk_attention_decode_gqa_fwd(dev, qkv.as_ptr(), ld, kc.as_ptr(), vc.as_ptr(), start, out.as_mut_ptr(), ws.as_mut_ptr(),
                                                 h.batch, h.seq, self.query_heads, h.heads, h.dh, self.capacity, self.scale)
            });
        }
    }
}

/// Floats of scratch `nk_attention_decode_paged_fwd` needs (`nk_attention_decode_paged_workspace`): the contiguous forms' at the
/// virtual capacity `max_pages * page`, or at the window.
pub(crate) fn decode_paged_workspace(batch: usize, rows: usize, heads: usize, dh: usize, max_pages: usize, page: usize, window: usize) -> usize {
    unsafe {
        ffi::nk_attention_decode_paged_workspace(batch as i32, rows as i32, heads as i32, dh as i32, max_pages as i32, page as i32,
                                                 window.min(i32::MAX as usize) as i32)
    }
}

/// `PackedDecodeAttention` over a PAGED cache (semantics at `nk_attention_decode_paged_fwd` in `include/neuronika_hip.h`): `keys` /
/// `values` are the pools `(num_pages, heads, page, dh)`; `image` holds, in one upload of int32 in f32 cells, the `batch` start
/// positions, the `(batch, max_pages)` table rows and the `copies` (src | dst) page ids.  The forward runs the page copies
/// (`nk_kv_pages_copy`), then the append (`nk_kv_pages_append`), then the attention; running it again repeats the same writes.
pub(crate) struct PagedDecodeAttention {
    geometry: Heads, // `seq` = new rows per sequence, `heads` = kv heads
    query_heads: i32,
    page: i32,
    max_pages: i32,
    num_pages: i32,
    copies: i32,
    window: i32, // 0: off
    packed: Shared<HipArray<Ix2>>,
    keys: Shared<HipArray<Ix4>>,
    values: Shared<HipArray<Ix4>>,
    image: HipArray<Ix1>,
    workspace: Shared<HipArray<Ix1>>,
    data: Shared<HipArray<Ix2>>,
    scale: f32,
}

impl PagedDecodeAttention {
    #[allow(clippy::too_many_arguments)]
    pub(crate) fn new(geometry: Heads, query_heads: i32, page: i32, max_pages: i32, num_pages: i32, copies: i32, window: i32,
                      packed: Shared<HipArray<Ix2>>, keys: Shared<HipArray<Ix4>>, values: Shared<HipArray<Ix4>>, image: HipArray<Ix1>,
                      workspace: Shared<HipArray<Ix1>>, data: Shared<HipArray<Ix2>>, scale: f32) -> Self {
        Self { geometry, query_heads, page, max_pages, num_pages, copies, window, packed, keys, values, image, workspace, data, scale }
    }
}

impl Forward for PagedDecodeAttention {
    fn forward(&self) {
        let qkv = self.packed.borrow();
        let (mut kp, mut vp) = (self.keys.borrow_mut(), self.values.borrow_mut());
        let mut ws = self.workspace.borrow_mut();
        let mut out = self.data.borrow_mut();
        let h = self.geometry;
        let (d, dkv) = ((self.query_heads * h.dh) as usize, (h.heads * h.dh) as usize);
        let ld = (d + 2 * dkv) as i32;
        let start = self.image.as_ptr() as *const i32;
        let table = unsafe { start.add(h.batch as usize) };
        let pairs = unsafe { table.add((h.batch * self.max_pages) as usize) };
        let dev = qkv.device().as_raw();
        if self.copies > 0 {
            ffi::check(unsafe {
                ffi::nk_kv_pages_copy(dev, kp.as_mut_ptr(), vp.as_mut_ptr(), pairs, pairs.add(self.copies as usize), self.copies, h.heads, h.dh,
                                      self.page, self.num_pages)
            });
        }
        ffi::check(unsafe {
            ffi::nk_kv_pages_append(dev, kp.as_mut_ptr(), vp.as_mut_ptr(), qkv.as_ptr().add(d), qkv.as_ptr().add(d + dkv), ld, start, table,
                                    self.max_pages, h.batch, h.seq, h.heads, h.dh, self.page, self.num_pages)
        });
        ffi::check(unsafe {
            ffi::nk_attention_decode_paged_fwd(dev, qkv.as_ptr(), ld, kp.as_ptr(), vp.as_ptr(), start, table, self.max_pages, out.as_mut_ptr(),
                                               ws.as_mut_ptr(), h.batch, h.seq, self.query_heads, h.heads, h.dh, self.page, self.num_pages,
                                               self.window, self.scale)
        });
    }
}
