"""NumPy f64 statement of the cross-entropy contract of include/neuronika_hip.h (`nk_cross_entropy_*`), and the ONE place the
tests' tolerances come from.

    x       logits (N, C, d1..dk);  target (N, d1..dk) class ids stored as f32, read as the device reads them (`read_ids`)
    active  id < C and id != ignore_index (negative: none)
    loss_p  (1 - e) (lse - x_t) + e (lse - mean_c x_c)       lse = log sum_c exp(x_c)
    Sum     the sum of loss_p over the active positions;  Mean: divided by the number of active positions, 0 when there is none
            (torch gives NaN there)
    dx      g w (softmax - (1 - e) onehot(t) - e / C) on active positions, zero rows elsewhere;  w = 1 or 1 / active count
"""
import math

import numpy as np

U = 2.0 ** -24  # unit roundoff of f32


def read_ids(target):
    """Rust's saturating `f32 as usize`, as nk_nll_* / nk_embedding_* / nk_cross_entropy_* read ids: NaN and negatives are 0, the
    fraction is dropped, values beyond i64 saturate"""
    t = np.asarray(target, dtype=np.float32).astype(np.float64)
    t = np.where(t > 0, t, 0.0)          # NaN, negatives, -0.0
    t = np.minimum(np.trunc(t), 9.0e18)  # any C is far below
    return t.astype(np.int64)


def active_mask(target, C, ignore_index=-1):
    ids = read_ids(target)
    on = ids < C
    if ignore_index is not None and ignore_index >= 0:
        on &= ids != ignore_index
    return ids, on


def _rows(x):
    """(N, C, inner) f64 view of the logits"""
    x = np.asarray(x)
    assert x.ndim >= 2
    return x.astype(np.float64).reshape(x.shape[0], x.shape[1], -1)


def pieces(x, target, ignore_index=-1, label_smoothing=0.0):
    """-> lse (N, inner), per-position loss (N, inner; 0 where inactive), ids, active mask, all f64 / exact"""
    X = _rows(x)
    N, C, inner = X.shape
    ids, on = active_mask(np.asarray(target).reshape(N, inner), C, ignore_index)
    with np.errstate(all="ignore"):
        m = np.maximum(X.max(axis=1), np.finfo(np.float32).min) if C else np.full((N, inner), np.finfo(np.float32).min)
        lse = m + np.log(np.exp(X - m[:, None, :]).sum(axis=1))
        safe = np.where(on, ids, 0)
        xt = np.take_along_axis(X, safe[:, None, :], axis=1)[:, 0, :] if C else np.zeros((N, inner))
        loss = lse - xt
        if label_smoothing:
            loss = (1.0 - label_smoothing) * loss + label_smoothing * (lse - X.mean(axis=1))
    return lse, np.where(on, loss, 0.0), ids, on


def forward(x, target, reduction="mean", ignore_index=-1, label_smoothing=0.0):
    """-> (loss, lse of the target's shape)"""
    lse, loss, _, on = pieces(x, target, ignore_index, label_smoothing)
    total, count = loss[on].sum(), int(on.sum())
    if reduction == "mean":
        total = total / count if count else 0.0
    return float(total), lse.reshape(np.asarray(target).shape)


def backward(x, target, lse=None, g=1.0, reduction="mean", ignore_index=-1, label_smoothing=0.0):
    """-> dx of x's shape (f64).  `lse`: the forward's (recomputed when None)"""
    X = _rows(x)
    N, C, inner = X.shape
    if lse is None:
        lse = pieces(x, target, ignore_index, label_smoothing)[0]
    lse = np.asarray(lse, dtype=np.float64).reshape(N, inner)
    ids, on = active_mask(np.asarray(target).reshape(N, inner), C, ignore_index)
    count = int(on.sum())
    w = (1.0 / count if count else 0.0) if reduction == "mean" else 1.0
    with np.errstate(all="ignore"):
        d = np.exp(X - lse[:, None, :]) - (label_smoothing / C if C else 0.0)
    n, r = np.nonzero(on)
    d[n, ids[n, r], r] -= 1.0 - label_smoothing
    d *= g * w
    d = np.where(on[:, None, :], d, 0.0)
    return d.reshape(np.asarray(x).shape)


def bounds(C, xmax, positions, label_smoothing=0.0, g=1.0, weight=1.0):
    """Absolute tolerances of an f32 evaluation against this oracle, from the class count, max |logit| and the position count.

    lse = m + log s.  s sums C terms exp(x - m) in (0, 1], each carrying the rounding of the subtraction (u |x - m|, a relative error
    of the term, weighted by a term <= 1 / e of it) and of expf (<= 2 ulp), through chains of additions whose length depends on the
    kernel (C / 64 .. C).  The worst case is linear in the chain; terms of one sign round independently, so the error grows as its
    square root: 4 sqrt(C) u covers every kernel with a factor to spare.  log turns that relative error into an absolute one; m + .
    rounds once more at the size of lse <= xmax + log C.
        lse   u (4 sqrt(C) + 16) + 2 u (xmax + log C)
    A position's loss subtracts x_t (one rounding at <= 2 xmax + log C) and, with smoothing e, e times the mean of the logits, a
    sum of C terms of size xmax divided by C:
        pos   lse + 2 u (2 xmax + log C) + e u (4 sqrt(C) + 16) xmax
    The Sum adds P such positions (errors add at worst) through partial sums whose own rounding is u (8 + sqrt(P)) of the sum of
    the magnitudes, each <= 2 xmax + log C; Mean divides both by the count, so `loss` is PER ACTIVE POSITION under Mean and the
    caller multiplies by the count under Sum:
        loss  pos + u (8 + sqrt(P)) (2 xmax + log C)
    dx = g w (exp(x - lse) - ...): the exponent carries lse's error and its own subtraction (u (2 xmax + log C)), the exponential
    is <= 1 when lse is right, and the two subtractions and the product round at O(1):
        dx    |g w| (lse + u (2 xmax + log C) + 8 u)
    """
    logc = math.log(max(C, 2))
    chain = U * (4.0 * math.sqrt(max(C, 1)) + 16.0)
    lse = chain + 2.0 * U * (xmax + logc)
    pos = lse + 2.0 * U * (2.0 * xmax + logc) + label_smoothing * chain * xmax
    loss = pos + U * (8.0 + math.sqrt(max(positions, 1))) * (2.0 * xmax + logc)
    dx = abs(g * weight) * (lse + U * (2.0 * xmax + logc) + 8.0 * U)
    return {"lse": lse, "loss": loss, "dx": dx}
