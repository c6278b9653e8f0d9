"""NumPy restatement of the embedding entry points (include/neuronika_hip.h, "embedding table"), in the device's summation order,
so that device and oracle are compared bit for bit.

ids are f32 and read with Rust's saturating `as usize` (NaN and negatives are 0, the fraction is dropped), as nk_nll_* reads its
targets.  Forward is indexing; an id >= V yields a zero row.  Backward: per table row the gradient rows of the tokens that selected it,
in ascending token order, summed sequentially in f32 STARTING FROM THE FIRST CONTRIBUTION ITSELF; a row more than CHUNK tokens
selected is summed chunk by chunk (CHUNK consecutive contributions each, the same rule inside a chunk) and the chunks' sums are added
in chunk order, again starting from the first.  The `+=` form then adds that sum to the table once; the assign form writes it, zeros
where no token selected the row."""
import numpy as np

CHUNK = 128  # a constant of the library (EMB_CHUNK), part of the summation order


def read_ids(idx):
    """the ids as int64 (2^63 - 1 where f32 saturates)"""
    f = np.asarray(idx, dtype=np.float32).reshape(-1)
    out = np.zeros(f.shape, np.int64)
    pos = f > 0                                   # False for NaN, negatives and zero
    big = pos & (f >= np.float32(9.2233720368547758e18))
    small = pos & ~big
    out[small] = np.trunc(f[small].astype(np.float64)).astype(np.int64)
    out[big] = np.iinfo(np.int64).max
    return out


def forward(weight, idx):
    weight = np.asarray(weight, dtype=np.float32)
    V, D = weight.shape
    ids = read_ids(idx)
    hit = ids < V
    out = np.zeros((ids.size, D), np.float32)
    out[hit] = weight[ids[hit]]
    return out.reshape(tuple(np.shape(idx)) + (D,))


def _ordered_sums(rows, seg, nseg):
    """rows (m, D) sorted by segment id `seg` (ascending, each segment's rows in the order they are to be added) ->
    (nseg, D): per segment the sequential f32 sum starting from its first row, zeros for an empty segment"""
    D = rows.shape[1]
    out = np.zeros((nseg, D), np.float32)
    if rows.shape[0] == 0:
        return out
    first = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]])
    length = np.diff(np.r_[first, seg.size])
    sid = seg[first]
    out[sid] = rows[first]                        # the first contribution as it is (-0.0 stays -0.0)
    for k in range(1, int(length.max())):
        live = length > k
        out[sid[live]] = out[sid[live]] + rows[first[live] + k]
    return out


def row_sums(g, idx, V, padding_idx=-1, chunk=CHUNK):
    """(sum (V, D) in the device's order, touched (V,) bool)"""
    g = np.asarray(g, dtype=np.float32)
    D = g.shape[-1]
    g = g.reshape(-1, D)
    ids = read_ids(idx)
    keep = ids < V
    if padding_idx is not None and padding_idx >= 0:
        keep &= ids != padding_idx
    t = np.flatnonzero(keep)
    order = t[np.argsort(ids[t], kind="stable")]  # by row, ascending token position inside a row
    rid = ids[order]
    touched = np.zeros(V, bool)
    touched[rid] = True
    if order.size == 0:
        return np.zeros((V, D), np.float32), touched
    first = np.flatnonzero(np.r_[True, rid[1:] != rid[:-1]])
    length = np.diff(np.r_[first, rid.size])
    within = np.arange(rid.size) - np.repeat(first, length)
    # segment = (row, chunk): one chunk for rows of at most `chunk` tokens
    cseg_of_row = np.r_[0, np.cumsum((length + chunk - 1) // chunk)]
    seg = np.repeat(cseg_of_row[:-1], length) + within // chunk
    partial = _ordered_sums(g[order], seg, int(cseg_of_row[-1]))
    # the chunks' sums in chunk order, per row
    prow = np.repeat(np.arange(first.size), np.diff(cseg_of_row))
    sums = _ordered_sums(partial, prow, first.size)
    out = np.zeros((V, D), np.float32)
    out[rid[first]] = sums
    return out, touched


def backward(dweight, g, idx, padding_idx=-1, chunk=CHUNK):
    """the `+=` form: a new table; rows no token selected are returned as they were"""
    dweight = np.asarray(dweight, dtype=np.float32)
    s, touched = row_sums(g, idx, dweight.shape[0], padding_idx, chunk)
    out = dweight.copy()
    out[touched] = dweight[touched] + s[touched]
    return out


def backward_assign(g, idx, V, padding_idx=-1, chunk=CHUNK):
    return row_sums(g, idx, V, padding_idx, chunk)[0]
