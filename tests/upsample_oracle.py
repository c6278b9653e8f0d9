"""NumPy oracle of nk_upsample_* (include/neuronika_hip.h, "upsampling"): the device's arithmetic restated operation for operation in
f32 - every product, sum and difference rounded on its own, the same order - so the device is compared with it BIT FOR BIT; and the
same maps in f64 through torch on the CPU, which pins this file.  The backward is the header's definition read literally: a scatter
in ascending row-major order of the outputs, corners in row-major order, which gives every input element its contributions in the
order the device's gather walks them.  It loops in Python over one plane's outputs and is vectorised over the planes."""
import itertools

import numpy as np

F = np.float32
MODES = ("nearest", "linear")

# (x_shape, out_size): the smallest shapes that reach each kernel class and each edge
SHAPES = [
    ((2, 3, 5), (8,)),
    ((2, 3, 4, 4), (8, 8)),            # nearest x2 class
    ((1, 2, 5, 7), (10, 14)),          # x2 but ragged: generic
    ((1, 2, 6, 8), (9, 20)),           # non-integer ratio, vector stores
    ((1, 1, 7, 8), (3, 4)),            # downsampling
    ((1, 1, 3, 12), (7, 40)),
    ((1, 1, 16, 16), (24, 40)),
    ((1, 2, 1, 4), (3, 8)),            # in = 1
    ((1, 2, 4, 4), (1, 1)),            # out = 1
    ((1, 2, 3, 4, 4), (6, 8, 8)),
    ((1, 1, 2, 3, 5), (5, 4, 7)),
]


def variants():
    """(mode, align_corners) of every form"""
    return [("nearest", False), ("linear", False), ("linear", True)]


def torch_mode(mode, nd):
    return "nearest" if mode == "nearest" else ("linear", "bilinear", "trilinear")[nd - 1]


def out_size(x_shape, scale):
    """nk_upsample_out_size: floor(in * scale) in f64"""
    nd = len(x_shape) - 2
    sc = [scale] * nd if not hasattr(scale, "__len__") else list(scale)
    return tuple(int(np.floor(np.float64(x_shape[2 + i]) * np.float64(sc[i]))) for i in range(nd))


def nearest_index(n_in, n_out):
    return np.minimum((np.arange(n_out, dtype=np.int64) * n_in) // n_out, n_in - 1)


def linear_axis(n_in, n_out, align_corners):
    """(i0, i1, l0, l1) of every output index of one axis: upsample_axis of the device, in f32"""
    o = np.arange(n_out, dtype=np.int64).astype(F)
    if align_corners:
        s = F(0) if n_out == 1 else F(n_in - 1) / F(n_out - 1)
        src = s * o
    else:
        s = F(n_in) / F(n_out)
        src = np.maximum(s * (o + F(0.5)) - F(0.5), F(0))
    assert src.dtype == F
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = src - i0.astype(F)
    l0 = F(1) - l1
    return i0, i1, l0, l1


def forward(x, size, mode, align_corners=False):
    x = np.asarray(x, F)
    nd = x.ndim - 2
    assert len(size) == nd and mode in MODES
    y = x
    for a in range(nd - 1, -1, -1):                      # innermost axis first, then outward
        ax = 2 + a
        if mode == "nearest":
            y = np.take(y, nearest_index(x.shape[ax], size[a]), axis=ax)
        else:
            i0, i1, l0, l1 = linear_axis(x.shape[ax], size[a], align_corners)
            bc = [1] * y.ndim
            bc[ax] = size[a]
            with np.errstate(invalid="ignore"):
                y = l0.reshape(bc) * np.take(y, i0, axis=ax) + l1.reshape(bc) * np.take(y, i1, axis=ax)
        assert y.dtype == F
    return np.ascontiguousarray(y)


def backward(g, x_shape, mode, align_corners=False):
    """total(i) of the header for every input element, from an all-zero start"""
    g = np.asarray(g, F)
    nd = len(x_shape) - 2
    ins, outs = tuple(x_shape[2:]), tuple(g.shape[2:])
    planes = x_shape[0] * x_shape[1]
    gp = g.reshape((planes,) + outs)
    dx = np.zeros((planes,) + ins, F)
    if mode == "nearest":
        idx = [nearest_index(ins[a], outs[a]) for a in range(nd)]
        for o in itertools.product(*(range(n) for n in outs)):
            i = tuple(int(idx[a][o[a]]) for a in range(nd))
            dx[(slice(None),) + i] = dx[(slice(None),) + i] + gp[(slice(None),) + o]
    else:
        axes = [linear_axis(ins[a], outs[a], align_corners) for a in range(nd)]
        for o in itertools.product(*(range(n) for n in outs)):
            go = gp[(slice(None),) + o]
            for corner in itertools.product((0, 1), repeat=nd):      # row-major corner order
                i = tuple(int(axes[a][corner[a]][o[a]]) for a in range(nd))
                w = axes[nd - 1][2 + corner[nd - 1]][o[nd - 1]]      # innermost first: w = l_w; w = l_h * w; w = l_d * w
                for a in range(nd - 2, -1, -1):
                    w = axes[a][2 + corner[a]][o[a]] * w
                assert w.dtype == F
                with np.errstate(invalid="ignore"):
                    dx[(slice(None),) + i] = dx[(slice(None),) + i] + w * go
    return dx.reshape(x_shape)


def readers(x_shape, size, mode, align_corners=False):
    """the largest number of (output, corner) contributions one input element receives"""
    nd = len(x_shape) - 2
    count = np.zeros(tuple(x_shape[2:]), np.int64)
    if mode == "nearest":
        idx = [nearest_index(x_shape[2 + a], size[a]) for a in range(nd)]
        for o in itertools.product(*(range(n) for n in size)):
            count[tuple(int(idx[a][o[a]]) for a in range(nd))] += 1
    else:
        axes = [linear_axis(x_shape[2 + a], size[a], align_corners) for a in range(nd)]
        for o in itertools.product(*(range(n) for n in size)):
            for corner in itertools.product((0, 1), repeat=nd):
                count[tuple(int(axes[a][corner[a]][o[a]]) for a in range(nd))] += 1
    return int(count.max())


def torch64(x, size, mode, align_corners=False, g=None):
    """(y, dx) in f64 through torch on the CPU; dx is None without g"""
    import torch
    import torch.nn.functional as TF
    X = torch.tensor(np.asarray(x, np.float64), requires_grad=g is not None)
    nd = X.dim() - 2
    kw = {} if mode == "nearest" else {"align_corners": bool(align_corners)}
    Y = TF.interpolate(X, size=tuple(size), mode=torch_mode(mode, nd), **kw)
    if g is None:
        return Y.detach().numpy(), None
    Y.backward(torch.tensor(np.asarray(g, np.float64)))
    return Y.detach().numpy(), X.grad.numpy()
