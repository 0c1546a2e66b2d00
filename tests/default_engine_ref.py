"""Reference definitions for the default convolution engine and MaxPool (a plain helper module: no fixture, no
pytest setting).

  im2col / col2im       numpy, from the definition: col[(c, ki, kj)][(oh, ow)] = x[c][oh*sh - pt + ki*dh][ow*sw - pl + kj*dw]
                        or 0 outside the image; col2im is its adjoint (every column entry added to the pixel it read).
  conv2d_f64 (+ grads)  float64 torch: F.pad([l, r, t, b]) then conv2d(padding=0, dilation=, groups=) under autograd.
  max_pool(_grad)       pool_op.cu MaxPoolForwardNCHW / MaxPoolBackwardNCHW: the window is clipped to the image, the
                        maximum is taken with `>` (a NaN never wins), and every input EQUAL to its window's maximum
                        receives that window's gradient (ties all receive it; torch gives it to one of them).

A geometry is a dict: kernel (kh, kw), stride (sh, sw), pads (t, l, b, r), dilation (dh, dw), group.
"""
import numpy as np
import torch


def geometry(kernel, stride=1, pads=0, dilation=1, group=1):
    two = lambda v: (int(v), int(v)) if np.isscalar(v) else tuple(int(a) for a in v)
    pads = (int(pads),) * 4 if np.isscalar(pads) else tuple(int(a) for a in pads)
    assert len(pads) == 4
    return dict(kernel=two(kernel), stride=two(stride), pads=pads, dilation=two(dilation), group=int(group))


def out_size(n, k, d, pa, pb, s):
    eff = d * (k - 1) + 1
    return (n + pa + pb - eff) // s + 1 if n + pa + pb >= eff else -1


def out_hw(H, W, g):
    (kh, kw), (sh, sw), (pt, pl, pb, pr), (dh, dw) = g["kernel"], g["stride"], g["pads"], g["dilation"]
    return out_size(H, kh, dh, pt, pb, sh), out_size(W, kw, dw, pl, pr, sw)


def im2col(x, g):
    """x [C][H][W] -> col [C * kh * kw][OH * OW], rows in (c, ki, kj) order, zero padding."""
    C, H, W = x.shape
    (kh, kw), (sh, sw), (pt, pl, _, _), (dh, dw) = g["kernel"], g["stride"], g["pads"], g["dilation"]
    OH, OW = out_hw(H, W, g)
    col = np.zeros((C, kh, kw, OH, OW), x.dtype)
    for ki in range(kh):
        for kj in range(kw):
            for oh in range(OH):
                h = oh * sh - pt + ki * dh
                if h < 0 or h >= H:
                    continue
                for ow in range(OW):
                    w = ow * sw - pl + kj * dw
                    if 0 <= w < W:
                        col[:, ki, kj, oh, ow] = x[:, h, w]
    return col.reshape(C * kh * kw, OH * OW)


def col2im(col, C, H, W, g):
    """The adjoint of im2col: col [C * kh * kw][OH * OW] -> x [C][H][W], summed in col's dtype in (ki, kj) order."""
    (kh, kw), (sh, sw), (pt, pl, _, _), (dh, dw) = g["kernel"], g["stride"], g["pads"], g["dilation"]
    OH, OW = out_hw(H, W, g)
    col = np.asarray(col).reshape(C, kh, kw, OH, OW)
    x = np.zeros((C, H, W), col.dtype)
    for ki in range(kh):
        for kj in range(kw):
            for oh in range(OH):
                h = oh * sh - pt + ki * dh
                if h < 0 or h >= H:
                    continue
                for ow in range(OW):
                    w = ow * sw - pl + kj * dw
                    if 0 <= w < W:
                        x[:, h, w] += col[:, ki, kj, oh, ow]
    return x


def _pad(x, g):
    pt, pl, pb, pr = g["pads"]
    return torch.nn.functional.pad(x, [pl, pr, pt, pb])


def conv2d_f64(X, Wt, b, g):
    """Y as float64 numpy; X [N][C][H][W], Wt [M][C / G][kh][kw], b [M] or None."""
    with torch.no_grad():
        y = torch.nn.functional.conv2d(_pad(torch.from_numpy(np.asarray(X, np.float64)), g),
                                       torch.from_numpy(np.asarray(Wt, np.float64)),
                                       None if b is None else torch.from_numpy(np.asarray(b, np.float64)),
                                       stride=g["stride"], padding=0, dilation=g["dilation"], groups=g["group"])
    return y.numpy()


def conv2d_grads_f64(X, Wt, dY, g):
    """(dW, db, dX) as float64 numpy."""
    x = torch.from_numpy(np.asarray(X, np.float64)).requires_grad_(True)
    w = torch.from_numpy(np.asarray(Wt, np.float64)).requires_grad_(True)
    b = torch.zeros(Wt.shape[0], dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(_pad(x, g), w, b, stride=g["stride"], padding=0, dilation=g["dilation"],
                                   groups=g["group"])
    y.backward(torch.from_numpy(np.asarray(dY, np.float64)))
    return w.grad.numpy(), b.grad.numpy(), x.grad.numpy()


def _windows(H, W, g):
    (kh, kw), (sh, sw), (pt, pl, _, _) = g["kernel"], g["stride"], g["pads"]
    OH, OW = out_hw(H, W, g)
    for oh in range(OH):
        h0, h1 = max(oh * sh - pt, 0), min(oh * sh - pt + kh, H)
        for ow in range(OW):
            w0, w1 = max(ow * sw - pl, 0), min(ow * sw - pl + kw, W)
            yield oh, ow, h0, h1, w0, w1


def max_pool(X, g):
    """Y [N][C][OH][OW] in X's dtype.  max by `>` from -inf: a NaN never becomes the maximum."""
    N, C, H, W = X.shape
    OH, OW = out_hw(H, W, g)
    Y = np.full((N, C, OH, OW), -np.inf, X.dtype)
    for oh, ow, h0, h1, w0, w1 in _windows(H, W, g):
        for h in range(h0, h1):
            for w in range(w0, w1):
                v = X[:, :, h, w]
                Y[:, :, oh, ow] = np.where(v > Y[:, :, oh, ow], v, Y[:, :, oh, ow])
    return Y


def max_pool_grad(X, Y, dY, g):
    """dX [N][C][H][W]: every input equal to its window's maximum receives that window's gradient; windows are added
    in (oh, ow) order in dY's dtype."""
    N, C, H, W = X.shape
    dX = np.zeros(X.shape, dY.dtype)
    for oh, ow, h0, h1, w0, w1 in _windows(H, W, g):
        hit = X[:, :, h0:h1, w0:w1] == Y[:, :, oh:oh + 1, ow:ow + 1]
        dX[:, :, h0:h1, w0:w1] += np.where(hit, dY[:, :, oh:oh + 1, ow:ow + 1], 0).astype(dY.dtype)
    return dX


def _case(name, route, cin, cout, hw, kernel, stride=1, pads=0, dilation=1, group=1, N=2):
    return dict(name=name, route=route, cin=cin, cout=cout, hw=hw, N=N,
                geo=geometry(kernel, stride, pads, dilation, group))


# The Conv geometries of the default-engine sweep.  `route` is the route of ops/conv_op.cc the case takes, forward /
# gradient, as read from RunDefaultEngine: "pw-gemm" the pointwise GEMM kernels (with ssad_subsample when strided),
# "igemm" the implicit GEMM, "kxk" the batched k x k gradient launchers, "loop" the per-image GEMM loop without im2col
# (the image is its own column matrix), "im2col" the per-image im2col (+ col2im) + general GEMM loop.
# M = 70 crosses the 64-row tile of gemm_general_kernel, no P is a multiple of 64, and no K of a case that reaches the
# general GEMM is a multiple of 16.
CONV_CASES = [
    _case("dil2_k3p2", "im2col/im2col", 5, 70, (9, 11), 3, 1, 2, 2),
    _case("dil_h2w1", "im2col/im2col", 5, 70, (9, 11), 3, 1, (2, 1, 2, 1), (2, 1)),
    _case("dil2_s2", "im2col/im2col", 5, 70, (9, 11), 3, 2, 2, 2),
    _case("rect_k3x2", "im2col/im2col", 5, 70, (9, 11), (3, 2), 1, (1, 0, 1, 1)),
    _case("asym_pads_k3s2", "im2col/im2col", 5, 70, (9, 11), 3, 2, (0, 2, 1, 0)),
    _case("stride_h2w1_k3", "im2col/im2col", 5, 70, (9, 11), 3, (2, 1), 1),
    _case("stride_h2w1_k1", "im2col/im2col", 6, 70, (9, 11), 1, (2, 1), 0),
    _case("k1_pad1", "igemm/kxk", 8, 70, (9, 11), 1, 1, 1),
    _case("pw_P96", "pw-gemm/pw-gemm", 8, 70, (8, 12), 1),                       # P % 16 == 0
    _case("pw_P108", "pw-gemm/loop", 8, 70, (9, 12), 1),                        # P % 4 == 0, P % 16 != 0
    _case("pw_P99", "loop/loop", 8, 70, (9, 11), 1),                            # P % 4 != 0
    _case("pw_C6_P108", "loop/loop", 6, 70, (9, 12), 1),                        # C % 4 != 0, P % 4 == 0
    _case("pw_s2_even_P32", "pw-gemm/pw-gemm", 8, 70, (8, 16), 1, 2),           # subsampled, P % 16 == 0
    _case("pw_s2_even_P24", "pw-gemm/kxk", 8, 70, (8, 12), 1, 2),               # subsampled, P % 16 != 0
    _case("pw_s2_odd_9x11", "igemm/kxk", 8, 70, (9, 11), 1, 2),                 # P = 30: kernel 1 on the implicit GEMM
    _case("k2s2", "igemm/kxk", 5, 70, (9, 11), 2, 2, 0),
    _case("k4s3p2", "igemm/kxk", 5, 70, (9, 11), 4, 3, 2),
    _case("K27_k3s2", "igemm/im2col", 3, 20, (9, 11), 3, 2, 1),                  # K % 4 != 0: dx_ok false
    _case("g3_dil2", "im2col/im2col", 6, 12, (9, 11), 3, 1, 2, 2, 3),
    _case("g2_rect", "im2col/im2col", 6, 70, (9, 11), (3, 2), 1, (1, 0, 1, 1), 1, 2),
    _case("g2_Mg5_Cg2", "im2col/im2col", 4, 10, (9, 11), 3, 1, 1, 1, 2),         # M / G != C / G
    _case("g3_Mg1", "im2col/im2col", 6, 3, (9, 11), 3, 2, 1, 1, 3),              # M / G == 1
    _case("N1_dil2", "im2col/im2col", 5, 70, (9, 11), 3, 1, 2, 2, N=1),
]
CONV_CASE = {c["name"]: c for c in CONV_CASES}

# MaxPool geometries; `sym` marks those torch's max_pool2d can express (symmetric pads, pad <= kernel / 2)
POOL_CASES = [
    dict(name="k2s2p0", hw=(8, 10), geo=geometry(2, 2, 0), sym=True),
    dict(name="k3s2p1_odd", hw=(9, 11), geo=geometry(3, 2, 1), sym=True),
    dict(name="k3s1p1", hw=(7, 9), geo=geometry(3, 1, 1), sym=True),
    dict(name="k2x3_s1x2_asym", hw=(8, 11), geo=geometry((2, 3), (1, 2), (0, 1, 1, 0)), sym=False),
    dict(name="k2s3_gaps", hw=(9, 11), geo=geometry(2, 3, 0), sym=True),
]


def conv_inputs(case, seed=0):
    """X, W, b, dY as float32 for a case (deterministic per case name and seed)."""
    g = case["geo"]
    rng = np.random.default_rng([seed] + [ord(ch) for ch in case["name"]])
    N, C, M = case["N"], case["cin"], case["cout"]
    H, W = case["hw"]
    kh, kw = g["kernel"]
    OH, OW = out_hw(H, W, g)
    X = rng.standard_normal((N, C, H, W)).astype(np.float32)
    Wt = (rng.standard_normal((M, C // g["group"], kh, kw)) * 0.2).astype(np.float32)
    b = rng.standard_normal(M).astype(np.float32)
    dY = rng.standard_normal((N, M, OH, OW)).astype(np.float32)
    return X, Wt, b, dY
