"""Kernel isolation, Part A (tests/test_gpu_isolation.py's docstring), for the launchers of the default engine and the
entry points the three earlier isolation files had not reached: ssad_gemm_f32, ssad_im2col / _batched, ssad_col2im,
ssad_channel_sum, ssad_max_pool_forward / _backward, ssad_weighted_sum, the single-input ssad_conv1x1_bias_act, the
_prezeroed loss forms, ssad_softmax_focal_loss_fused and the batched packers ssad_transpose_filters /
ssad_conv_wino_pack_filters.  Every operand, output and workspace is a view of one sentinel arena; guards intact,
inputs frozen, outputs fully written, bits equal to the same call on ordinary allocations, the family's bar against the
float64 definition.  The launchers are bound through ctypes on K.lib() here where kernels.py's wrapper allocates its
own output (or has no wrapper)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle  # noqa: E402
from ssad_amd import synth  # noqa: E402
from guarded import Arena  # noqa: E402
import default_engine_ref as R  # noqa: E402
from test_gpu_kernels import CONV_FLOOR, CONV_RTOL, DX_FLOOR, DX_RTOL, LOSS_RTOL, close  # noqa: E402
from test_gpu_isolation import LOSS_MAPS, Guarded, Plain, bits, randn  # noqa: E402

pytestmark = pytest.mark.gpu

BADARG = -1


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ssad_amd import kernels
    kernels.lib()  # raises if the HIP extension is missing: no fallback
    return kernels


@pytest.fixture(scope="module")
def L(K):
    lib = K.lib()
    vp, i32, f32, ll = C.c_void_p, C.c_int, C.c_float, C.c_longlong
    lib.ssad_gemm_f32.argtypes = [i32, i32, i32, i32, i32, f32, vp, i32, ll, vp, i32, ll, f32, vp, i32, ll, i32, vp]
    lib.ssad_im2col.argtypes = [vp] + [i32] * 13 + [vp, vp]
    lib.ssad_col2im.argtypes = [vp] + [i32] * 13 + [vp, vp]
    lib.ssad_im2col_batched.argtypes = [vp] + [i32] * 7 + [vp, vp]
    lib.ssad_channel_sum.argtypes = [vp, i32, i32, i32, vp, i32, vp]
    lib.ssad_max_pool_forward.argtypes = [vp] + [i32] * 12 + [vp, vp]
    lib.ssad_max_pool_backward.argtypes = [vp, vp, vp] + [i32] * 12 + [vp, vp]
    lib.ssad_weighted_sum.argtypes = [C.POINTER(vp), C.POINTER(vp), i32, vp, C.c_int64, vp]
    return lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(rc):
    assert rc == 0, "launcher returned %d" % rc


def isolated(fn, modified=(), nan_ok=None):
    """fn(al) -> {name: tensor}, once on ordinary allocations and once inside an arena sized from the first run.
    Returns (the arena run's results as numpy, the arena) after the guard / frozen-operand / unwritten-output checks
    and the bit comparison of the two runs."""
    plain = Plain()
    want = {k: v.detach().cpu().numpy().copy() for k, v in fn(plain).items()}
    arena = Arena(Arena.bytes_for(*plain.sizes))
    g = Guarded(arena)
    res = fn(g)
    assert g.n_ws == plain.n_ws
    assert arena.check(modified=modified, nan_ok=nan_ok)
    got = {k: v.detach().cpu().numpy().copy() for k, v in res.items()}
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), "%s depends on where its operands are placed" % k
    return got, arena


# ---------------------------------------------------------------------------------------------------------------------
# ssad_gemm_f32
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=["nn", "nt", "tn", "tt"])
def test_guarded_general_gemm(L, ta, tb):
    """sizes of test_general_gemm_matches_float64 (75 x 131 x 147, batch 3), all three leading dimensions padded.
    beta = 0 over a C full of the sentinel NaN, then beta = 1 onto the result; the padding columns of C still hold
    the sentinel word for word."""
    M, N, Kk, batch = 75, 131, 147, 3
    lda, ldb, ldc = (M if ta else Kk) + 5, (Kk if tb else N) + 3, N + 2
    rng = np.random.default_rng(9000 + 2 * ta + tb)
    A, B = randn(rng, batch, Kk if ta else M, lda), randn(rng, batch, N if tb else Kk, ldb)
    pad = np.zeros((batch, M, ldc), bool)
    pad[:, :, N:] = True

    def fn(al):
        a, b = al.inp("A", A), al.inp("B", B)
        c0, c1 = al.out("C_beta0", (batch, M, ldc)), al.out("C_beta1", (batch, M, ldc))
        for c, launches in ((c0, 1), (c1, 2)):
            ok(L.ssad_gemm_f32(ta, tb, M, N, Kk, 1.5, a.data_ptr(), lda, a.stride(0), b.data_ptr(), ldb, b.stride(0), 0.0,
                               c.data_ptr(), ldc, c.stride(0), batch, stream()))
            if launches == 2:
                ok(L.ssad_gemm_f32(ta, tb, M, N, Kk, -0.5, a.data_ptr(), lda, a.stride(0), b.data_ptr(), ldb,
                                   b.stride(0), 1.0, c.data_ptr(), ldc, c.stride(0), batch, stream()))
        return dict(c0=c0[:, :, :N].contiguous(), c1=c1[:, :, :N].contiguous())

    got, arena = isolated(fn, nan_ok={"C_beta0": pad, "C_beta1": pad})
    for name in ("C_beta0", "C_beta1"):
        assert np.array_equal(arena.untouched(name), pad), name + ": the padding columns of C were written"
    opA = (A[:, :, :M].transpose(0, 2, 1) if ta else A[:, :, :Kk]).astype(np.float64)
    opB = (B[:, :, :Kk].transpose(0, 2, 1) if tb else B[:, :, :N]).astype(np.float64)
    want = 1.5 * np.matmul(opA, opB)
    assert np.isfinite(got["c0"]).all() and np.isfinite(got["c1"]).all()
    # the bars of test_general_gemm_matches_float64
    assert np.abs(got["c0"] - want).max() <= 1e-5 * np.abs(want).max()
    assert np.abs(got["c1"] - want / 1.5).max() <= 2e-5 * np.abs(want).max()


# ---------------------------------------------------------------------------------------------------------------------
# ssad_im2col / ssad_im2col_batched / ssad_col2im / ssad_channel_sum
# ---------------------------------------------------------------------------------------------------------------------

def geo_ints(Cc, H, W, g):
    (kh, kw), (sh, sw), (pt, pl, pb, pr), (dh, dw) = g["kernel"], g["stride"], g["pads"], g["dilation"]
    return [Cc, H, W, kh, kw, dh, dw, pt, pl, pb, pr, sh, sw]


@pytest.mark.parametrize("name", ["dil2_k3p2", "asym_pads_k3s2", "rect_k3x2", "stride_h2w1_k3"])
def test_guarded_im2col_and_col2im(L, name):
    case = R.CONV_CASE[name]
    g, Cc, (H, W) = case["geo"], case["cin"], case["hw"]
    rng = np.random.default_rng(9100)
    x = randn(rng, Cc, H, W)
    want = R.im2col(x, g)
    c = randn(rng, *want.shape)

    def fn(al):
        tx, tc = al.inp("x", x), al.inp("col_in", c)
        col, back = al.out("col", want.shape), al.out("x_back", x.shape)
        ok(L.ssad_im2col(tx.data_ptr(), *geo_ints(Cc, H, W, g), col.data_ptr(), stream()))
        ok(L.ssad_col2im(tc.data_ptr(), *geo_ints(Cc, H, W, g), back.data_ptr(), stream()))
        return dict(col=col, back=back)

    got, _ = isolated(fn)
    assert np.array_equal(bits(got["col"]), bits(want))
    close(got["back"], R.col2im(c.astype(np.float64), Cc, H, W, g), DX_RTOL, DX_FLOOR, "col2im")


@pytest.mark.parametrize("shape,skew", [((2, 5, 9, 16), 0), ((2, 5, 9, 11), 0), ((2, 5, 9, 16), 4)],
                         ids=["rows_kernel", "fallback_OW6", "fallback_col_4_bytes_off"])
def test_guarded_im2col_batched(L, shape, skew):
    N, Cc, H, W = shape
    g = R.geometry(3, 2, 1)
    rng = np.random.default_rng(9200)
    X = randn(rng, *shape)
    want = np.stack([R.im2col(x, g) for x in X])

    def fn(al):
        tx, col = al.inp("x", X), al.out("col", want.shape, skew=skew)
        ok(L.ssad_im2col_batched(tx.data_ptr(), N, Cc, H, W, 3, 2, 1, col.data_ptr(), stream()))
        return dict(col=col)

    got, _ = isolated(fn)
    assert np.array_equal(bits(got["col"]), bits(want))


@pytest.mark.parametrize("hw", [1, 99, 1030])
def test_guarded_channel_sum(L, hw):
    """the bias gradient's channel sums (double partials): overwrite, then accumulate onto the result"""
    N, Cc = 3, 5
    rng = np.random.default_rng(9300 + hw)
    dy = randn(rng, N, Cc, hw)

    def fn(al):
        t, out, acc = al.inp("dy", dy), al.out("sum", Cc), al.out("sum_twice", Cc)
        ok(L.ssad_channel_sum(t.data_ptr(), N, Cc, hw, out.data_ptr(), 0, stream()))
        ok(L.ssad_channel_sum(t.data_ptr(), N, Cc, hw, acc.data_ptr(), 0, stream()))
        ok(L.ssad_channel_sum(t.data_ptr(), N, Cc, hw, acc.data_ptr(), 1, stream()))
        return dict(out=out, acc=acc)

    got, _ = isolated(fn)
    want = dy.astype(np.float64).sum((0, 2))
    close(got["out"], want, CONV_RTOL, CONV_FLOOR, "channel sums")
    close(got["acc"], 2 * want, CONV_RTOL, CONV_FLOOR, "channel sums, accumulated")


# ---------------------------------------------------------------------------------------------------------------------
# ssad_max_pool_forward / _backward
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.POOL_CASES, ids=lambda c: c["name"])
def test_guarded_max_pool(L, case):
    """N = 2, C = 3, data with ties (X from {0, 1, 2}, integer dY): bit equality with the definition"""
    g = case["geo"]
    (kh, kw), (sh, sw), (pt, pl, pb, pr) = g["kernel"], g["stride"], g["pads"]
    H, W = case["hw"]
    rng = np.random.default_rng(9400)
    X = rng.integers(0, 3, (2, 3, H, W)).astype(np.float32)
    Yd = R.max_pool(X, g)
    dY = rng.integers(-3, 4, Yd.shape).astype(np.float32)
    geo = [2, 3, H, W, kh, kw, sh, sw, pt, pl, pb, pr]

    def fn(al):
        x, dy = al.inp("x", X), al.inp("dy", dY)
        y, dx = al.out("y", Yd.shape), al.out("dx", X.shape)
        ok(L.ssad_max_pool_forward(x.data_ptr(), *geo, y.data_ptr(), stream()))
        ok(L.ssad_max_pool_backward(x.data_ptr(), y.data_ptr(), dy.data_ptr(), *geo, dx.data_ptr(), stream()))
        return dict(y=y, dx=dx)

    got, _ = isolated(fn)
    assert np.array_equal(bits(got["y"]), bits(Yd))
    assert np.array_equal(got["dx"], R.max_pool_grad(X, Yd, dY, g))


# ---------------------------------------------------------------------------------------------------------------------
# ssad_weighted_sum
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("skew", [0, 4])
@pytest.mark.parametrize("pairs", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 5, 1023])
def test_guarded_weighted_sum(L, n, pairs, skew):
    """out = sum_k w_k[0] * x_k for 1, 2 and the maximum of 8 pairs, into its own output and in place (out is xs[0],
    as the update operators use it); skew 4: every view starts 4 bytes into its slot"""
    rng = np.random.default_rng(9500 + n + pairs)
    xs, ws = [randn(rng, n) for _ in range(pairs)], [randn(rng, 1) for _ in range(pairs)]
    vp = C.c_void_p

    def fn(al):
        tx = [al.inp("x%d" % k, a, skew=skew) for k, a in enumerate(xs)]
        tw = [al.inp("w%d" % k, a) for k, a in enumerate(ws)]
        first = al.inp("x0_in_place", xs[0], skew=skew)
        out = al.out("out", n, skew=skew)
        wp = (vp * pairs)(*[t.data_ptr() for t in tw])
        ok(L.ssad_weighted_sum((vp * pairs)(*[t.data_ptr() for t in tx]), wp, pairs, out.data_ptr(), n, stream()))
        ok(L.ssad_weighted_sum((vp * pairs)(*[t.data_ptr() for t in [first] + tx[1:]]), wp, pairs, first.data_ptr(), n,
                               stream()))
        return dict(out=out, in_place=first)

    got, _ = isolated(fn, modified=("x0_in_place",))
    want = sum(w.astype(np.float64)[0] * x.astype(np.float64) for w, x in zip(ws, xs))
    # `pairs` fp32 products summed in order: 1e-6 relative of the largest term's scale covers pairs * 2^-24
    scale = sum(abs(float(w[0])) * np.abs(x).astype(np.float64) for w, x in zip(ws, xs))
    assert np.all(np.abs(got["out"] - want) <= 1e-6 * scale)
    assert np.array_equal(bits(got["in_place"]), bits(got["out"]))
    assert L.ssad_weighted_sum(None, None, 9, None, n, None) == BADARG and L.ssad_weighted_sum(None, None, 0, None, n, None) == BADARG


# ---------------------------------------------------------------------------------------------------------------------
# ssad_conv1x1_bias_act (single input)
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cin", [32, 64], ids=["C32_chunked_kernel", "C64_persistent_kernel"])
def test_guarded_conv1x1_bias_act(K, Cin):
    """the smallest C, M and P the argument check of conv1x1_fused.hip admits (C % 32, M % 128, P % 4): C = 32 on the
    chunked kernel and C = 64 on the persistent one, M = 128, P = 4, two images; bias, residual and ReLU on and off"""
    Lb = K.lib()
    N, M, P = 2, 128, 4
    rng = np.random.default_rng(9600 + Cin)
    X, Wt, b, Rs = randn(rng, N, Cin, 2, 2), randn(rng, M, Cin, scale=Cin ** -0.5), randn(rng, M), randn(rng, N, M, 2, 2)
    forms = [("plain", False, False, 0), ("bias_relu", True, False, 1), ("bias_residual_relu", True, True, 1),
             ("residual", False, True, 0)]

    def fn(al):
        x, w, bias, res = al.inp("x", X), al.inp("w", Wt), al.inp("bias", b), al.inp("residual", Rs)
        out = {}
        for name, hb, hr, relu in forms:
            y = al.out("y_" + name, (N, M, 2, 2))
            ok(Lb.ssad_conv1x1_bias_act(x.data_ptr(), w.data_ptr(), bias.data_ptr() if hb else None,
                                        res.data_ptr() if hr else None, y.data_ptr(), N, Cin, P, M, relu, stream()))
            out[name] = y
        return out

    got, _ = isolated(fn)
    lin = np.einsum("mc,nchw->nmhw", Wt.astype(np.float64), X.astype(np.float64))
    for name, hb, hr, relu in forms:
        ref = lin + (b.reshape(1, M, 1, 1) if hb else 0) + (Rs if hr else 0)
        close(got[name], np.maximum(ref, 0) if relu else ref, CONV_RTOL, CONV_FLOOR, name)
    # what the check excludes: SSAD_E_BADARG before any launch
    x, w, y = torch.zeros(N * 64 * 8 + 4, device="cuda"), torch.zeros(256 * 64, device="cuda"), torch.zeros(N * 256 * 8, device="cuda")
    call = lambda Cc, Mm, Pp, xp=None: Lb.ssad_conv1x1_bias_act(xp or x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(),
                                                                 N, Cc, Pp, Mm, 0, stream())
    for Cc, Mm, Pp in ((16, 128, 4), (48, 128, 4), (32, 64, 4), (32, 192, 4), (32, 128, 2), (32, 128, 6), (0, 128, 4)):
        assert call(Cc, Mm, Pp) == BADARG, (Cc, Mm, Pp)
    assert call(32, 128, 4, x.data_ptr() + 4) == BADARG           # x not 16-byte aligned
    assert Lb.ssad_conv1x1_bias_act(None, w.data_ptr(), None, None, y.data_ptr(), N, 32, 4, 128, 0, stream()) == BADARG
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# the _prezeroed loss forms and ssad_softmax_focal_loss_fused: the loss family's three-level case
# ---------------------------------------------------------------------------------------------------------------------

def test_guarded_prezeroed_loss_forms(K):
    """ssad_cls_losses_fused_prezeroed and ssad_pow_sum_prezeroed: the caller zero-fills the workspace (exactly
    *_workspace_bytes long, inside the arena) once; two launches in a row on it -- every completed launch leaves the
    counters zero again -- give the bits of the self-zeroing forms."""
    Lb = K.lib()
    Cn = 3
    rng = np.random.default_rng(8000)
    lv = [synth.distill_inputs(rng, n, a, Cn, h, w) for n, a, h, w in LOSS_MAPS]
    dkw = dict(gamma=2.0, alpha=0.5, beta=0.3, num_classes=Cn, ignored_label=-1, scale=0.5)
    fkw = dict(gamma=2.0, alpha=0.25, num_classes=Cn, scale=0.5)
    DP = K.DistillParams(dkw["gamma"], dkw["alpha"], dkw["beta"], Cn, -1, dkw["scale"])
    FP = K.FocalParams(fkw["gamma"], fkw["alpha"], Cn, fkw["scale"])

    def fn(al):
        levels = [(al.inp("logits%d" % i, x), al.inp("teacher%d" % i, q), al.inp("labels%d" % i, g))
                  for i, (x, q, g) in enumerate(lv)]
        norm, fg = al.inp("normalizer", np.array([37.5], np.float32)), al.inp("fg", np.array([11.0], np.float32))
        res = {}
        nb = Lb.ssad_cls_losses_fused_workspace_bytes(3)
        ws = al.ws(nb, "clsfused")
        ws.zero_()
        for run in (0, 1):
            outs = [al.out("cdx%d_run%d" % (i, run), x.shape) for i, (x, _, _) in enumerate(lv)]
            dl, fl = al.out("distill_run%d" % run, 3), al.out("focal_run%d" % run, 3)
            arr = K._distill_levels(levels, outs)
            ok(Lb.ssad_cls_losses_fused_prezeroed(arr, 3, norm.data_ptr(), fg.data_ptr(), C.byref(DP), C.byref(FP),
                                                  dl.data_ptr(), fl.data_ptr(), ws.data_ptr(), nb, stream()))
            res.update({"distill%d" % run: dl, "focal%d" % run: fl}, **{"cdx%d_%d" % (i, run): t for i, t in enumerate(outs)})
        nbp = Lb.ssad_pow_sum_workspace_bytes(3)
        wsp = al.ws(nbp, "powsum")
        wsp.zero_()
        ptrs = (C.c_void_p * 3)(*[q.data_ptr() for _, q, _ in levels])
        sizes = (C.c_int64 * 3)(*[q.numel() for _, q, _ in levels])
        for run in (0, 1):
            out = al.out("powsum_run%d" % run, ())
            ok(Lb.ssad_pow_sum_prezeroed(ptrs, sizes, 3, 1.8, out.data_ptr(), wsp.data_ptr(), nbp, stream()))
            res["powsum%d" % run] = out
        # the self-zeroing forms on their own (dirty) workspaces
        d2, f2, dxs = K.cls_losses_fused(levels, norm, fg, dkw, fkw, out=[al.out("sdx%d" % i, x.shape) for i, (x, _, _) in enumerate(lv)],
                                         losses=(al.out("self_distill", 3), al.out("self_focal", 3)))
        res.update(self_distill=d2, self_focal=f2, self_powsum=K.pow_sum([q for _, q, _ in levels], 1.8, out=al.out("self_powsum", ())),
                   **{"sdx%d" % i: t for i, t in enumerate(dxs)})
        return res

    got = isolated_with_workspaces(K, fn)
    for run in (0, 1):
        for key, other in (("distill%d" % run, "self_distill"), ("focal%d" % run, "self_focal"), ("powsum%d" % run, "self_powsum")):
            assert np.array_equal(bits(got[key]), bits(got[other])), key
        for i in range(3):
            assert np.array_equal(bits(got["cdx%d_%d" % (i, run)]), bits(got["sdx%d" % i])), (i, run)
    for i, (x, q, g) in enumerate(lv):
        _, d64, _ = oracle.distill_loss_forward(x, q, g, 37.5, **dkw)
        _, f64, _ = oracle.focal_loss_forward(x, g, 11.0, **fkw)
        close(got["distill0"][i], d64, LOSS_RTOL, 0, "distill loss %d" % i)
        close(got["focal0"][i], f64, LOSS_RTOL, 0, "focal loss %d" % i)
        both = oracle.distill_loss_backward(x, q, g, 37.5, 1.0, **dkw) + oracle.focal_loss_backward(x, g, 11.0, 1.0, **fkw)
        close(got["cdx%d_0" % i], both, DX_RTOL, 2 * DX_FLOOR, "fused dX %d" % i)
    close(got["powsum0"], sum(np.sum(q.astype(np.float64) ** 1.8) for _, q, _ in lv), 1e-5, 0, "powsum")


def isolated_with_workspaces(K, fn):
    """isolated() with kernels.py's cached workspaces taken from the allocator too (K._workspace patched for the call)"""
    cached = K._workspace

    def wrapped(al):
        K._workspace = al.ws
        try:
            return fn(al)
        finally:
            K._workspace = cached

    return isolated(wrapped)[0]


def test_guarded_softmax_focal_loss_fused(K):
    """loss and dX in one pass over three levels (4095 / 33 / 420 logits at 3 classes), probabilities written for one
    level only; against the two-pass forms' definition in float64"""
    Cn = 3
    rng = np.random.default_rng(8200)
    maps = [(1, 1, 1, 1365), (1, 1, 1, 11), (2, 2, 5, 7)]
    xs = [randn(rng, n, a * Cn, h, w, scale=2.0) for n, a, h, w in maps]
    labs = [rng.integers(-1, Cn, size=(n, a, h, w)).astype(np.int32) for n, a, h, w in maps]
    kw = dict(gamma=2.0, alpha=0.25, num_classes=Cn, scale=0.5)

    def fn(al):
        tx = [al.inp("logits%d" % i, x) for i, x in enumerate(xs)]
        tl = [al.inp("labels%d" % i, g) for i, g in enumerate(labs)]
        fg = al.inp("fg", np.array([11.0], np.float32))
        nb = K.lib().ssad_softmax_focal_loss_fused_workspace_bytes(3)
        probs = [None, None, al.out("prob2", xs[2].shape)]
        losses, dxs = K.softmax_focal_loss_fused(list(zip(tx, tl)), fg, dloss=2.0, probs=probs,
                                                 out=(al.out("loss", 3), [al.out("dx%d" % i, x.shape) for i, x in enumerate(xs)]),
                                                 workspace=al.ws(nb, "softmaxfocal"), **kw)
        return dict(loss=losses, prob2=probs[2], **{"dx%d" % i: t for i, t in enumerate(dxs)})

    got, _ = isolated(fn)
    for i, ((n, a, h, w), x, g) in enumerate(zip(maps, xs, labs)):
        z = torch.tensor(x.astype(np.float64).reshape(n, a, Cn, h, w), requires_grad=True)
        p = torch.softmax(z, 2)
        t = torch.tensor(np.clip(g, 0, None).astype(np.int64))
        pt = torch.gather(p, 2, t[:, :, None])[:, :, 0]
        wgt = torch.tensor(np.where(g > 0, 0.25, 0.75) * (g >= 0))
        loss = (-wgt * (1 - pt) ** 2.0 * torch.log(pt)).sum() * 0.5 / 11.0
        loss.backward()
        close(float(got["loss"][i]), float(loss.detach()), LOSS_RTOL, 0, "softmax focal loss %d" % i)
        close(got["dx%d" % i], 2.0 * z.grad.numpy().reshape(x.shape), DX_RTOL, DX_FLOOR, "dX %d" % i)
        if i == 2:
            close(got["prob2"], p.detach().numpy().reshape(x.shape), 1e-5, 1e-7, "probabilities")


# ---------------------------------------------------------------------------------------------------------------------
# the batched packers: a table of three entries, one ragged, against the single-entry launchers
# ---------------------------------------------------------------------------------------------------------------------

def test_guarded_transpose_filters_table(K):
    """ssad_transpose_filters over (M, K) = (8, 16), (70, 45) -- ldm = 72, two zero columns per row -- and (128, 64):
    bit-identical to ssad_transpose_filter entry by entry, equal to the transposition with zero padding"""
    Lb = K.lib()
    dims = [(8, 16), (70, 45), (128, 64)]
    rng = np.random.default_rng(9700)
    Ws = [randn(rng, m, k) for m, k in dims]

    def fn(al):
        tw = [al.inp("w%d" % i, w) for i, w in enumerate(Ws)]
        table = [al.out("table_wt%d" % i, (k, (m + 3) // 4 * 4)) for i, (m, k) in enumerate(dims)]
        single = [al.out("single_wt%d" % i, (k, (m + 3) // 4 * 4)) for i, (m, k) in enumerate(dims)]
        tab = (K.TransposeEntry * 3)(*[K.TransposeEntry(w.data_ptr(), t.data_ptr(), m, k, (m + 3) // 4 * 4, 0)
                                       for w, t, (m, k) in zip(tw, table, dims)])
        ok(Lb.ssad_transpose_filters(tab, 3, stream()))
        for w, t, (m, k) in zip(tw, single, dims):
            ok(Lb.ssad_transpose_filter(w.data_ptr(), m, k, (m + 3) // 4 * 4, t.data_ptr(), stream()))
        return dict(**{"table%d" % i: t for i, t in enumerate(table)}, **{"single%d" % i: t for i, t in enumerate(single)})

    got, _ = isolated(fn)
    for i, (w, (m, k)) in enumerate(zip(Ws, dims)):
        want = np.zeros((k, (m + 3) // 4 * 4), np.float32)
        want[:, :m] = w.T
        assert np.array_equal(bits(got["table%d" % i]), bits(got["single%d" % i])), i
        assert np.array_equal(bits(got["table%d" % i]), bits(want)), i


def test_guarded_conv_wino_pack_filters_table(K):
    """ssad_conv_wino_pack_filters over (Cout, Cin) = (8, 16), (70, 37) and (128, 64), forward and data-gradient packs
    (the second entry without a data-gradient pack): bit-identical to ssad_conv_wino_pack_filter entry by entry, the
    never-written padding of a pack included (it holds the sentinel in both), and a forward through the packed table
    meets the convolution bar"""
    Lb = K.lib()
    dims = [(8, 16), (70, 37), (128, 64)]
    rng = np.random.default_rng(9800)
    Ws = [randn(rng, m, c, 3, 3, scale=(9 * c) ** -0.5) for m, c in dims]
    X = randn(rng, 2, 37, 5, 6)
    floats = Lb.ssad_conv_wino_filter_floats
    names = []

    def fn(al):
        tw = [al.inp("w%d" % i, w) for i, w in enumerate(Ws)]
        packs = {}
        for kind in ("table", "single"):
            for i, (m, c) in enumerate(dims):
                packs[kind, i, "f"] = al.out("%s_fwd%d" % (kind, i), floats(m, c))
                packs[kind, i, "d"] = al.out("%s_dgrad%d" % (kind, i), floats(c, m)) if i != 1 else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        tab = (K.PackEntry * 3)(*[K.PackEntry(w.data_ptr(), m, c, ptr(packs["table", i, "f"]), ptr(packs["table", i, "d"]))
                                  for i, (w, (m, c)) in enumerate(zip(tw, dims))])
        ok(Lb.ssad_conv_wino_pack_filters(tab, 3, stream()))
        for i, (w, (m, c)) in enumerate(zip(tw, dims)):
            ok(Lb.ssad_conv_wino_pack_filter(w.data_ptr(), m, c, ptr(packs["single", i, "f"]), ptr(packs["single", i, "d"]),
                                             stream()))
        y = al.out("y", (2, 70, 5, 6))
        K.conv3x3_forward([al.inp("x", X)], packs["table", 1, "f"], None, 70, wino=True, out=[y])
        return dict(y=y)

    for kind in ("table", "single"):
        for i in range(3):
            names += ["%s_fwd%d" % (kind, i)] + (["%s_dgrad%d" % (kind, i)] if i != 1 else [])
    got, arena = isolated(fn, nan_ok={n: True for n in names})
    for n in names:
        if n.startswith("table"):
            a, b = arena[n].cpu().numpy(), arena[n.replace("table", "single")].cpu().numpy()
            assert np.array_equal(bits(a), bits(b)), n
            assert not np.array_equal(bits(a), np.tile(bits(np.array([0x7FC0A5A5], np.uint32)), a.size)), n + " not written"
    close(got["y"], oracle.conv_forward(X, Ws[1], None), CONV_RTOL, CONV_FLOOR, "forward through the table's pack")
