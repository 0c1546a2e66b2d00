"""Kernel isolation of the fp16-storage family (conv3x3_f16.hip, gemm_f16.hip, grouped_f16.hip: BASELINE config 5).

Part A -- every operand, output and workspace of a launch is a view of ONE sentinel-filled arena (tests/guarded.py),
the workspace exactly *_workspace_bytes long and that length passed.  After the launch: guards intact, inputs
bit-identical, outputs fully written (filter packs may keep sentinel in their padding: it then holds a NaN in every odd
half, so a kernel that multiplies padding into a result fails its comparison), bit equality with the same call on
ordinary allocations, and the family's own bar against float64 on the same fp16-rounded operands:
  6e-4 of the output scale for blocked fp16 results of the 3x3 kernels, 2e-5 for fp32 results (NCHW outputs, dw, db),
  test_gpu_f16_backbone._close (1.5e-3) for the backbone kernels, exact for packers, casts and elementwise passes
  (EW_SUM2 / upsample-grad: the float64 sum rounded once).
Shapes are the smallest that cross each kernel's internal boundaries: a half-used 8-block (C = 37), a K chunk holding
one block of four, a second 128-block of 8 channels (M = 136), M off the block (37, 65), pixel tiles that cross an image
boundary, and the 256-pixel instantiation of the pointwise kernel sized from the device's CU count.

Part B -- one fp16 NaN, then one +Inf, planted in a blocked operand (the three positions of test_gpu_isolation.py):
the kernel's non-finite set equals the set the operation's definition gives, and everything finite is held to the
float64 reference computed without the planted value.  These kernels are direct: no tile enlargement.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_isolation import Plain, Guarded, isolated, bits, refused, plants  # noqa: E402,F401
from test_gpu_f16 import _conv64, _r16  # noqa: E402
from test_gpu_f16_backbone import _close  # noqa: E402

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
BLOCKED_TOL, F32_TOL = 6e-4, 2e-5


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ssad_amd import kernels
    kernels.lib()  # raises if the HIP extension is missing: no fallback
    return kernels


def sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def ok(rc):
    assert rc == 0, "launcher returned %d" % rc


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def randn(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


# ---- the layouts, in numpy ------------------------------------------------------------------------------------------

def blk(a):
    """NCHW -> blocked fp16 [N][ceil(C/8)][H][W][8], the tail lanes zero"""
    N, Cc, H, W = a.shape
    CB = (Cc + 7) // 8
    full = np.zeros((N, CB * 8, H, W), np.float16)
    full[:, :Cc] = a.astype(np.float16)
    return np.ascontiguousarray(full.reshape(N, CB, 8, H, W).transpose(0, 1, 3, 4, 2))


def unblk(b, Cc):
    N, CB, H, W, _ = b.shape
    return np.ascontiguousarray(b.transpose(0, 1, 4, 2, 3).reshape(N, CB * 8, H, W)[:, :Cc])


def packn(w):
    """[M][C][T] -> [T][ceil(C/8)][M][8] fp16, the tail lanes zero (T = 9: ssad_f16_pack_filter's forward pack; T = 1:
    ssad_pw_f16_pack_filter's)"""
    M, Cc, T = w.shape
    CB = (Cc + 7) // 8
    full = np.zeros((M, CB * 8, T), np.float16)
    full[:, :Cc] = w.astype(np.float16)
    return np.ascontiguousarray(full.reshape(M, CB, 8, T).transpose(3, 1, 0, 2)).reshape(-1)


def flipped(w):
    """the data gradient's filter: [M][C][3][3] -> [C][M][3][3] with the taps reversed"""
    return np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))


def pack3(w):
    return packn(w.reshape(w.shape[0], w.shape[1], 9))


def pack3d(w):
    return pack3(flipped(w))


def bar(got, want, tol, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.all(np.isfinite(got)), "%s: non-finite outputs" % what
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    assert err <= tol * scale, "%s: max abs err %.3e of the scale (bar %.1e)" % (what, err / scale, tol)


def close_bb(got, want, what):
    _close(torch.from_numpy(np.asarray(got, np.float64)), torch.from_numpy(np.asarray(want, np.float64)), what)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def pw(K, x, w, y, Cin, M, bias=None, res=None, mask=None, relu=False, res_up=False, stride=1):
    """ssad_conv1x1_f16 on blocked tensors; returns the launcher's code"""
    d = K.PwF16()
    d.x, d.w, d.y = x.data_ptr(), w.data_ptr(), y.data_ptr()
    d.bias = bias.data_ptr() if bias is not None else None
    d.residual = res.data_ptr() if res is not None else None
    d.mask = mask.data_ptr() if mask is not None else None
    d.N, d.C, d.M, d.Ho, d.Wo, d.Hi, d.Wi, d.stride = x.shape[0], Cin, M, y.shape[2], y.shape[3], x.shape[2], x.shape[3], stride
    d.flags = (K.CONV_RELU if relu else 0) | (K.PW_F16_RES_UPSAMPLE2 if res_up else 0)
    return K.lib().ssad_conv1x1_f16(C.byref(d), sp())


def pw64(x, w):
    return np.einsum("mc,nchw->nmhw", _r16(w), _r16(x))


# ---------------------------------------------------------------------------------------------------------------------
# Part A: packers and casts
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cc", [1, 7, 8, 9, 37])
def test_guarded_f16_activation_packers(K, monkeypatch, Cc):
    """ssad_f16_pack_activations / _unpack_, both _dyn variants with a device scale and with NULL, ssad_f16_block_ /
    _unblock_activations: exact (power-of-two scales), the tail lanes of the last block written as zero"""
    L = K.lib()
    N, H, W = 2, 5, 7
    CB = (Cc + 7) // 8
    X = randn(np.random.default_rng(100 + Cc), N, Cc, H, W)
    X16 = X.astype(np.float16)
    geo = (N, Cc, H, W)

    def fn(al):
        x, x16, sd = al.inp("x", X), al.inp("x16", X16), al.inp("scale_dev", np.array([0.25], np.float32))
        xb, xbd, xb0, xbb = (al.out(n, (N, CB, H, W, 8), F16) for n in ("xb", "xb_dyn", "xb_dyn_null", "xb_block"))
        ok(L.ssad_f16_pack_activations(p(x), *geo, 2.0, p(xb), sp()))
        ok(L.ssad_f16_pack_activations_dyn(p(x), *geo, C.c_float(2.0), p(sd), p(xbd), sp()))
        ok(L.ssad_f16_pack_activations_dyn(p(x), *geo, C.c_float(2.0), p(None), p(xb0), sp()))
        ok(L.ssad_f16_block_activations(p(x16), *geo, p(xbb), sp()))
        xu, xud, xu0 = (al.out(n, geo, F32) for n in ("xu", "xu_dyn", "xu_dyn_null"))
        ok(L.ssad_f16_unpack_activations(p(xb), *geo, 0.5, p(xu), sp()))
        ok(L.ssad_f16_unpack_activations_dyn(p(xb), *geo, C.c_float(2.0), p(sd), p(xud), sp()))
        ok(L.ssad_f16_unpack_activations_dyn(p(xb), *geo, C.c_float(0.5), p(None), p(xu0), sp()))
        x16u = al.out("x16_unblocked", geo, F16)
        ok(L.ssad_f16_unblock_activations(p(xbb), *geo, p(x16u), sp()))
        return dict(xb=xb, xbd=xbd, xb0=xb0, xbb=xbb, xu=xu, xud=xud, xu0=xu0, x16u=x16u)

    got = isolated(K, monkeypatch, fn)
    assert same(got["xb"], blk(X * np.float32(2))) and same(got["xb0"], got["xb"])        # zero tails included
    assert same(got["xbd"], blk(X * np.float32(0.5)))
    assert same(got["xbb"], blk(X16)) and same(got["x16u"], X16)
    back = (X * np.float32(2)).astype(np.float16).astype(np.float32) * np.float32(0.5)
    assert same(got["xu"], back) and same(got["xud"], back) and same(got["xu0"], back)


@pytest.mark.parametrize("n,skewed", [(1, False), (5, False), (1023, False), (1023, True)],
                         ids=["n1", "n5", "n1023", "n1023_skewed"])
def test_guarded_f16_casts(K, monkeypatch, n, skewed):
    """ssad_cast_f32_to_f16 / _f16_to_f32; skewed: every view starts one element (2 / 4 bytes) into its slot"""
    L = K.lib()
    rng = np.random.default_rng(200 + n)
    a32, a16 = randn(rng, n), randn(rng, n).astype(np.float16)
    s2, s4 = (2, 4) if skewed else (0, 0)

    def fn(al):
        y16, y32 = al.out("y16", (n,), F16, skew=s2), al.out("y32", (n,), F32, skew=s4)
        ok(L.ssad_cast_f32_to_f16(p(al.inp("x32", a32, skew=s4)), p(y16), C.c_longlong(n), sp()))
        ok(L.ssad_cast_f16_to_f32(p(al.inp("x16", a16, skew=s2)), p(y32), C.c_longlong(n), sp()))
        return dict(y16=y16, y32=y32)

    got = isolated(K, monkeypatch, fn)
    assert same(got["y16"], a32.astype(np.float16)) and same(got["y32"], a16.astype(np.float32))


@pytest.mark.parametrize("M,Cc", [(40, 37), (8, 8), (136, 72)], ids=lambda v: str(v))
def test_guarded_f16_filter_packs_and_their_use(K, monkeypatch, M, Cc):
    """ssad_f16_pack_filter, ssad_pw_f16_pack_filter and ssad_f16_pack_filters (three entries: taps 9 / 1 / 9, the
    last with wd only): the written part exact, the batched packs bit-equal to the single ones; then each batched pack
    feeds a convolution (3 x 4 map) with the sentinel NaNs of its padding -- and of the guard behind it -- in place"""
    L = K.lib()
    rng = np.random.default_rng(300 + M + Cc)
    W3, W1 = randn(rng, M, Cc, 3, 3, scale=(9 * Cc) ** -0.5), randn(rng, M, Cc, scale=Cc ** -0.5)
    N, H, Wd = 1, 3, 4
    X, dY = randn(rng, N, Cc, H, Wd), randn(rng, N, M, H, Wd)
    n3, n1 = L.ssad_f16_filter_halves(M, Cc), L.ssad_pw_f16_filter_halves(M, Cc)
    want = dict(f3=pack3(W3), d3=pack3d(W3), f1=packn(W1.reshape(M, Cc, 1)), d1=packn(W1.T.reshape(Cc, M, 1)))
    assert all(len(v) <= (n3 if k.endswith("3") else n1) for k, v in want.items())
    dgrad_blocked = Cc % 8 == 0

    def fn(al):
        w3, w1 = al.inp("w3", W3), al.inp("w1", W1)
        s = {k: al.out(k, (n3 if "3" in k else n1,), F16)
             for k in ("f3", "d3", "f1", "d1", "batch_f3", "batch_d3", "batch_f1", "batch_d1", "batch_d3_only")}
        ok(L.ssad_f16_pack_filter(p(w3), M, Cc, p(s["f3"]), p(s["d3"]), sp()))
        ok(L.ssad_pw_f16_pack_filter(p(w1), M, Cc, p(s["f1"]), p(s["d1"]), sp()))
        tab = (K.F16PackEntry * 3)(
            K.F16PackEntry(w3.data_ptr(), s["batch_f3"].data_ptr(), s["batch_d3"].data_ptr(), M, Cc, 9, 0),
            K.F16PackEntry(w1.data_ptr(), s["batch_f1"].data_ptr(), s["batch_d1"].data_ptr(), M, Cc, 1, 0),
            K.F16PackEntry(w3.data_ptr(), None, s["batch_d3_only"].data_ptr(), M, Cc, 9, 0))
        ok(L.ssad_f16_pack_filters(tab, 3, sp()))
        res = {k: t[:len(want[k.replace("batch_", "").replace("_only", "")])] for k, t in s.items()}      # the written part
        xb, dyb = al.inp("xb", blk(X)), al.inp("dyb", blk(dY))
        res["y3"] = K.conv3x3_forward_f16(xb, s["batch_f3"], None, Cc, M, out_nchw_f32=True, out=al.out("y3", (N, M, H, Wd)))
        res["dx3"] = K.conv3x3_forward_f16(dyb, s["batch_d3_only"], None, M, Cc, out_nchw_f32=True,
                                           out=al.out("dx3", (N, Cc, H, Wd)))
        res["y1"] = al.out("y1", (N, M // 8, H, Wd, 8), F16)
        ok(pw(K, xb, s["batch_f1"], res["y1"], Cc, M))
        if dgrad_blocked:
            res["dx1"] = al.out("dx1", (N, Cc // 8, H, Wd, 8), F16)
            ok(pw(K, dyb, s["batch_d1"], res["dx1"], M, Cc))
        return res

    packs = ("f3", "d3", "f1", "d1", "batch_f3", "batch_d3", "batch_f1", "batch_d1", "batch_d3_only")
    got = isolated(K, monkeypatch, fn, nan_ok={k: True for k in packs})
    for k in packs:
        assert same(got[k], want[k.replace("batch_", "").replace("_only", "")]), k
    bar(got["y3"], _conv64(_r16(X), _r16(W3), None), F32_TOL, "3x3 on the batched forward pack")
    bar(got["dx3"], _conv64(_r16(dY), _r16(flipped(W3)), None), F32_TOL, "3x3 data gradient on the wd-only entry")
    close_bb(unblk(got["y1"], M), pw64(X, W1), "pointwise on the batched pack")
    if dgrad_blocked:
        close_bb(unblk(got["dx1"], Cc), pw64(dY, W1.T), "pointwise data gradient on the batched pack")
    else:                                   # a blocked output needs whole 8-blocks
        y = torch.empty((N, (Cc + 7) // 8, H, Wd, 8), dtype=F16, device="cuda")
        assert pw(K, dev(blk(dY)), torch.zeros(n1, dtype=F16, device="cuda"), y, M, Cc) == -1
    tab = (K.F16PackEntry * 1)(K.F16PackEntry(dev(W1).data_ptr(), None, None, M, Cc, 1, 0))
    assert L.ssad_f16_pack_filters(tab, 1, sp()) == -1


# ---------------------------------------------------------------------------------------------------------------------
# Part A: 3x3 forward / data gradient
# ---------------------------------------------------------------------------------------------------------------------

SHAPE_ID = "N%d_C%d_M%d_%dx%d"
FWD_CASES = [(2, 37, 40, 9, 17),       # half-used block, a second chunk of ONE block, an idle wo = 1 wave, a one-column x tile
             (3, 8, 136, 2, 31),       # a second 128-block of 8 channels; a chunk of one block (taps 6..8 address memory behind the pack)
             (2, 40, 37, 7, 9)]        # M off the block: NCHW fp32 only


@pytest.mark.parametrize("shape", FWD_CASES, ids=lambda s: SHAPE_ID % s)
def test_guarded_conv3x3_forward_f16(K, monkeypatch, shape):
    """bias + ReLU blocked; NCHW fp32 with and without the sigmoid; the masked data-gradient form (packed_dgrad, aux)
    with dY of C channels and dX of M"""
    L = K.lib()
    N, Cc, M, H, W = shape
    blocked = M % 8 == 0
    rng = np.random.default_rng(400 + sum(shape))
    X, Wt, b = randn(rng, N, Cc, H, W), randn(rng, M, Cc, 3, 3, scale=(9 * Cc) ** -0.5), randn(rng, M, scale=0.3)
    Wg, mask = randn(rng, Cc, M, 3, 3, scale=(9 * Cc) ** -0.5), np.maximum(randn(rng, N, M, H, W), 0)

    def fn(al):
        pf = al.out("packed_fwd", (L.ssad_f16_filter_halves(M, Cc),), F16)
        ok(L.ssad_f16_pack_filter(p(al.inp("w", Wt)), M, Cc, p(pf), p(None), sp()))
        xb, bias = al.inp("xb", blk(X)), al.inp("bias", b)
        res = dict(yn=K.conv3x3_forward_f16(xb, pf, bias, Cc, M, out_nchw_f32=True, out=al.out("y_nchw", (N, M, H, W))),
                   ys=K.conv3x3_forward_f16(xb, pf, bias, Cc, M, sigmoid=True, out_nchw_f32=True,
                                            out=al.out("y_sigmoid", (N, M, H, W))))
        if blocked:
            res["yb"] = K.conv3x3_forward_f16(xb, pf, bias, Cc, M, relu=True, out=al.out("y_blocked", (N, M // 8, H, W, 8), F16))
            pd = al.out("packed_dgrad", (L.ssad_f16_filter_halves(Cc, M),), F16)
            ok(L.ssad_f16_pack_filter(p(al.inp("w_dgrad", Wg)), Cc, M, p(None), p(pd), sp()))
            res["dx"] = K.conv3x3_forward_f16(xb, pd, None, Cc, M, mask_by=al.inp("mask", blk(mask)),
                                              out=al.out("dx", (N, M // 8, H, W, 8), F16))
        return res

    got = isolated(K, monkeypatch, fn, nan_ok={"packed_fwd": True, "packed_dgrad": True} if blocked else {"packed_fwd": True})
    ref = _conv64(_r16(X), _r16(Wt), b.astype(np.float64))
    bar(got["yn"], ref, F32_TOL, "NCHW fp32")
    assert np.abs(got["ys"] - 1.0 / (1.0 + np.exp(-ref))).max() <= F32_TOL, "sigmoid"
    if blocked:
        bar(unblk(got["yb"], M), np.maximum(ref, 0), BLOCKED_TOL, "relu(Y) blocked")
        assert not np.any(got["yb"].astype(np.float32) < 0)
        rdx = _conv64(_r16(X), _r16(flipped(Wg)), None)
        m16 = mask.astype(np.float16)
        dx = unblk(got["dx"], M)
        bar(dx, np.where(m16 > 0, rdx, 0), BLOCKED_TOL, "masked data gradient")
        assert np.all(dx[m16 <= 0] == 0)
    else:
        refused(K, lambda: K.conv3x3_forward_f16(dev(blk(X)), torch.zeros(L.ssad_f16_filter_halves(M, Cc), dtype=F16, device="cuda"),
                                                 None, Cc, M))
        refused(K, lambda: K.conv3x3_forward_f16(dev(blk(X)), torch.zeros(L.ssad_f16_filter_halves(M, Cc), dtype=F16, device="cuda"),
                                                 None, Cc, 40, sigmoid=True))


LEVELS2 = [(2, 7, 9), (2, 2, 3)]


def test_guarded_conv3x3_forward_f16_levels_and_multi(K, monkeypatch):
    """two levels (7 x 9 and 2 x 3) sharing a filter in one launch, and two independent problems x two levels with
    per-entry filter and bias: both bit-equal to the single calls"""
    L = K.lib()
    Cc, M = 37, 40
    rng = np.random.default_rng(500)
    Xs = [[randn(rng, n, Cc, h, w) for n, h, w in LEVELS2] for _ in range(2)]
    Ws = [randn(rng, M, Cc, 3, 3, scale=(9 * Cc) ** -0.5) for _ in range(2)]
    bs = [randn(rng, M, scale=0.3) for _ in range(2)]

    def fn(al):
        res, probs = {}, []
        for q in range(2):
            pf = al.out("packed%d" % q, (L.ssad_f16_filter_halves(M, Cc),), F16)
            ok(L.ssad_f16_pack_filter(p(al.inp("w%d" % q, Ws[q])), M, Cc, p(pf), p(None), sp()))
            xs = [al.inp("x%d_%d" % (q, l), blk(x)) for l, x in enumerate(Xs[q])]
            new = lambda tag: [al.out("%s%d_%d" % (tag, q, l), (x.shape[0], M // 8) + x.shape[2:] + (8,), F16)
                               for l, x in enumerate(Xs[q])]
            bias = al.inp("bias%d" % q, bs[q])
            single = [K.conv3x3_forward_f16(x, pf, bias, Cc, M, relu=True, out=o) for x, o in zip(xs, new("single"))]
            probs.append(dict(xs=xs, packed=pf, bias=bias, out=new("multi")))
            res.update({"single%d_%d" % (q, l): t for l, t in enumerate(single)})
            res.update({"multi%d_%d" % (q, l): t for l, t in enumerate(probs[q]["out"])})
            if q == 0:
                lv = K.conv3x3_forward_f16_levels(xs, pf, bias, Cc, M, new("levels"), relu=True)
                res.update({"levels0_%d" % l: t for l, t in enumerate(lv)})
        K.conv3x3_forward_f16_multi(probs, Cc, M, relu=True)
        return res

    got = isolated(K, monkeypatch, fn, nan_ok={"packed0": True, "packed1": True})
    for q in range(2):
        for l, x in enumerate(Xs[q]):
            ref = np.maximum(_conv64(_r16(x), _r16(Ws[q]), bs[q].astype(np.float64)), 0)
            bar(unblk(got["single%d_%d" % (q, l)], M), ref, BLOCKED_TOL, "problem %d level %d" % (q, l))
            assert same(got["multi%d_%d" % (q, l)], got["single%d_%d" % (q, l)]), "multi differs from the single call"
            if q == 0:
                assert same(got["levels0_%d" % l], got["single0_%d" % l]), "levels differ from the single call"


# ---------------------------------------------------------------------------------------------------------------------
# Part A: filter gradients
# ---------------------------------------------------------------------------------------------------------------------

def wgrad64(x, dy, taps=3):
    xr, dyr = _r16(x), _r16(dy)
    if taps == 1:
        return np.einsum("nmhw,nchw->mc", dyr, xr)
    N, Cc, H, W = x.shape
    xp = np.zeros((N, Cc, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = xr
    out = np.zeros((dy.shape[1], Cc, 3, 3))
    for ky in range(3):
        for kx in range(3):
            out[:, :, ky, kx] = np.einsum("nmhw,nchw->mc", dyr, xp[:, :, ky:ky + H, kx:kx + W])
    return out


WGRAD_CASES = [((2, 37, 40), [(9, 17)]), ((3, 8, 65), [(2, 31)]), ((2, 37, 136), [(7, 9), (2, 3)])]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=["N2_C37_M40_9x17", "N3_C8_M65_2x31", "N2_C37_M136_7x9+2x3"])
def test_guarded_conv3x3_wgrad_f16(K, monkeypatch, case):
    """ssad_conv3x3_wgrad_f16 (one level), _levels and _levels_dyn: written with scale 0.5, then accumulate = 1; the same
    scale as 2.0 x scale_dev[0] = 0.25; db NULL.  dw [M][C][3][3] and db [M] are exactly sized fp32, the operands
    block-padded."""
    L = K.lib()
    (N, Cc, M), maps = case
    n = len(maps)
    rng = np.random.default_rng(600 + Cc + M)
    Xs, dYs = [randn(rng, N, Cc, h, w) for h, w in maps], [randn(rng, N, M, h, w) for h, w in maps]
    baseW, baseb = randn(rng, M, Cc, 3, 3), randn(rng, M)

    def fn(al):
        xs = [al.inp("x%d" % l, blk(x)) for l, x in enumerate(Xs)]
        dys = [al.inp("dy%d" % l, blk(d)) for l, d in enumerate(dYs)]
        arr = (K.F16WgradLevel * n)()
        for l, (h, w) in enumerate(maps):
            arr[l].x, arr[l].dy, arr[l].N, arr[l].H, arr[l].W = xs[l].data_ptr(), dys[l].data_ptr(), N, h, w
        nb = L.ssad_conv3x3_wgrad_f16_levels_workspace_bytes(arr, n, Cc, M)
        sd = al.inp("scale_dev", np.array([0.25], np.float32))
        dW, db = al.out("dW", (M, Cc, 3, 3)), al.out("db", (M,))
        aW, ab = al.inp("dW_acc", baseW), al.inp("db_acc", baseb)
        dW2, dW3 = al.out("dW_dyn_no_db", (M, Cc, 3, 3)), al.out("dW_levels", (M, Cc, 3, 3))
        db3 = al.out("db_levels", (M,))
        if n == 1:
            (h, w) = maps[0]
            assert nb == L.ssad_conv3x3_wgrad_f16_workspace_bytes(N, Cc, h, w, M)
            ok(L.ssad_conv3x3_wgrad_f16(p(xs[0]), p(dys[0]), N, Cc, h, w, M, 0, 0.5, p(dW), p(db), p(al.ws(nb, "wgrad")), nb, sp()))
            ok(L.ssad_conv3x3_wgrad_f16(p(xs[0]), p(dys[0]), N, Cc, h, w, M, 1, 0.5, p(aW), p(ab), p(al.ws(nb, "wgrad")), nb, sp()))
        else:
            ok(L.ssad_conv3x3_wgrad_f16_levels(arr, n, Cc, M, 0, 0.5, p(dW), p(db), p(al.ws(nb, "wgrad")), nb, sp()))
            ok(L.ssad_conv3x3_wgrad_f16_levels(arr, n, Cc, M, 1, 0.5, p(aW), p(ab), p(al.ws(nb, "wgrad")), nb, sp()))
        ok(L.ssad_conv3x3_wgrad_f16_levels_dyn(arr, n, Cc, M, 0, C.c_float(2.0), p(sd), p(dW2), p(None), p(al.ws(nb, "wgrad")),
                                               C.c_size_t(nb), sp()))
        ok(L.ssad_conv3x3_wgrad_f16_levels(arr, n, Cc, M, 0, 0.5, p(dW3), p(db3), p(al.ws(nb, "wgrad")), nb, sp()))
        assert L.ssad_conv3x3_wgrad_f16_levels(arr, n, Cc, M, 0, 0.5, p(dW3), p(db3), p(al.ws(nb, "short")), nb - 1, sp()) != 0
        return dict(dW=dW, db=db, aW=aW, ab=ab, dW2=dW2, dW3=dW3, db3=db3)

    got = isolated(K, monkeypatch, fn, modified=("dW_acc", "db_acc"))
    rW = 0.5 * sum(wgrad64(x, d) for x, d in zip(Xs, dYs))
    rb = 0.5 * sum(_r16(d).sum((0, 2, 3)) for d in dYs)
    bar(got["dW"], rW, F32_TOL, "dW")
    bar(got["db"], rb, F32_TOL, "db")
    bar(got["aW"], rW + baseW, F32_TOL, "dW accumulated")
    bar(got["ab"], rb + baseb, F32_TOL, "db accumulated")
    assert same(got["dW2"], got["dW"]) and same(got["dW3"], got["dW"]) and same(got["db3"], got["db"])


@pytest.mark.parametrize("shape", [(2, 37, 40, 5, 5), (2, 72, 136, 9, 11)], ids=lambda s: SHAPE_ID % s)
def test_guarded_conv1x1_wgrad_f16(K, monkeypatch, shape):
    """with scale_dev and without; written, accumulated; db NULL"""
    L = K.lib()
    N, Cc, M, H, W = shape
    rng = np.random.default_rng(700 + sum(shape))
    X, dY, baseW, baseb = randn(rng, N, Cc, H, W), randn(rng, N, M, H, W), randn(rng, M, Cc), randn(rng, M)
    nb = L.ssad_conv1x1_wgrad_f16_workspace_bytes(N, Cc, H, W, M)

    def fn(al):
        x, dy, sd = al.inp("x", blk(X)), al.inp("dy", blk(dY)), al.inp("scale_dev", np.array([0.25], np.float32))
        call = lambda acc, scale, s, dw, db, tag="wgrad": L.ssad_conv1x1_wgrad_f16(
            p(x), p(dy), N, Cc, H, W, M, acc, scale, p(s), p(dw), p(db), p(al.ws(nb, tag)), nb, sp())
        dW, db, dW2 = al.out("dW", (M, Cc)), al.out("db", (M,)), al.out("dW_no_scale_dev_no_db", (M, Cc))
        aW, ab = al.inp("dW_acc", baseW), al.inp("db_acc", baseb)
        ok(call(0, 2.0, sd, dW, db))
        ok(call(0, 0.5, None, dW2, None))
        ok(call(1, 0.5, None, aW, ab))
        return dict(dW=dW, db=db, dW2=dW2, aW=aW, ab=ab)

    got = isolated(K, monkeypatch, fn, modified=("dW_acc", "db_acc"))
    rW, rb = 0.5 * wgrad64(X, dY, taps=1), 0.5 * _r16(dY).sum((0, 2, 3))
    bar(got["dW"], rW, F32_TOL, "dW")
    bar(got["db"], rb, F32_TOL, "db")
    bar(got["aW"], rW + baseW, F32_TOL, "dW accumulated")
    bar(got["ab"], rb + baseb, F32_TOL, "db accumulated")
    assert same(got["dW2"], got["dW"])


# ---------------------------------------------------------------------------------------------------------------------
# Part A: pointwise
# ---------------------------------------------------------------------------------------------------------------------

def pw_pack(K, al, name, Wt, dgrad=False):
    L = K.lib()
    M, Cc = Wt.shape
    out = al.out(name, (L.ssad_pw_f16_filter_halves(M, Cc),), F16)
    ok(L.ssad_pw_f16_pack_filter(p(al.inp(name + "_w", Wt)), M, Cc, p(None if dgrad else out), p(out if dgrad else None), sp()))
    return out


@pytest.mark.parametrize("shape", [(2, 37, 40, 9, 12),       # 216 pixels: a partial second 128-tile, a tile crossing the image boundary
                                   (1, 72, 136, 5, 5)], ids=lambda s: SHAPE_ID % s)
def test_guarded_conv1x1_f16(K, monkeypatch, shape):
    """bias + residual + ReLU; the data-gradient form (packed_dgrad, dY of C channels, dX of M) with the ReluGradient
    mask and the shortcut's gradient as residual"""
    N, Cc, M, H, W = shape
    rng = np.random.default_rng(800 + sum(shape))
    X, Wt, b, R = randn(rng, N, Cc, H, W), randn(rng, M, Cc, scale=Cc ** -0.5), randn(rng, M, scale=0.3), randn(rng, N, M, H, W)
    Wg, mask = randn(rng, Cc, M, scale=Cc ** -0.5), np.maximum(randn(rng, N, M, H, W), 0)

    def fn(al):
        xb, r = al.inp("xb", blk(X)), al.inp("residual", blk(R))
        y, dx = al.out("y", (N, M // 8, H, W, 8), F16), al.out("dx", (N, M // 8, H, W, 8), F16)
        ok(pw(K, xb, pw_pack(K, al, "packed_fwd", Wt), y, Cc, M, bias=al.inp("bias", b), res=r, relu=True))
        ok(pw(K, xb, pw_pack(K, al, "packed_dgrad", Wg, dgrad=True), dx, Cc, M, res=r, mask=al.inp("mask", blk(mask))))
        return dict(y=y, dx=dx)

    got = isolated(K, monkeypatch, fn, nan_ok={"packed_fwd": True, "packed_dgrad": True})
    close_bb(unblk(got["y"], M), np.maximum(pw64(X, Wt) + b.reshape(1, -1, 1, 1).astype(np.float64) + _r16(R), 0),
             "bias + residual + relu")
    m16 = mask.astype(np.float16)
    dx = unblk(got["dx"], M)
    close_bb(dx, np.where(m16 > 0, pw64(X, Wg.T) + _r16(R), 0), "masked data gradient + sum")
    assert np.all(dx[m16 <= 0] == 0)


def test_guarded_conv1x1_f16_stride2_and_upsampled_residual(K, monkeypatch):
    """stride 2 from an odd map (9 x 13 -> 5 x 7) in the loader; SSAD_PW_F16_RES_UPSAMPLE2 (2 x 3 -> 4 x 6)"""
    N, Cc, M = 2, 37, 40
    rng = np.random.default_rng(900)
    X, Wt = randn(rng, N, Cc, 9, 13), randn(rng, M, Cc, scale=Cc ** -0.5)
    X2, coarse = randn(rng, N, Cc, 4, 6), randn(rng, N, M, 2, 3)

    def fn(al):
        pf = pw_pack(K, al, "packed", Wt)
        ys, yu = al.out("y_stride2", (N, M // 8, 5, 7, 8), F16), al.out("y_upsampled", (N, M // 8, 4, 6, 8), F16)
        ok(pw(K, al.inp("x", blk(X)), pf, ys, Cc, M, stride=2))
        ok(pw(K, al.inp("x2", blk(X2)), pf, yu, Cc, M, res=al.inp("coarse", blk(coarse)), res_up=True))
        return dict(ys=ys, yu=yu)

    got = isolated(K, monkeypatch, fn, nan_ok={"packed": True})
    close_bb(unblk(got["ys"], M), pw64(X[:, :, ::2, ::2], Wt), "stride 2")
    close_bb(unblk(got["yu"], M), pw64(X2, Wt) + _r16(coarse).repeat(2, axis=2).repeat(2, axis=3), "upsampled residual")
    y = torch.empty((N, M // 8, 3, 5, 8), dtype=F16, device="cuda")                       # odd output map: refused
    zeros = torch.zeros(K.lib().ssad_pw_f16_filter_halves(M, Cc), dtype=F16, device="cuda")
    assert pw(K, dev(blk(X2[:, :, :3, :5])), zeros, y, Cc, M, res=dev(blk(coarse)), res_up=True) == -1


def test_guarded_conv1x1_f16_256_pixel_tiles(K, monkeypatch):
    """the 256-pixel instantiation: the smallest N Ho Wo with ceil(px / 256) ceil(M / 128) >= 2 CUs (the launcher's
    rule), C = 8, M = 1032 (a ninth 128-block of 8 channels), ragged H and W"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N, Cc, M, W = 1, 8, 1032, 131
    mblocks = (M + 127) // 128
    tiles = (2 * cus + mblocks - 1) // mblocks
    H = ((tiles - 1) * 256 + 1 + W - 1) // W
    px = H * W
    assert (px + 255) // 256 * mblocks >= 2 * cus > (px - W + 255) // 256 * mblocks          # one row less takes 128
    rng = np.random.default_rng(1000)
    X, Wt, b = randn(rng, N, Cc, H, W), randn(rng, M, Cc, scale=Cc ** -0.5), randn(rng, M, scale=0.3)

    def fn(al):
        y = al.out("y", (N, M // 8, H, W, 8), F16)
        ok(pw(K, al.inp("xb", blk(X)), pw_pack(K, al, "packed", Wt), y, Cc, M, bias=al.inp("bias", b), relu=True))
        return dict(y=y)

    got = isolated(K, monkeypatch, fn, nan_ok={"packed": True})
    close_bb(unblk(got["y"], M), np.maximum(pw64(X, Wt) + b.reshape(1, -1, 1, 1).astype(np.float64), 0), "256-pixel tiles")


# ---------------------------------------------------------------------------------------------------------------------
# Part A: grouped, elementwise, stem pool
# ---------------------------------------------------------------------------------------------------------------------

def grouped64(x, w, b, cg):
    G = x.shape[1] // cg
    out = [_conv64(_r16(x[:, g * cg:(g + 1) * cg]), _r16(w[g * cg:(g + 1) * cg]), None) for g in range(G)]
    return np.concatenate(out, axis=1) + (b.reshape(1, -1, 1, 1).astype(np.float64) if b is not None else 0.0)


@pytest.mark.parametrize("cg", [4, 8, 16, 32])
def test_guarded_grouped_conv3x3_f16(K, monkeypatch, cg):
    L = K.lib()
    N, Cc, H, W = 2, 64, 7, 9
    G = Cc // cg
    rng = np.random.default_rng(1100 + cg)
    X, Wt, b = randn(rng, N, Cc, H, W), randn(rng, Cc, cg, 3, 3, scale=(9 * cg) ** -0.5), randn(rng, Cc, scale=0.2)
    nh = L.ssad_grouped_conv3x3_f16_filter_halves(Cc, G)
    assert nh > 0

    def fn(al):
        pf = al.out("packed", (nh,), F16)
        ok(L.ssad_grouped_conv3x3_f16_pack_filter(p(al.inp("w", Wt)), Cc, G, p(pf), sp()))
        xb, bias = al.inp("xb", blk(X)), al.inp("bias", b)
        yr, yl = al.out("y_relu", (N, Cc // 8, H, W, 8), F16), al.out("y_linear", (N, Cc // 8, H, W, 8), F16)
        ok(L.ssad_grouped_conv3x3_f16(p(xb), p(pf), p(bias), N, Cc, H, W, G, 1, p(yr), sp()))
        ok(L.ssad_grouped_conv3x3_f16(p(xb), p(pf), p(None), N, Cc, H, W, G, 0, p(yl), sp()))
        return dict(pf=pf, yr=yr, yl=yl)

    got = isolated(K, monkeypatch, fn)                      # the grouped pack has no padding: written completely
    close_bb(unblk(got["yr"], Cc), np.maximum(grouped64(X, Wt, b, cg), 0), "grouped, bias + relu")
    close_bb(unblk(got["yl"], Cc), grouped64(X, Wt, None, cg), "grouped, linear")
    if cg == 4:                                             # geometries the launcher refuses
        xb, pf, y = dev(blk(X)), dev(got["pf"]), torch.empty((N, Cc // 8, H, W, 8), dtype=F16, device="cuda")
        for c, g in ((64, 32), (64, 1), (64, 3), (32, 8), (96, 24)):        # cg = 2, cg = 64, C % group, C % 64
            assert L.ssad_grouped_conv3x3_f16(p(xb), p(pf), p(None), N, c, H, W, g, 0, p(y), sp()) == -1, (c, g)
            assert L.ssad_grouped_conv3x3_f16_pack_filter(p(dev(Wt)), c, g, p(pf), sp()) == -1, (c, g)


def test_guarded_f16_elementwise_and_subsample(K, monkeypatch):
    """all six modes of ssad_f16_elementwise and ssad_f16_subsample at N2 C37 7 x 9; subsample and its gradient at stride
    2 on the odd map (7 x 9 <-> 4 x 5), written and accumulated; upsample-grad with and without b"""
    L = K.lib()
    N, Cc, H, W = 2, 37, 7, 9
    CB = (Cc + 7) // 8
    rng = np.random.default_rng(1200)
    A, B, big, small = randn(rng, N, Cc, H, W), randn(rng, N, Cc, H, W), randn(rng, N, Cc, 2 * H, 2 * W), randn(rng, N, Cc, 4, 5)
    shape = lambda h, w: (N, CB, h, w, 8)

    def fn(al):
        a, b, bg, sm = al.inp("a", blk(A)), al.inp("b", blk(B)), al.inp("big", blk(big)), al.inp("small", blk(small))
        ew = lambda mode, x, y_, out, h, w, stride=1, acc=0: ok(L.ssad_f16_elementwise(
            mode, p(x), p(y_), p(out), N, Cc, h, w, stride, acc, sp()))
        res = {k: al.out(k, shape(*hw), F16) for k, hw in (
            ("sub_even", (H, W)), ("sub_odd", (4, 5)), ("subgrad", (H, W)), ("upgrad", (H, W)), ("upgrad_b", (H, W)),
            ("sum2", (H, W)), ("relu", (H, W)), ("relugrad", (H, W)))}
        res["subgrad_acc"] = al.inp("subgrad_acc", blk(B))
        ew(K.EW_SUBSAMPLE, bg, None, res["sub_even"], H, W, stride=2)
        ok(L.ssad_f16_subsample(p(a), N, Cc, H, W, 2, p(res["sub_odd"]), sp()))
        ew(K.EW_SUBSAMPLE_GRAD, sm, None, res["subgrad"], H, W, stride=2)
        ew(K.EW_SUBSAMPLE_GRAD, sm, None, res["subgrad_acc"], H, W, stride=2, acc=1)
        ew(K.EW_UPSAMPLE_GRAD, bg, None, res["upgrad"], H, W)
        ew(K.EW_UPSAMPLE_GRAD, bg, b, res["upgrad_b"], H, W)
        ew(K.EW_SUM2, a, b, res["sum2"], H, W)
        ew(K.EW_RELU, a, None, res["relu"], H, W)
        ew(K.EW_RELU_GRAD, a, b, res["relugrad"], H, W)
        return res

    got = isolated(K, monkeypatch, fn, modified=("subgrad_acc",))
    a16, b16, big16, small16 = (t.astype(np.float16) for t in (A, B, big, small))
    once = lambda a64: blk(a64.astype(np.float16))                          # float64, rounded once
    assert same(got["sub_even"], blk(big16[:, :, ::2, ::2])) and same(got["sub_odd"], blk(a16[:, :, ::2, ::2]))
    scat = np.zeros((N, Cc, H, W), np.float16)
    scat[:, :, ::2, ::2] = small16
    assert same(got["subgrad"], blk(scat))
    assert same(got["subgrad_acc"], once(b16.astype(np.float64) + scat))
    up = big16.astype(np.float64).reshape(N, Cc, H, 2, W, 2).sum(axis=(3, 5))
    assert same(got["upgrad"], once(up)), "upsample gradient"
    assert same(got["upgrad_b"], once(up + b16)), "upsample gradient + b: one rounding of the float64 sum"
    assert same(got["sum2"], once(a16.astype(np.float64) + b16))
    assert same(got["relu"], blk(np.maximum(a16, np.float16(0))))
    assert same(got["relugrad"], blk(np.where(a16 > 0, b16, np.float16(0))))


@pytest.mark.parametrize("Cc,H,W", [(8, 9, 11), (16, 8, 12)], ids=["C8_9x11", "C16_8x12"])
def test_guarded_stem_pool_f16(K, monkeypatch, Cc, H, W):
    L = K.lib()
    N = 2
    rng = np.random.default_rng(1300 + Cc)
    Z, b = randn(rng, N, Cc, H, W), randn(rng, Cc)
    oh, ow = (H + 1) // 2, (W + 1) // 2

    def fn(al):
        z, bias, y = al.inp("z", Z), al.inp("bias", b), al.out("y", (N, Cc // 8, oh, ow, 8), F16)
        ok(L.ssad_stem_pool_f16(p(z), p(bias), N, Cc, H, W, p(y), sp()))
        return dict(y=y)

    got = isolated(K, monkeypatch, fn)
    pooled = torch.nn.functional.max_pool2d(torch.from_numpy(Z), 3, 2, 1).numpy()
    assert same(got["y"], blk(np.maximum(pooled + b.reshape(1, -1, 1, 1), np.float32(0))))
    y = torch.empty((N, 2, oh, ow, 8), dtype=F16, device="cuda")
    tz, tb = dev(Z), dev(b)
    refused(K, lambda: K._check(L.ssad_stem_pool_f16(p(tz), p(tb), N, Cc + 4, H, W, p(y), sp()), "stem_pool_f16"))


# ---------------------------------------------------------------------------------------------------------------------
# Part B: one fp16 NaN / +Inf in a blocked operand.  N = 3, unit-scale data, no ReLU (it would turn -Inf into a finite
# 0 in kernel and reference alike).  No filter value rounds to fp16 zero (asserted), so the float64 reference on the
# planted operand is non-finite on the whole definitional set -- asserted per case -- and no output is excluded from
# the comparison other than that set.
# ---------------------------------------------------------------------------------------------------------------------

VALUES = [("nan", np.float32(np.nan)), ("inf", np.float32(np.inf))]


def quiet(f, *a):
    with np.errstate(all="ignore"):
        return f(*a)


def neighbourhood(shape, at, channels=slice(None)):
    """the 3 x 3 neighbourhood of pixel at[2:] in image at[0], the given output channels"""
    s = np.zeros(shape, bool)
    s[at[0], channels, max(at[2] - 1, 0):at[2] + 2, max(at[3] - 1, 0):at[3] + 2] = True
    return s


def check_set(got, expected, ref_clean, tol, what, where=None):
    """non-finite exactly on `expected`; every other element (of `where`) within tol of the clean reference's scale"""
    got = np.asarray(got, np.float64)
    nf = ~np.isfinite(got)
    assert not (expected & ~nf).any(), "%s: %d outputs the planted value must reach are finite" % (what, int((expected & ~nf).sum()))
    leak = nf & ~expected
    assert not leak.any(), "%s: %d non-finite outputs outside the definitional set, the first at %s" % (
        what, int(leak.sum()), tuple(int(v[0]) for v in np.nonzero(leak)))
    keep = ~nf if where is None else ~nf & where
    err = np.abs(got[keep] - ref_clean[keep])
    assert err.size and float(err.max()) <= tol * float(np.abs(ref_clean).max()), "%s: %.3e of the scale" % (
        what, float(err.max()) / float(np.abs(ref_clean).max()))


def nonzero16(*arrays):
    for a in arrays:
        assert np.all(a.astype(np.float16) != 0), "an operand value rounds to fp16 zero"


def pack_dev(K, Wt, dgrad=False, taps=9):
    L = K.lib()
    M, Cc = Wt.shape[:2]
    out = torch.zeros((L.ssad_f16_filter_halves if taps == 9 else L.ssad_pw_f16_filter_halves)(M, Cc), dtype=F16, device="cuda")
    fn = L.ssad_f16_pack_filter if taps == 9 else L.ssad_pw_f16_pack_filter
    ok(fn(p(dev(Wt)), M, Cc, p(None if dgrad else out), p(out if dgrad else None), sp()))
    return out


@pytest.mark.parametrize("Cc,M", [(37, 40), (40, 37)], ids=["37to40", "40to37"])
def test_nonfinite_locality_conv3x3_f16(K, Cc, M):
    """forward (blocked for M = 40, NCHW fp32 for M = 37): the 3 x 3 neighbourhood of that image, every output channel;
    M = 40 also the masked data-gradient form: an output whose mask is <= 0 is exactly 0 even if its value is NaN"""
    N, H, W = 3, 7, 9
    rng = np.random.default_rng(2000 + Cc)
    X0, Wt = randn(rng, N, Cc, H, W), randn(rng, M, Cc, 3, 3, scale=(9 * Cc) ** -0.5)
    Wg, mask = randn(rng, Cc, M, 3, 3, scale=(9 * Cc) ** -0.5), np.maximum(randn(rng, N, M, H, W), 0)
    nonzero16(Wt, Wg, X0)
    nchw = M % 8 != 0
    pf = pack_dev(K, Wt)
    tol = F32_TOL if nchw else BLOCKED_TOL

    def run(x):
        y = K.conv3x3_forward_f16(dev(blk(x)), pf, None, Cc, M, out_nchw_f32=nchw).cpu().numpy()
        return y if nchw else unblk(y, M)

    ref = lambda x, w: quiet(_conv64, _r16(x), _r16(w), None)
    ref_clean = ref(X0, Wt)
    bar(run(X0), ref_clean, tol, "clean run")
    if not nchw:
        pd, m16, tm = pack_dev(K, Wg, dgrad=True), mask.astype(np.float16), dev(blk(mask))
        run_dx = lambda x: unblk(K.conv3x3_forward_f16(dev(blk(x)), pd, None, Cc, M, mask_by=tm).cpu().numpy(), M)
        dx_clean = np.where(m16 > 0, ref(X0, flipped(Wg)), 0)
    for at in plants(X0.shape):
        want = neighbourhood((N, M, H, W), at)
        for vname, v in VALUES:
            x = X0.copy()
            x[at] = v
            what = "%s at %s" % (vname, at)
            assert np.array_equal(~np.isfinite(ref(x, Wt)), want)
            check_set(run(x), want, ref_clean, tol, what)
            if not nchw:
                dx = run_dx(x)
                assert np.array_equal(~np.isfinite(ref(x, flipped(Wg))), want)
                assert (want & (m16 <= 0)).any() and np.all(dx[m16 <= 0] == 0), what + ": masked outputs are not exactly 0"
                check_set(dx, want & (m16 > 0), dx_clean, tol, what + ", masked data gradient")


def test_nonfinite_locality_conv3x3_f16_across_levels(K):
    """two levels in one launch, the value in level 0: level 1 keeps its bits"""
    Cc, M = 37, 40
    rng = np.random.default_rng(2100)
    Wt, X0, X1 = randn(rng, M, Cc, 3, 3, scale=(9 * Cc) ** -0.5), randn(rng, 3, Cc, 7, 9), randn(rng, 3, Cc, 2, 3)
    nonzero16(Wt, X0)
    pf = pack_dev(K, Wt)

    def run(a, b):
        outs = [torch.empty((3, M // 8) + t.shape[2:] + (8,), dtype=F16, device="cuda") for t in (a, b)]
        K.conv3x3_forward_f16_levels([dev(blk(a)), dev(blk(b))], pf, None, Cc, M, outs)
        return [unblk(o.cpu().numpy(), M) for o in outs]

    c0, c1 = run(X0, X1)
    ref0 = _conv64(_r16(X0), _r16(Wt), None)
    at = plants(X0.shape)[0]
    for vname, v in VALUES:
        x = X0.copy()
        x[at] = v
        g0, g1 = run(x, X1)
        check_set(g0, neighbourhood(g0.shape, at), ref0, BLOCKED_TOL, "level 0, %s" % vname)
        assert same(g1, c1), "level 1 changed its bits with a %s in level 0" % vname


@pytest.mark.parametrize("stride", [1, 2])
def test_nonfinite_locality_conv1x1_f16(K, stride):
    """pointwise 37 -> 40: that output pixel; with stride 2 nothing when the pixel is not sampled (the interior plant at
    (3, 4)), and then the bits of the clean run"""
    N, Cc, M, H, W = 3, 37, 40, 7, 9
    rng = np.random.default_rng(2200 + stride)
    X0, Wt = randn(rng, N, Cc, H, W), randn(rng, M, Cc, scale=Cc ** -0.5)
    nonzero16(Wt, X0)
    pf = pack_dev(K, Wt, taps=1)
    oh, ow = (H - 1) // stride + 1, (W - 1) // stride + 1

    def run(x):
        y = torch.empty((N, M // 8, oh, ow, 8), dtype=F16, device="cuda")
        ok(pw(K, dev(blk(x)), pf, y, Cc, M, stride=stride))
        return unblk(y.cpu().numpy(), M)

    ref = lambda x: quiet(pw64, x[:, :, ::stride, ::stride], Wt)
    clean, ref_clean = run(X0), ref(X0)
    close_bb(clean, ref_clean, "clean run")
    sampled = 0
    for at in plants(X0.shape):
        want = np.zeros((N, M, oh, ow), bool)
        if at[2] % stride == 0 and at[3] % stride == 0:
            want[at[0], :, at[2] // stride, at[3] // stride] = True
            sampled += 1
        for vname, v in VALUES:
            x = X0.copy()
            x[at] = v
            assert np.array_equal(~np.isfinite(ref(x)), want)
            got = run(x)
            check_set(got, want, ref_clean, 1.5e-3, "%s at %s" % (vname, at))
            if not want.any():
                assert same(got, clean)
    assert sampled == (3 if stride == 1 else 2)


@pytest.mark.parametrize("cg", [4, 8, 32])
def test_nonfinite_locality_grouped_f16(K, cg):
    """C = 64: only the channels of the planted channel's group.  Groups of 4 and 8 share one 16-channel MFMA operand
    (block-diagonal filter, zeros across groups): a tile with a non-finite accumulator is recomputed once per group
    with the other groups' channels read as zeros -- multiplied by the zeros of the filter instead, a NaN in channel 63
    reached the 3 x 3 neighbourhood in channels 48..59 as well (108 outputs, measured before that change)."""
    L = K.lib()
    N, Cc, H, W = 3, 64, 7, 9
    G = Cc // cg
    rng = np.random.default_rng(2300 + cg)
    X0, Wt = randn(rng, N, Cc, H, W), randn(rng, Cc, cg, 3, 3, scale=(9 * cg) ** -0.5)
    nonzero16(Wt, X0)
    pf = torch.zeros(L.ssad_grouped_conv3x3_f16_filter_halves(Cc, G), dtype=F16, device="cuda")
    ok(L.ssad_grouped_conv3x3_f16_pack_filter(p(dev(Wt)), Cc, G, p(pf), sp()))

    def run(x):
        xb, y = dev(blk(x)), torch.empty((N, Cc // 8, H, W, 8), dtype=F16, device="cuda")
        ok(L.ssad_grouped_conv3x3_f16(p(xb), p(pf), p(None), N, Cc, H, W, G, 0, p(y), sp()))
        return unblk(y.cpu().numpy(), Cc)

    ref_clean = grouped64(X0, Wt, None, cg)
    close_bb(run(X0), ref_clean, "clean run")
    for at in plants(X0.shape):
        g = at[1] // cg
        want = neighbourhood((N, Cc, H, W), at, slice(g * cg, (g + 1) * cg))
        for vname, v in VALUES:
            x = X0.copy()
            x[at] = v
            assert np.array_equal(~np.isfinite(quiet(grouped64, x, Wt, None, cg)), want)
            check_set(run(x), want, ref_clean, 1.5e-3, "%s at %s" % (vname, at))


@pytest.mark.parametrize("taps,Cc,M", [(9, 37, 40), (9, 40, 37), (1, 37, 40)], ids=["3x3_37to40", "3x3_40to37", "1x1_37to40"])
def test_nonfinite_locality_filter_gradients_f16(K, taps, Cc, M):
    """planted in dY at channel m0: only row m0 of dW (and db[m0]); planted in X at channel c0: only column c0, db not
    at all.  Required non-finite: every tap whose partner pixel lies inside the image; the zero padding may add the
    other taps of that row / column (0 x NaN), nothing else."""
    L = K.lib()
    N, H, W = 3, 7, 9
    rng = np.random.default_rng(2400 + Cc + taps)
    X0, dY0 = randn(rng, N, Cc, H, W), randn(rng, N, M, H, W)
    nonzero16(X0, dY0)
    nb = (L.ssad_conv3x3_wgrad_f16_workspace_bytes if taps == 9 else L.ssad_conv1x1_wgrad_f16_workspace_bytes)(N, Cc, H, W, M)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")

    def run(x, dy):
        xb, dyb = dev(blk(x)), dev(blk(dy))
        dw, db = torch.empty((M, Cc, 3, 3) if taps == 9 else (M, Cc), device="cuda"), torch.empty((M,), device="cuda")
        if taps == 9:
            ok(L.ssad_conv3x3_wgrad_f16(p(xb), p(dyb), N, Cc, H, W, M, 0, 1.0, p(dw), p(db), p(ws), nb, sp()))
        else:
            ok(L.ssad_conv1x1_wgrad_f16(p(xb), p(dyb), N, Cc, H, W, M, 0, 1.0, p(None), p(dw), p(db), p(ws), nb, sp()))
        return dw.cpu().numpy().reshape(M, Cc, -1), db.cpu().numpy()

    rW, rb = wgrad64(X0, dY0, taps=3 if taps == 9 else 1).reshape(M, Cc, -1), _r16(dY0).sum((0, 2, 3))
    cW, cb = run(X0, dY0)
    bar(cW, rW, F32_TOL, "clean dW")
    bar(cb, rb, F32_TOL, "clean db")
    for which, base in (("dY", dY0), ("X", X0)):
        for at in plants(base.shape):
            required, allowed = np.zeros(rW.shape, bool), np.zeros(rW.shape, bool)
            sel = (at[1],) if which == "dY" else (slice(None), at[1])
            allowed[sel] = True
            for t in range(taps):
                oy, ox = (t // 3 - 1, t % 3 - 1) if taps == 9 else (0, 0)
                py, px = (at[2] + oy, at[3] + ox) if which == "dY" else (at[2] - oy, at[3] - ox)      # the partner pixel
                if 0 <= py < H and 0 <= px < W:
                    required[sel + (t,)] = True
            for vname, v in VALUES:
                t_ = base.copy()
                t_[at] = v
                gW, gb = run(*((X0, t_) if which == "dY" else (t_, dY0)))
                what = "%s in %s at %s" % (vname, which, at)
                nf = ~np.isfinite(gW)
                assert not (required & ~nf).any(), what + ": dW elements the value must reach are finite"
                leak = nf & ~allowed
                assert not leak.any(), "%s: %d non-finite dW elements outside %s, the first at %s" % (
                    what, int(leak.sum()), "row m0" if which == "dY" else "column c0", tuple(int(i[0]) for i in np.nonzero(leak)))
                check_set(gW, nf, rW, F32_TOL, what + ", dW")        # row m0 / column c0 too, wherever they came out finite
                want_b = np.zeros(M, bool)
                if which == "dY":
                    want_b[at[1]] = True
                check_set(gb, want_b, rb, F32_TOL, what + ", db")


def test_nonfinite_locality_f16_elementwise_subsample_pool(K):
    """the elements that read the planted one: sum, upsample-grad (the 2 x 2 block's output), subsample at stride 2 on
    the odd map (nothing when the pixel is not sampled), relu-grad with the value in the gradient (selected by a > 0),
    the stem pool's 3 x 3 / 2 windows (+Inf; a NaN, which fmaxf drops, may reach those windows only)"""
    L = K.lib()
    N, Cc, H, W = 3, 37, 7, 9
    CB = (Cc + 7) // 8
    rng = np.random.default_rng(2500)
    A, B, big = randn(rng, N, Cc, H, W), randn(rng, N, Cc, H, W), randn(rng, N, Cc, 2 * H, 2 * W)

    def ew(mode, a, b, h, w, stride=1):
        y = torch.empty((N, CB, h, w, 8), dtype=F16, device="cuda")
        ta, tb = dev(blk(a)), dev(blk(b)) if b is not None else None          # (kept alive: the launcher only sees addresses)
        ok(L.ssad_f16_elementwise(mode, p(ta), p(tb), p(y), N, Cc, h, w, stride, 0, sp()))
        return unblk(y.cpu().numpy(), Cc)

    def sub(a):
        y = torch.empty((N, CB, 4, 5, 8), dtype=F16, device="cuda")
        ok(L.ssad_f16_subsample(p(dev(blk(a))), N, Cc, H, W, 2, p(y), sp()))
        return unblk(y.cpu().numpy(), Cc)

    once = lambda a64: quiet(lambda t: t.astype(np.float16), a64)
    a16, b16 = A.astype(np.float16), B.astype(np.float16)
    for at in plants(A.shape):
        for vname, v in VALUES:
            x = A.copy()
            x[at] = v
            x16 = x.astype(np.float16)
            for name, got, want in (("sum", ew(K.EW_SUM2, x, B, H, W), once(x16.astype(np.float64) + b16)),
                                    ("subsample", sub(x), x16[:, :, ::2, ::2]),
                                    ("relu grad", ew(K.EW_RELU_GRAD, B, x, H, W), np.where(b16 > 0, x16, np.float16(0)))):
                assert np.array_equal(np.isnan(got), np.isnan(want)) and same(got[~np.isnan(want)], want[~np.isnan(want)]), \
                    "%s, %s at %s" % (name, vname, at)
    for at in plants(big.shape):
        for vname, v in VALUES:
            x = big.copy()
            x[at] = v
            want = once(quiet(lambda t: t.reshape(N, Cc, H, 2, W, 2).sum(axis=(3, 5)), x.astype(np.float16).astype(np.float64)))
            got = ew(K.EW_UPSAMPLE_GRAD, x, None, H, W)
            assert int((~np.isfinite(want)).sum()) == 1
            assert np.array_equal(np.isnan(got), np.isnan(want)) and same(got[~np.isnan(want)], want[~np.isnan(want)]), \
                "upsample grad, %s at %s" % (vname, at)
    Z, b = randn(rng, N, 16, H, W), randn(rng, 16)
    pool = lambda z: torch.nn.functional.max_pool2d(torch.from_numpy(z), 3, 2, 1).numpy() + b.reshape(1, -1, 1, 1)

    def run_pool(z):
        y, tz, tb = torch.empty((N, 2, 4, 5, 8), dtype=F16, device="cuda"), dev(z), dev(b)
        ok(L.ssad_stem_pool_f16(p(tz), p(tb), N, 16, H, W, p(y), sp()))
        return unblk(y.cpu().numpy(), 16)

    clean = run_pool(Z)
    for at in plants(Z.shape):
        z = Z.copy()
        z[at] = np.inf
        want = blk(np.maximum(pool(z), np.float32(0)))
        got = run_pool(z)
        assert same(blk(got), want) and np.isinf(got).sum() == np.isinf(unblk(want, 16)).sum() > 0, "pool, inf at %s" % (at,)
        z[at] = np.nan
        got = run_pool(z)
        windows = np.isinf(unblk(want, 16))
        assert same(got[~windows], clean[~windows]), "pool, nan at %s: an output outside the windows changed" % (at,)
