"""The default engine behind Conv, ConvGradient and MaxPool (ops/conv_op.cc RunDefaultEngine, kernels/im2col.hip,
kernels/gemm_general.hip) on every geometry ParseConvGeometryFrom accepts: dilation, rectangular kernels, asymmetric
pads, unequal strides, the boundaries between the seven routes of conv_op.cc, groups, the operator forms and the three
argument spellings -- against the float64 definitions of tests/default_engine_ref.py at the project's CONV_RTOL /
CONV_FLOOR; the launchers ssad_im2col / ssad_im2col_batched / ssad_col2im directly (pure copies: bit equality);
MaxPool / MaxPoolGradient with ties (every input equal to its window's maximum receives the gradient); and the
non-finite locality of the im2col route (the padding is a select, a zero-filled GEMM tile tail never reaches a
stored element).

Each case's id names the route of conv_op.cc it takes, forward/gradient, as read from the code (the legend is at
default_engine_ref.CONV_CASES)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ssad_amd  # noqa: E402,F401
from ssad_amd.caffe2_hip import core, dyndep, workspace  # noqa: E402
import default_engine_ref as R  # noqa: E402
import default_engine_ops as D  # noqa: E402
from default_engine_ops import GPU, check, feed, geo_args, reference, run_conv  # noqa: E402
from test_gpu_kernels import CONV_FLOOR, CONV_RTOL, DX_FLOOR, DX_RTOL, close  # noqa: E402
from test_gpu_isolation import bits, plants, within_bar  # noqa: E402

pytestmark = pytest.mark.gpu

CASE_IDS = ["%s[%s]" % (c["name"], c["route"]) for c in R.CONV_CASES]


@pytest.fixture(autouse=True)
def fresh_workspace():
    assert torch.cuda.is_available()
    dyndep.InitOpsLibrary()
    workspace.ResetWorkspace()
    yield
    workspace.ResetWorkspace()


@pytest.fixture(scope="module")
def K():
    from ssad_amd import kernels
    kernels.lib()  # raises if the HIP extension is missing: no fallback
    return kernels


@functools.lru_cache(maxsize=None)
def problem(name):
    """(inputs, float64 reference) of a case, computed once and shared; callers do not write into either"""
    case = R.CONV_CASE[name]
    ins = R.conv_inputs(case)
    return ins, reference(case["geo"], *ins)


# ---------------------------------------------------------------------------------------------------------------------
# Conv / ConvGradient: the geometry sweep
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.CONV_CASES, ids=CASE_IDS)
def test_conv_and_gradient_geometry(case):
    """Y, dW, db and dX of one geometry through CreateOperator / RunOperatorOnce / GradientRegistry."""
    (X, Wt, b, dY), ref = problem(case["name"])
    got = run_conv(case["geo"], X, Wt, b, dY)
    assert set(got) == {"Y", "dW", "db", "dX"}
    check(got, ref, case["name"])


FORMS = [("dil2_k3p2", "im2col"), ("K27_k3s2", "igemm_fwd_im2col_grad"), ("k2s2", "igemm_kxk"), ("pw_P108", "pw-gemm_loop")]


@pytest.mark.parametrize("name,route", FORMS, ids=["%s[%s]" % f for f in FORMS])
def test_conv_operator_forms_no_bias_and_no_data_gradient(name, route):
    """no_bias = 1 (ConvGradient with [dW, dX] and with [dW] alone) and a bias without the dX output ([dW, db]).
    Without dX the K % 4 rule of the batched gradient (dx_ok) does not apply: K27_k3s2 then takes the kxk route."""
    (X, Wt, b, dY), ref = problem(name)
    g = R.CONV_CASE[name]["geo"]
    ref_nb = dict(ref, Y=R.conv2d_f64(X, Wt, None, g))
    got = run_conv(g, X, Wt, None, dY)
    assert set(got) == {"Y", "dW", "dX"}
    check(got, ref_nb, name + " no_bias")
    got = run_conv(g, X, Wt, None, dY, want_dx=False)
    assert set(got) == {"Y", "dW"}
    check(got, ref_nb, name + " no_bias, no dX")
    got = run_conv(g, X, Wt, b, dY, want_dx=False)
    assert set(got) == {"Y", "dW", "db"}
    check(got, ref, name + " no dX")
    # three gradient outputs under no_bias are refused at construction (conv_gradient_op.cc)
    with core.DeviceScope(GPU):
        bad = core.CreateOperator("ConvGradient", ["X", "w", "Y_grad"], ["w_grad", "b_grad", "X_grad"], no_bias=1,
                                  **geo_args(g))
    with pytest.raises(Exception, match="you should not have 3 grad output"):
        workspace.RunOperatorOnce(bad)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("name,route", [("dil2_k3p2", "im2col"), ("K27_k3s2", "igemm")],
                         ids=["dil2_k3p2[im2col]", "K27_k3s2[igemm]"])
def test_conv_fuse_relu(name, route, bias):
    """fuse_relu = 1: Y = max(conv (+ b), 0).  On the im2col route without a bias it is ssad_affine_channel with
    neither scale nor bias; on the implicit GEMM it is the epilogue's flag.  The gradient definition does not carry
    the argument."""
    (X, Wt, b, dY), ref = problem(name)
    g = R.CONV_CASE[name]["geo"]
    Y64 = R.conv2d_f64(X, Wt, b if bias else None, g)
    got = run_conv(g, X, Wt, b if bias else None, dY, fuse_relu=True)
    close(got["Y"], np.maximum(Y64, 0), CONV_RTOL, CONV_FLOOR, name + " relu(Y)")
    assert (got["Y"] >= 0).all() and (got["Y"] == 0).any() and (got["Y"] > 0).any()
    check({k: got[k] for k in ("dW", "dX")}, ref, name + " gradient of a fuse_relu Conv")


def test_conv_argument_spellings_are_bit_identical():
    """kernel | kernel_h + kernel_w | kernels (likewise stride, pad, dilation) of one dilated, strided geometry: the
    same ConvGeometry, so the same launches."""
    name = "dil2_s2"
    (X, Wt, b, dY), ref = problem(name)
    g = R.CONV_CASE[name]["geo"]
    runs = {sp: run_conv(g, X, Wt, b, dY, spelling=sp) for sp in D.SPELLINGS}
    check(runs["single"], ref, name)
    for sp in ("hw", "list"):
        for key in ("Y", "dW", "db", "dX"):
            assert np.array_equal(bits(runs[sp][key]), bits(runs["single"][key])), (sp, key)


def test_dilated_conv_relu_through_a_net_equals_operator_by_operator():
    """Conv (3x3, dilation 2, pad 2) + in-place Relu and their gradients through CreateNet / RunNet against the same
    definitions run one by one.  The lowering fuses Conv + Relu and ConvGradient + ReluGradient only for the 3x3 engines'
    geometry (net_lowering.cc IsFusedPathConv -> IsSubnetGeometry), so a dilated pair stays four operators on the
    default engine: the same launches, hence bit equality."""
    name = "dil2_k3p2"
    (X, Wt, b, dY), _ = problem(name)
    g = R.CONV_CASE[name]["geo"]
    net = core.Net("dilated_conv_relu")
    with core.DeviceScope(GPU):
        net.Conv(["X", "w", "b"], ["Y"], order="NCHW", **geo_args(g))
        net.Relu(["Y"], ["Y"])
        gmap = net.AddGradientOperators({"Y": "Y_grad"})
    names = ["Y", gmap["w"], gmap["b"], gmap["X"]]

    def feed_all():
        workspace.ResetWorkspace()
        feed("X", X); feed("w", Wt); feed("b", b); feed("Y_grad", dY)

    feed_all()
    workspace.CreateNet(net)
    lowered = [o.type for o in workspace.LoweredOps(net)]
    assert sorted(lowered) == ["Conv", "ConvGradient", "Relu", "ReluGradient"], lowered
    workspace.RunNet(net)
    through_net = {n: workspace.FetchBlob(n) for n in names}
    feed_all()
    workspace.RunOperatorsOnce(list(net.Proto().op))
    for n in names:
        assert np.array_equal(bits(through_net[n]), bits(workspace.FetchBlob(n))), n
    Y64 = np.maximum(R.conv2d_f64(X, Wt, b, g), 0)
    close(through_net["Y"], Y64, CONV_RTOL, CONV_FLOOR, "relu(Y)")
    dpre = np.where(through_net["Y"] > 0, dY, 0).astype(np.float32)
    dW, db, dX = R.conv2d_grads_f64(X, Wt, dpre, g)
    close(through_net[gmap["w"]], dW, CONV_RTOL, CONV_FLOOR, "dW")
    close(through_net[gmap["b"]], db, CONV_RTOL, CONV_FLOOR, "db")
    close(through_net[gmap["X"]], dX, CONV_RTOL, CONV_FLOOR, "dX")


REFUSALS = [
    ("kernel_larger_than_padded_input", "Conv", dict(kernel=5, dilation=3, pad=1), "does not fit the padded input"),
    ("no_kernel_argument", "Conv", dict(stride=1, pad=1), "kernel size"),
    ("legacy_pad_1", "Conv", dict(kernel=3, pad=1, legacy_pad=1), "legacy padding"),
    ("legacy_pad_2", "Conv", dict(kernel=3, pad=1, legacy_pad=2), "legacy padding"),
    ("pads_of_the_wrong_length", "Conv", dict(kernels=[3, 3], pads=[1, 1, 1]), r"pads\.size\(\)"),
    ("order_NHWC", "Conv", dict(kernel=3, pad=1, order="NHWC"), "Cannot create operator|HIP Conv engine"),
    ("max_pool_dilation_2", "MaxPool", dict(kernel=3, pad=1, dilation=2), "Cannot create operator|HIP MaxPool implements"),
]


@pytest.mark.parametrize("what,op_type,args,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_by_message(what, op_type, args, message):
    feed("X", np.zeros((1, 4, 9, 11), np.float32))
    k = args.get("kernel", 3)
    feed("w", np.zeros((6, 4, k, k), np.float32))
    with core.DeviceScope(GPU):
        op = core.CreateOperator(op_type, ["X", "w"] if op_type == "Conv" else ["X"], ["Y"], **args)
    with pytest.raises(Exception, match=message):
        workspace.RunOperatorOnce(op)


def test_conv1x1_engine_blas_switch():
    """SSAD_CONV1X1_ENGINE=blas (README: switches) is read once per process (conv_op.cc BlasRouteForced): one fresh
    child process runs the pointwise, strided pointwise, 7x7/2, 3x3/2 and 5x5 layers, which the switch moves from the
    pointwise / implicit GEMM kernels to im2col + the general GEMM, and checks each against the float64 reference at
    CONV_RTOL / CONV_FLOOR.  It exits non-zero with the failing case's name."""
    env = dict(os.environ, SSAD_CONV1X1_ENGINE="blas")
    r = subprocess.run([sys.executable, os.path.abspath(D.__file__)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and ("ok %d" % len(D.BLAS_CASES)) in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------------------------
# MaxPool / MaxPoolGradient
# ---------------------------------------------------------------------------------------------------------------------

def run_pool(g, X, dY):
    workspace.ResetWorkspace()
    feed("X", X)
    with core.DeviceScope(GPU):
        op = core.CreateOperator("MaxPool", ["X"], ["Y"], **geo_args(g, pool=True))
    workspace.RunOperatorOnce(op)
    Y = workspace.FetchBlob("Y")
    feed("Y_grad", dY)
    gops, gin = core.GradientRegistry.GetGradientForOp(op, ["Y_grad"])
    workspace.RunOperatorsOnce(gops)
    return Y, workspace.FetchBlob(gin[0])


@pytest.mark.parametrize("case", R.POOL_CASES, ids=lambda c: c["name"])
def test_max_pool_geometries_tie_free(case):
    """forward bit-equal to the definition; gradient at the existing test's bar (rtol = atol = 1e-6)"""
    g = case["geo"]
    rng = np.random.default_rng(43)
    X = rng.standard_normal((2, 3) + case["hw"]).astype(np.float32)
    Yd = R.max_pool(X, g)
    dY = rng.standard_normal(Yd.shape).astype(np.float32)
    Y, dX = run_pool(g, X, dY)
    assert np.array_equal(bits(Y), bits(Yd))
    want = R.max_pool_grad(X.astype(np.float64), Yd.astype(np.float64), dY.astype(np.float64), g)
    np.testing.assert_allclose(dX, want, rtol=1e-6, atol=1e-6)
    if case["name"] == "k2s3_gaps":               # pixels no window covers get exactly +0
        covered = R.max_pool_grad(np.ones_like(X), np.ones_like(Yd), np.ones_like(dY), g) > 0
        assert (~covered).any() and np.all(bits(dX[~covered]) == 0)


@pytest.mark.parametrize("case", R.POOL_CASES, ids=lambda c: c["name"])
def test_max_pool_gradient_reaches_every_tied_maximum(case):
    """X from {0, 1, 2}, dY small integers: every sum is exact, so bit equality with the definition ("every input equal
    to its window's maximum receives the gradient", pool_op.cu).  torch breaks ties differently and is no reference."""
    g = case["geo"]
    rng = np.random.default_rng(47)
    X = rng.integers(0, 3, (2, 3) + case["hw"]).astype(np.float32)
    Yd = R.max_pool(X, g)
    dY = rng.integers(-3, 4, Yd.shape).astype(np.float32)
    want = R.max_pool_grad(X, Yd, dY, g)
    ties = R.max_pool_grad(X, Yd, np.ones_like(dY), g).sum() - Yd.size
    assert ties > 0, "the data has no tie"
    Y, dX = run_pool(g, X, dY)
    assert np.array_equal(bits(Y), bits(Yd))
    assert np.array_equal(dX, want) and not np.signbit(dX[dX == 0]).any()


# ---------------------------------------------------------------------------------------------------------------------
# ssad_im2col / ssad_im2col_batched / ssad_col2im, directly (ctypes on K.lib(), like ssad_gemm_f32's test)
# ---------------------------------------------------------------------------------------------------------------------

def launchers(K):
    L = K.lib()
    geo = [C.c_int] * 13
    L.ssad_im2col.argtypes = [C.c_void_p] + geo + [C.c_void_p, C.c_void_p]
    L.ssad_col2im.argtypes = [C.c_void_p] + geo + [C.c_void_p, C.c_void_p]
    L.ssad_im2col_batched.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p, C.c_void_p]
    for f in (L.ssad_im2col, L.ssad_col2im, L.ssad_im2col_batched):
        f.restype = C.c_int
    return L


def geo_ints(Cc, H, W, g):
    (kh, kw), (sh, sw), (pt, pl, pb, pr), (dh, dw) = g["kernel"], g["stride"], g["pads"], g["dilation"]
    return [Cc, H, W, kh, kw, dh, dw, pt, pl, pb, pr, sh, sw]


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("case", R.CONV_CASES, ids=[c["name"] for c in R.CONV_CASES])
def test_im2col_and_col2im_launchers(K, case):
    """im2col is a pure copy: bit equality with the definition.  col2im against the float64 definition at DX_RTOL /
    DX_FLOOR, and on integer data (exact sums) bit for bit."""
    L = launchers(K)
    g, Cc, (H, W) = case["geo"], case["cin"], case["hw"]
    rng = np.random.default_rng(3)
    x = rng.standard_normal((Cc, H, W)).astype(np.float32)
    want = R.im2col(x, g)
    col = torch.full(want.shape, float("nan"), device="cuda")
    assert L.ssad_im2col(torch.from_numpy(x).cuda().data_ptr(), *geo_ints(Cc, H, W, g), col.data_ptr(), stream()) == 0
    assert np.array_equal(bits(col.cpu().numpy()), bits(want))
    for ints in (False, True):
        c = (rng.integers(-4, 5, want.shape) if ints else rng.standard_normal(want.shape)).astype(np.float32)
        back = torch.full((Cc, H, W), float("nan"), device="cuda")
        assert L.ssad_col2im(torch.from_numpy(c).cuda().data_ptr(), *geo_ints(Cc, H, W, g), back.data_ptr(),
                             stream()) == 0
        got = back.cpu().numpy()
        if ints:
            assert np.array_equal(got, R.col2im(c, Cc, H, W, g))
        else:
            close(got, R.col2im(c.astype(np.float64), Cc, H, W, g), DX_RTOL, DX_FLOOR, "col2im")


def batched_want(X, k, st, pad):
    g = R.geometry(k, st, pad)
    return np.stack([R.im2col(x, g) for x in X])


BATCHED = [
    # name, (N, C, H, W), kernel, stride, pad, byte offset of col from a 16-byte boundary
    ("rows_kernel_OW8", (2, 5, 9, 16), 3, 2, 1, 0),                  # OW = 8, aligned: im2col_rows_kernel
    ("fallback_OW_not_multiple_of_4", (2, 5, 9, 11), 3, 2, 1, 0),      # OW = 6
    ("fallback_col_4_bytes_off", (2, 5, 9, 16), 3, 2, 1, 4),
    ("fallback_N_rows_65592", (8, 911, 4, 4), 3, 1, 1, 0),           # N * C * k * k = 65592 >= 65536, 4 x 4 outputs
]


@pytest.mark.parametrize("name,shape,k,st,pad,off", BATCHED, ids=[b[0] for b in BATCHED])
def test_im2col_batched_paths_equal_the_definition_and_each_other(K, name, shape, k, st, pad, off):
    L = launchers(K)
    rng = np.random.default_rng(11)
    X = rng.standard_normal(shape).astype(np.float32)
    want = batched_want(X, k, st, pad)
    N, Cc, H, W = shape
    OW = R.out_size(W, k, 1, pad, pad, st)
    takes_rows_kernel = OW % 4 == 0 and off == 0 and N * Cc * k * k < 65536
    assert takes_rows_kernel == name.startswith("rows_kernel")
    x = torch.from_numpy(X).cuda()
    raw = torch.full((want.size + 8,), float("nan"), device="cuda")
    assert raw.data_ptr() % 16 == 0
    col = raw[off // 4: off // 4 + want.size]
    assert L.ssad_im2col_batched(x.data_ptr(), N, Cc, H, W, k, st, pad, col.data_ptr(), stream()) == 0
    got = col.cpu().numpy().reshape(want.shape)
    assert np.array_equal(bits(got), bits(want))
    assert torch.isnan(raw[:off // 4]).all() and torch.isnan(raw[off // 4 + want.size:]).all()
    # ... and the per-image launcher, image by image, gives the same bits
    one = torch.empty(want.shape[1:], device="cuda")
    g = R.geometry(k, st, pad)
    for n in range(0, N, max(1, N - 1)):
        assert L.ssad_im2col(x[n].data_ptr(), *geo_ints(Cc, H, W, g), one.data_ptr(), stream()) == 0
        assert np.array_equal(bits(one.cpu().numpy()), bits(got[n]))


def test_im2col_batched_rows_kernel_and_fallback_agree_bit_for_bit(K):
    """the same batch through the 16-byte row kernel and through the fallback (col 4 bytes off alignment)"""
    L = launchers(K)
    rng = np.random.default_rng(12)
    shape, k, st, pad = (3, 6, 10, 14), 3, 1, 0                          # OH = 8, OW = 12
    X = rng.standard_normal(shape).astype(np.float32)
    want = batched_want(X, k, st, pad)
    x = torch.from_numpy(X).cuda()
    outs = []
    for off in (0, 1):
        raw = torch.full((want.size + 4,), float("nan"), device="cuda")
        col = raw[off:off + want.size]
        assert L.ssad_im2col_batched(x.data_ptr(), *shape, k, st, pad, col.data_ptr(), stream()) == 0
        outs.append(col.cpu().numpy())
    assert np.array_equal(bits(outs[0]), bits(outs[1])) and np.array_equal(bits(outs[0]), bits(want.reshape(-1)))


def test_im2col_batched_of_no_image_returns_0_and_writes_nothing(K):
    L = launchers(K)
    x = torch.zeros((1, 5, 9, 16), device="cuda")
    col = torch.full((5 * 9 * 5 * 8,), float("nan"), device="cuda")
    assert L.ssad_im2col_batched(x.data_ptr(), 0, 5, 9, 16, 3, 2, 1, col.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(col).all()
    assert L.ssad_im2col_batched(x.data_ptr(), -1, 5, 9, 16, 3, 2, 1, col.data_ptr(), stream()) == -1
    assert L.ssad_im2col_batched(x.data_ptr(), 1, 5, 2, 2, 7, 1, 0, col.data_ptr(), stream()) == -1   # no output pixel


# ---------------------------------------------------------------------------------------------------------------------
# non-finite locality on the default engine: N = 3, the three planted positions of tests/test_gpu_isolation.py
# ---------------------------------------------------------------------------------------------------------------------

VALUES = [("nan", np.float32(np.nan)), ("inf", np.float32(np.inf))]
LOCALITY = ["dil2_k3p2", "asym_pads_k3s2", "g3_dil2"]


def three_images(name):
    case = dict(R.CONV_CASE[name], N=3)
    return case, R.conv_inputs(case, seed=1)


def check_exact_locality(got, ref_planted, ref_clean, what):
    """the non-finite outputs are exactly the definition's on the poisoned input; every other output is within the bar
    of the clean reference (where the definition stays finite it does not depend on the planted value)"""
    nf, nf_ref = ~np.isfinite(got), ~np.isfinite(ref_planted)
    assert nf_ref.any(), what + ": the planted value reaches nothing in the definition"
    missing, leak = nf_ref & ~nf, nf & ~nf_ref
    assert not missing.any(), "%s: %d outputs the planted value must reach are finite" % (what, int(missing.sum()))
    assert not leak.any(), "%s: %d non-finite outputs the definition does not connect, the first at %s" % (
        what, int(leak.sum()), tuple(int(v[0]) for v in np.nonzero(leak)))
    within_bar(got, ref_clean, ~nf, what)


@pytest.mark.parametrize("name", LOCALITY)
def test_nonfinite_locality_forward_of_a_value_in_x(name):
    """One NaN / +Inf in X reaches its own image, its own group and the windows that contain it (Y), and the filter-
    gradient columns (c, ki, kj) that read it (dW); nothing else."""
    case, (X, Wt, b, dY) = three_images(name)
    g = case["geo"]
    clean = reference(g, X, Wt, b, dY)
    for vname, v in VALUES:
        for at in plants(X.shape):
            Xp = X.copy()
            Xp[at] = v
            got = run_conv(g, Xp, Wt, b, dY)
            what = "%s %s in X at %s" % (name, vname, at)
            Yp = R.conv2d_f64(Xp, Wt, b, g)
            assert not (~np.isfinite(Yp))[np.arange(3) != at[0]].any()            # the definition itself is local
            check_exact_locality(got["Y"], Yp, clean["Y"], what + ": Y")
            if vname == "nan":
                dWp = R.conv2d_grads_f64(Xp, Wt, dY, g)[0]
                check_exact_locality(got["dW"], dWp, clean["dW"], what + ": dW")
                assert np.isfinite(got["dX"]).all() and np.isfinite(got["db"]).all()
                check({k: got[k] for k in ("dX", "db")}, clean, what)


@pytest.mark.parametrize("name", LOCALITY)
def test_nonfinite_locality_gradients_of_a_nan_in_dy(name):
    """One NaN in dY reaches row m0 of dW (its group's block), db[m0], and the pixels of its image and group whose
    windows contain the output pixel (dX); nothing else."""
    case, (X, Wt, b, dY) = three_images(name)
    g = case["geo"]
    clean = reference(g, X, Wt, b, dY)
    for at in plants(dY.shape):
        dYp = dY.copy()
        dYp[at] = np.nan
        got = run_conv(g, X, Wt, b, dYp)
        what = "%s nan in dY at %s" % (name, at)
        dWp, dbp, dXp = R.conv2d_grads_f64(X, Wt, dYp, g)
        assert np.isnan(dWp[at[1]]).all() and np.isnan(dWp).sum() == dWp[0].size and np.isnan(dbp).sum() == 1
        assert not np.isnan(dXp)[np.arange(3) != at[0]].any()
        check_exact_locality(got["dW"], dWp, clean["dW"], what + ": dW")
        check_exact_locality(got["db"], dbp, clean["db"], what + ": db")
        check_exact_locality(got["dX"], dXp, clean["dX"], what + ": dX")
        assert np.isfinite(got["Y"]).all()


def test_nonfinite_locality_max_pool():
    """A NaN in X never becomes a maximum (the definition's `>`; fmaxf in max_pool_kernel) and receives no gradient:
    Y equals the definition on the poisoned input bit for bit, so only the windows that contain the pixel can change."""
    g = R.geometry(3, 2, 1)
    rng = np.random.default_rng(53)
    X = rng.standard_normal((3, 3, 9, 11)).astype(np.float32)
    Yc = R.max_pool(X, g)
    dY = rng.integers(-3, 4, Yc.shape).astype(np.float32)
    for at in plants(X.shape):
        Xp = X.copy()
        Xp[at] = np.nan
        Yp = R.max_pool(Xp, g)
        Y, dX = run_pool(g, Xp, dY)
        assert np.array_equal(bits(Y), bits(Yp)) and np.isfinite(Y).all()
        differs = Y != Yc
        oh, ow = np.nonzero(differs[at[0], at[1]])
        assert differs.sum() == differs[at[0], at[1]].sum(), "another plane changed"
        assert all(abs(2 * r - at[2]) <= 1 and abs(2 * c - at[3]) <= 1 for r, c in zip(oh, ow))
        assert np.array_equal(dX, R.max_pool_grad(Xp, Yp, dY, g)) and dX[at] == 0
