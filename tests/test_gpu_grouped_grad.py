"""The grouped 3x3 convolution's two gradients on the GPU (csrc/kernels/grouped_conv3x3_grad.hip): against the CPU
oracle's dense conv_backward applied group by group, against the reference's own compiled ConvGradientOp, in the
guarded arena, with a planted NaN, twice for the same bits; then `hip_algo="grouped"` on Conv / ConvGradient against
torch and against the default engine, and one ResNeXt bottleneck built with BodyConfig(grouped_engine=True) as a net.

Every dx element of a 3x3 / pad 1 / stride 2 layer has a contributing tap (an even row takes the centre tap, an odd
row the bottom tap of the output row above it), so there is no map with zero-contribution elements to choose;
test_guarded_grouped_gradients computes the contribution count from the definition, asserts that, and checks every
word of dx written -- with the mask, which does write zeros."""
import os

import numpy as np
import pytest
import torch

import ssad_amd  # noqa: F401
from oracle import oracle
import make_golden as mg
from ssad_amd.caffe2_hip import caffe2_pb2, core, dyndep, workspace
from test_gpu_kernels import CONV_FLOOR, CONV_RTOL, close, dev
from test_gpu_x101_32x8d import NARROW_GEOMS, case

pytestmark = pytest.mark.gpu
GPU = core.DeviceOption(caffe2_pb2.CUDA, 0)
# (N, cg, G, H, W, stride): the eight narrow geometries and the 64-wide ones of test_gpu_x101_32x8d
WIDE_GEOMS = [(2, 64, 1, 9, 19, 1), (2, 64, 2, 11, 21, 2), (1, 64, 2, 16, 32, 2), (1, 64, 32, 5, 7, 1)]
GEOMS = NARROW_GEOMS + WIDE_GEOMS
GEOM_ID = lambda g: "N%d_cg%d_G%d_%dx%d_s%d" % tuple(g)     # noqa: E731


@pytest.fixture(scope="module")
def K():
    from ssad_amd import kernels
    kernels.lib()
    return kernels


def out_hw(H, W, s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def grad_case(geom, seed=None):
    """(X, Wt, dY) of one geometry: case() of test_gpu_x101_32x8d plus an output gradient from the same stream."""
    N, cg, G, H, W, s = geom
    seed = 1000 + sum(geom) if seed is None else seed
    X, Wt, _ = case(N, G, H, W, seed, cg)
    dY = np.random.default_rng(seed + 1).standard_normal((N, cg * G) + out_hw(H, W, s)).astype(np.float32)
    return X, Wt, dY


def grouped_backward_oracle(X, Wt, dY, group, stride):
    """(dW, dX): oracle.conv_backward on each group's contiguous channel block (conv_op_impl.h:451-500,524-560)."""
    cg = X.shape[1] // group
    dW, dX = np.empty_like(Wt), np.empty_like(X)
    for g in range(group):
        sl = slice(g * cg, (g + 1) * cg)
        dw, _, dx = oracle.conv_backward(np.ascontiguousarray(X[:, sl]), np.ascontiguousarray(Wt[sl]),
                                         np.ascontiguousarray(dY[:, sl]), kernel=3, stride=stride, pad=1, want_db=False)
        dW[sl], dX[:, sl] = dw, dx
    return dW, dX


_REF = {}


def dv(a):
    """a device copy of a shared (read-only) array"""
    return dev(np.array(a))


def reference(geom):
    """computed once per geometry, shared, never modified"""
    if geom not in _REF:
        X, Wt, dY = grad_case(geom)
        dW, dX = grouped_backward_oracle(X, Wt, dY, geom[2], geom[5])
        for a in (X, Wt, dY, dW, dX):
            a.setflags(write=False)
        _REF[geom] = (X, Wt, dY, dW, dX)
    return _REF[geom]


def wgrad_partials(K, geom):
    """SPLIT of include/ssad_kernels.h, from the documented formula: min(T, max(1, 1024 / B)) with T the pixel tiles
    (8 x 16 outputs at stride 1, 4 x 16 at stride 2) and B the workgroups per range; checked against the function."""
    N, cg, G, H, W, s = geom
    oh, ow = out_hw(H, W, s)
    tr = 8 if s == 1 else 4
    T = N * ((oh + tr - 1) // tr) * ((ow + 15) // 16)
    gpw = {4: 4, 8: 4, 16: 2, 32: 1, 64: 1}[cg]
    B = (G + gpw - 1) // gpw * (4 if cg == 64 else 1)
    split = min(T, max(1, 1024 // B))
    assert K.lib().ssad_grouped_conv3x3_wgrad_workspace_bytes(N, cg * G, H, W, G, s) == split * cg * G * cg * 9 * 4
    return split


# ---- 1. against the oracle -------------------------------------------------------------------------------------------

def test_oracle_per_group_agrees_with_float64_torch_autograd():
    """the oracle of this file, once, on the CPU: torch's grouped conv2d in float64"""
    geom = (2, 8, 4, 9, 17, 2)
    X, Wt, dY, dW, dX = reference(geom)
    xt, wt = torch.tensor(X.astype(np.float64), requires_grad=True), torch.tensor(Wt.astype(np.float64), requires_grad=True)
    torch.nn.functional.conv2d(xt, wt, None, geom[5], 1, 1, geom[2]).backward(torch.tensor(dY.astype(np.float64)))
    close(dW, wt.grad.numpy(), CONV_RTOL, CONV_FLOOR, "oracle dW")
    close(dX, xt.grad.numpy(), CONV_RTOL, CONV_FLOOR, "oracle dX")


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_ID)
def test_both_gradients_vs_oracle(K, geom):
    N, cg, G, H, W, s = geom
    X, Wt, dY, dW, dX = reference(geom)
    tdy, tw, tx = dv(dY), dv(Wt), dv(X)
    got = K.grouped_conv3x3_dgrad(tdy, tw, G, s, (H, W))
    assert tuple(got.shape) == X.shape
    close(got.cpu().numpy(), dX, CONV_RTOL, CONV_FLOOR, "dX")
    # the mask operand: the ReluGradient of the in-place ReLU that produced the layer's input
    got = K.grouped_conv3x3_dgrad(tdy, tw, G, s, (H, W), relu_x=tx)
    masked = np.where(X > 0, dX, np.float32(0))
    close(got.cpu().numpy(), masked, CONV_RTOL, CONV_FLOOR, "masked dX")
    assert np.all(got.cpu().numpy()[X <= 0] == 0)
    got = K.grouped_conv3x3_wgrad(tx, tdy, G, s)
    assert tuple(got.shape) == Wt.shape
    close(got.cpu().numpy(), dW, CONV_RTOL, CONV_FLOOR, "dW")


def test_every_width_has_a_case_with_several_partials(K):
    """the filter-gradient cases above that cross the kernel's own split of the pixel range, per width"""
    crossing = {}
    for geom in GEOMS:
        crossing.setdefault(geom[1], []).append(wgrad_partials(K, geom))
    assert sorted(crossing) == [4, 8, 16, 32, 64]
    for cg, splits in crossing.items():
        assert max(splits) > 1, (cg, splits)


# ---- 2. against the reference's compiled operator --------------------------------------------------------------------

def test_vs_reference_operator_golden(K, golden_dir):
    """tests/golden/grouped_grad_ref.npz (make_grouped_grad_golden.py): ConvGradientOp<float, CPUContext> with group"""
    g = np.load(os.path.join(golden_dir, "grouped_grad_ref.npz"))
    names = sorted(k[:-5] for k in g.files if k.endswith("_dims"))
    assert len(names) >= 3
    seen = set()
    for name in names:
        seed, N, Cin, M, H, W, k, s, p, grp = [int(v) for v in g[name + "_dims"]]
        assert (k, p) == (3, 1) and Cin == M
        seen.add((Cin // grp, s))
        X, Wt, _, dY = mg.conv_ref_inputs(seed, N, Cin, M, H, W, k, s, p, grp)
        dx = K.grouped_conv3x3_dgrad(dev(dY), dev(Wt), grp, s, (H, W)).cpu().numpy()
        dw = K.grouped_conv3x3_wgrad(dev(X), dev(dY), grp, s).cpu().numpy()
        close(dx.ravel()[g[name + "_dX_idx"]], g[name + "_dX"], CONV_RTOL, CONV_FLOOR, name + " dX")
        close(dw.ravel()[g[name + "_dW_idx"]], g[name + "_dW"], CONV_RTOL, CONV_FLOOR, name + " dW")
    assert {(4, 2), (16, 1), (64, 1)} <= seen


# ---- 3. isolation ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", [(2, 8, 3, 9, 18, 2), (2, 64, 2, 7, 21, 2), (3, 16, 3, 7, 9, 1), (1, 64, 1, 9, 17, 1)],
                         ids=GEOM_ID)
def test_guarded_grouped_gradients(K, monkeypatch, geom):
    """Guard bands intact, x / w / dy unchanged, dx, dw and both packs written completely, the workspace exactly as
    long as its function says (K._workspace inside `isolated`), bit-equal to the run on ordinary allocations."""
    from test_gpu_isolation import isolated
    N, cg, G, H, W, s = geom
    C = cg * G
    X, Wt, dY = grad_case(geom, 8100 + sum(geom))
    dW, dX = grouped_backward_oracle(X, Wt, dY, G, s)
    # how many (m, tap, output pixel) terms each dx element receives, from the definition
    oh, ow = out_hw(H, W, s)
    terms = np.zeros((H, W), int)
    for ky in range(3):
        for kx in range(3):
            for oy in range(oh):
                for ox in range(ow):
                    iy, ix = oy * s + ky - 1, ox * s + kx - 1
                    if 0 <= iy < H and 0 <= ix < W:
                        terms[iy, ix] += 1
    assert terms.min() >= 1                      # pad 1: no dx element without a contribution (see the module docstring)
    L = K.lib()
    floats, dfloats = L.ssad_grouped_conv3x3_filter_floats(C, G), L.ssad_grouped_conv3x3_dgrad_filter_floats(C, G)
    assert floats == dfloats

    def fn(al):
        w = al.inp("w", Wt)
        x, dy = al.inp("x", X), al.inp("dy", dY)
        packed = K.grouped_conv3x3_pack_filter(w, G, out=al.out("packed", floats))
        packed_d = K.grouped_conv3x3_pack_filter_dgrad(w, G, out=al.out("packed_dgrad", dfloats))
        dx = K.grouped_conv3x3_dgrad(dy, None, G, s, (H, W), out=al.out("dx", X.shape), packed=packed_d)
        dxm = K.grouped_conv3x3_dgrad(dy, None, G, s, (H, W), relu_x=x, out=al.out("dx_masked", X.shape), packed=packed_d)
        dw = K.grouped_conv3x3_wgrad(x, dy, G, s, out=al.out("dw", Wt.shape))
        return dict(dx=dx, dx_masked=dxm, dw=dw, packed=packed, packed_dgrad=packed_d)

    got = isolated(K, monkeypatch, fn)
    close(got["dx"], dX, CONV_RTOL, CONV_FLOOR, "dX")
    close(got["dx_masked"], np.where(X > 0, dX, np.float32(0)), CONV_RTOL, CONV_FLOOR, "masked dX")
    close(got["dw"], dW, CONV_RTOL, CONV_FLOOR, "dW")
    # either pack: the filter's words and zeros for the idle MFMA rows of groups narrower than 16, nothing else
    pad = floats - Wt.size
    want = np.sort(np.concatenate([Wt.ravel(), np.zeros(pad, np.float32)]))
    assert np.array_equal(np.sort(got["packed"].ravel()), want)
    assert np.array_equal(np.sort(got["packed_dgrad"].ravel()), want)


# ---- 4. non-finite locality --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cg,G", [(8, 3), (64, 2)], ids=["cg8", "cg64"])
@pytest.mark.parametrize("s", [1, 2])
def test_nan_in_dy_stays_in_its_image_group_and_window(K, s, cg, G):
    N, H, W = 2, 9, 13
    X, Wt, dY = grad_case((N, cg, G, H, W, s), 4400 + s + cg)
    oh, ow = out_hw(H, W, s)
    tw = dev(Wt)
    clean = K.grouped_conv3x3_dgrad(dev(dY), tw, G, s, (H, W)).cpu().numpy()
    assert np.all(np.isfinite(clean))
    n0, ch, oy, ox = 1, cg + 3, oh // 2, ow // 2                # group 1
    dYn = dY.copy()
    dYn[n0, ch, oy, ox] = np.nan
    got = K.grouped_conv3x3_dgrad(dev(dYn), tw, G, s, (H, W)).cpu().numpy()
    want = np.zeros(X.shape, bool)
    for ky in range(3):
        for kx in range(3):
            iy, ix = oy * s + ky - 1, ox * s + kx - 1           # the definition: dy(oy, ox) reaches dx(oy s + ky - 1, ..)
            if 0 <= iy < H and 0 <= ix < W:
                want[n0, cg:2 * cg, iy, ix] = True
    assert want.sum() == 9 * cg
    assert np.array_equal(np.isnan(got), want)
    assert np.array_equal(got[~want].view(np.uint32), clean[~want].view(np.uint32))


@pytest.mark.parametrize("cg,G", [(4, 5), (64, 2)], ids=["cg4", "cg64"])
@pytest.mark.parametrize("s", [1, 2])
def test_nan_in_x_stays_in_its_groups_rows_its_channels_column_and_its_taps(K, s, cg, G):
    N, H, W = 2, 10, 19                                         # two tile columns, a ragged last one
    X, Wt, dY = grad_case((N, cg, G, H, W, s), 4500 + s + cg)
    oh, ow = out_hw(H, W, s)
    tdy = dev(dY)
    clean = K.grouped_conv3x3_wgrad(dev(X), tdy, G, s).cpu().numpy()
    assert np.all(np.isfinite(clean))
    for iy, ix in ((4, 7), (H - 1, W - 1)):                     # the interior; the corner the padded outputs would read
        c = 2
        Xn = X.copy()
        Xn[1, cg + c, iy, ix] = np.nan                          # group 1, input channel c
        got = K.grouped_conv3x3_wgrad(dev(Xn), tdy, G, s).cpu().numpy()
        want = np.zeros(Wt.shape, bool)
        for ky in range(3):
            for kx in range(3):
                ny, nx = iy - ky + 1, ix - kx + 1               # the definition: x(oy s + ky - 1, ..) with oy in the map
                if ny % s == 0 and nx % s == 0 and 0 <= ny // s < oh and 0 <= nx // s < ow:
                    want[cg:2 * cg, c, ky, kx] = True
        assert 0 < want.sum() <= 9 * cg
        assert np.array_equal(np.isnan(got), want), (iy, ix)
        assert np.array_equal(got[~want].view(np.uint32), clean[~want].view(np.uint32))


# ---- 5. deterministic ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", [(2, 4, 16, 19, 23, 2), (2, 64, 1, 9, 19, 1)], ids=GEOM_ID)
def test_both_gradients_are_deterministic(K, geom):
    N, cg, G, H, W, s = geom
    assert wgrad_partials(K, geom) > 1                          # the filter gradient spans several partials
    X, Wt, dY, _, _ = reference(geom)
    tx, tw, tdy = dv(X), dv(Wt), dv(dY)
    for run in (lambda: K.grouped_conv3x3_dgrad(tdy, tw, G, s, (H, W), relu_x=tx),
                lambda: K.grouped_conv3x3_wgrad(tx, tdy, G, s)):
        a, b = run(), run()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 6. operators ----------------------------------------------------------------------------------------------------

@pytest.fixture
def fresh_workspace():
    dyndep.InitOpsLibrary()
    workspace.ResetWorkspace()
    yield
    workspace.ResetWorkspace()


def feed(name, arr):
    workspace.FeedBlob(name, arr, device_option=GPU)


def run_conv_and_gradient(tag, G, s, kernel=3, pad=1, **extra):
    """Conv + the ConvGradient its gradient maker emits, through RunOperatorOnce; (Y, dW, db, dX)"""
    with core.DeviceScope(GPU):
        conv = core.CreateOperator("Conv", ["X", "w", "b"], ["Y" + tag], kernel=kernel, pad=pad, stride=s, group=G,
                                   order="NCHW", **extra)
    workspace.RunOperatorOnce(conv)
    gops, _ = core.GradientRegistry.GetGradientForOp(conv, ["Y_grad"])
    assert [o.type for o in gops] == ["ConvGradient"]
    algo = [a.s.decode() if isinstance(a.s, bytes) else a.s for a in gops[0].arg if a.name == "hip_algo"]
    assert algo == ([extra["hip_algo"]] if "hip_algo" in extra else [])      # the gradient maker carries the argument
    workspace.RunOperatorsOnce(gops)
    return [workspace.FetchBlob(n) for n in ("Y" + tag, "w_grad", "b_grad", "X_grad")]


@pytest.mark.parametrize("cg,G,s,hw", [(8, 3, 2, (11, 21)), (64, 2, 1, (9, 19))], ids=["cg8_s2", "cg64_s1"])
def test_operators_with_hip_algo_grouped(fresh_workspace, cg, G, s, hw):
    rng = np.random.default_rng(600 + cg)
    N, C = 2, cg * G
    H, W = hw
    X = rng.standard_normal((N, C, H, W)).astype(np.float32)
    Wt = (rng.standard_normal((C, cg, 3, 3)) * (1.0 / np.sqrt(9 * cg))).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    xt, wt, bt = (torch.tensor(v, requires_grad=True) for v in (X, Wt, b))
    yt = torch.nn.functional.conv2d(xt, wt, bt, s, 1, 1, G)
    dY = rng.standard_normal(tuple(yt.shape)).astype(np.float32)
    yt.backward(torch.tensor(dY))
    feed("X", X); feed("w", Wt); feed("b", b); feed("Y_grad", dY)
    want = [yt.detach().numpy(), wt.grad.numpy(), bt.grad.numpy(), xt.grad.numpy()]
    grouped = run_conv_and_gradient("g", G, s, hip_algo="grouped")
    default = run_conv_and_gradient("d", G, s)
    for name, g, d, t in zip(("Y", "dW", "db", "dX"), grouped, default, want):
        close(g, t, CONV_RTOL, CONV_FLOOR, name + " vs torch")
        close(g, d, CONV_RTOL, CONV_FLOOR, name + " vs the default engine")

    # fuse_relu on the forward operator, relu_grad_on_input on the gradient: the unfused result masked on the host
    with core.DeviceScope(GPU):
        fused = core.CreateOperator("Conv", ["X", "w", "b"], ["Yr"], kernel=3, pad=1, stride=s, group=G, order="NCHW",
                                    hip_algo="grouped", fuse_relu=1)
        gfused = core.CreateOperator("ConvGradient", ["X", "w", "Y_grad"], ["w_grad_r", "b_grad_r", "X_grad_r"], kernel=3,
                                     pad=1, stride=s, group=G, order="NCHW", hip_algo="grouped", relu_grad_on_input=1)
    workspace.RunOperatorOnce(fused)
    assert np.array_equal(workspace.FetchBlob("Yr"), np.maximum(grouped[0], 0))
    workspace.RunOperatorOnce(gfused)
    masked = np.where(X > 0, grouped[3], np.float32(0))
    assert np.array_equal(workspace.FetchBlob("X_grad_r").view(np.uint32), masked.view(np.uint32))
    assert np.array_equal(workspace.FetchBlob("w_grad_r"), grouped[1])

    # what the grouped engine does not take fails by the operator's name, with the geometry -- no fall-back
    with core.DeviceScope(GPU):
        sig = core.CreateOperator("Conv", ["X", "w", "b"], ["Ys"], kernel=3, pad=1, stride=s, group=G, order="NCHW",
                                  hip_algo="grouped", fuse_sigmoid=1)
    with pytest.raises(Exception, match=r"Conv\(hip_algo=grouped\).*fuse_sigmoid"):
        workspace.RunOperatorOnce(sig)
    feed("w5", np.zeros((C, cg, 5, 5), np.float32))
    with core.DeviceScope(GPU):
        k5 = core.CreateOperator("Conv", ["X", "w5", "b"], ["Y5"], kernel=5, pad=2, stride=s, group=G, order="NCHW",
                                 hip_algo="grouped")
        g5 = core.CreateOperator("ConvGradient", ["X", "w5", "Y_grad"], ["w5_grad", "b5_grad", "X5_grad"], kernel=5,
                                 pad=2, stride=s, group=G, order="NCHW", hip_algo="grouped")
    with pytest.raises(Exception, match=r"Conv\(hip_algo=grouped\): kernel 5x5.*group %d" % G):
        workspace.RunOperatorOnce(k5)
    with pytest.raises(Exception, match=r"ConvGradient\(hip_algo=grouped\): kernel 5x5.*group %d" % G):
        workspace.RunOperatorOnce(g5)


def test_operator_packs_follow_the_filter_blob(fresh_workspace):
    """a net of Conv + ConvGradient with hip_algo="grouped": two packs on the first run, none on the second, two
    again after the filter blob was written"""
    rng = np.random.default_rng(77)
    N, cg, G, H, W, s = 1, 16, 2, 8, 16, 1
    C = cg * G
    feed("X", rng.standard_normal((N, C, H, W)).astype(np.float32))
    Wt = (rng.standard_normal((C, cg, 3, 3)) * 0.1).astype(np.float32)
    feed("w", Wt)
    feed("Y_grad", rng.standard_normal((N, C, H, W)).astype(np.float32))
    net = core.Net("grouped_packs")
    with core.DeviceScope(GPU):
        net.Conv(["X", "w"], "Y", kernel=3, pad=1, stride=s, group=G, order="NCHW", hip_algo="grouped")
    net.AddGradientOperators({"Y": "Y_grad"})
    ops = net.Proto().op
    assert [o.type for o in ops] == ["Conv", "ConvGradient"]
    assert all(any(a.name == "hip_algo" for a in o.arg) for o in ops)
    workspace.CreateNet(net)
    p0 = workspace.Counter("filter_packs")
    workspace.RunNet(net)
    assert workspace.Counter("filter_packs") - p0 == 2
    first = workspace.FetchBlob("X_grad")
    workspace.RunNet(net)
    assert workspace.Counter("filter_packs") - p0 == 2
    assert np.array_equal(workspace.FetchBlob("X_grad"), first)
    feed("w", Wt * 2)
    workspace.RunNet(net)
    assert workspace.Counter("filter_packs") - p0 == 4
    close(workspace.FetchBlob("X_grad"), first * 2, CONV_RTOL, CONV_FLOOR, "dX after the filter write")


# ---- 7. one bottleneck on the net route ------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 2])
def test_bottleneck_net_grouped_engine_vs_default_engine(fresh_workspace, stride):
    """1x1 -> grouped 3x3 (cardinality 4 x width 4) -> 1x1 + projection shortcut, built by the builder, forward and
    backward as a net: the gradient maker and the lowering carry hip_algo, every parameter gradient agrees."""
    from ssad_amd.modeling import resnet_fpn as rf
    rng = np.random.default_rng(707)
    N, dim_in, dim_out, H, W = 2, 32, 64, 16, 16
    results, values = {}, None
    for engine in (True, False):
        workspace.ResetWorkspace()
        model = rf.BodyModel(rf.BodyConfig(stride_1x1=False, num_groups=4, width_per_group=4, grouped_engine=engine),
                             name="bottleneck_%d" % engine)
        with core.DeviceScope(GPU):
            out = rf.add_residual_block(model, "res2_0", "data", dim_in, dim_out, 16, 1, stride_init=stride)
        fwd = list(model.net.Proto().op)
        tagged = [o for o in fwd if any(a.name == "hip_algo" for a in o.arg)]
        assert [(o.type, list(o.output)) for o in tagged] == ([("Conv", ["res2_0_branch2b"])] if engine else [])
        if values is None:
            values = {"data": rng.standard_normal((N, dim_in, H, W)).astype(np.float32)}
            for name, shape, _ in model.params:
                if name.endswith("_s"):
                    v = rng.uniform(0.5, 1.5, shape)
                elif name.endswith("_b"):
                    v = rng.standard_normal(shape) * 0.1
                else:
                    v = rng.standard_normal(shape) * np.sqrt(2.0 / int(np.prod(shape[1:])))
                values[name] = v.astype(np.float32)
            oh, ow = out_hw(H, W, stride)
            values["out_grad_in"] = rng.standard_normal((N, dim_out, oh, ow)).astype(np.float32)
        for name, v in values.items():
            feed(name, v)
        grad_map = model.net.AddGradientOperators({str(out): "out_grad_in"})
        bwd = list(model.net.Proto().op)[len(fwd):]
        gtag = [o for o in bwd if any(a.name == "hip_algo" for a in o.arg)]
        assert [(o.type, list(o.input)[:2]) for o in gtag] == \
            ([("ConvGradient", ["res2_0_branch2a", "res2_0_branch2b_w"])] if engine else [])
        workspace.CreateNet(model.net)
        workspace.RunNet(model.net)
        filters = [n for n, _, _ in model.params if n.endswith("_w")]
        assert len(filters) == 4 and all(n in grad_map for n in filters)
        results[engine] = {n: workspace.FetchBlob(grad_map[n]) for n in filters}
        results[engine]["out"] = workspace.FetchBlob(str(out))
        results[engine]["data_grad"] = workspace.FetchBlob(grad_map["data"]) if "data" in grad_map else None
    for name, ref in results[False].items():
        if ref is None:
            continue
        assert float(np.abs(ref).max()) > 0
        close(results[True][name], ref, CONV_RTOL, CONV_FLOOR, name)
