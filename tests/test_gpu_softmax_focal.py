"""The softmax RetinaNet head on the device: csrc/kernels/softmax_focal.hip through the C entry points, the kernel
wrappers, the operators, the graph builder and RetinanetDetector(softmax=True), against
tests/golden/softmax_focal_ref*.npz (the reference's own kernels, see make_softmax_focal_golden.py).

Gate: P and dX per element within 1e-4 * max|ref|, a loss within 1e-4 relative (1e-7 absolute where the reference
loss is 0) -- the project's fp32 parity gate."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ssad_amd  # noqa: E402,F401
from ssad_amd import kernels as K  # noqa: E402
from ssad_amd.caffe2_hip import caffe2_pb2, core, dyndep, workspace  # noqa: E402
from ssad_amd.modeling import retinanet_heads as rh  # noqa: E402
from test_softmax_heads_cpu import load_fixture  # noqa: E402

pytestmark = pytest.mark.gpu
GATE = 1e-4
GPU = core.DeviceOption(caffe2_pb2.CUDA, 0)


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda().contiguous()


def scalar(v):
    return torch.tensor([float(v)], dtype=torch.float32, device="cuda")


def within(got, ref, what):
    """per element within GATE * max|ref|; returns the error as a fraction of max|ref|"""
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    top = float(np.abs(ref).max())
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    assert np.isfinite(got).all(), what
    assert err <= GATE * top, (what, err, top)
    return err / top if top > 0 else 0.0


def loss_close(got, ref, what):
    got, ref = float(got), float(ref)
    if ref == 0.0:
        assert abs(got) <= 1e-7, (what, got)
        return 0.0
    assert abs(got - ref) <= GATE * abs(ref), (what, got, ref)
    return abs(got - ref) / abs(ref)


def single_cases(fx):
    for k, (name, dset) in enumerate(zip(fx["case_names"], fx["case_sets"])):
        dset = str(dset)
        gamma, alpha, scale, dloss = [float(v) for v in fx["case_%d_params" % k]]
        yield dict(name=str(name), x=fx["x_" + dset].astype(np.float32), p=fx["p_" + dset],
                   labels=fx["case_%d_labels" % k].astype(np.int32), fg=float(fx["case_%d_fg" % k][0]),
                   C=int(fx["shape_" + dset][2]), loss=float(fx["case_%d_loss" % k][0]), dx=fx["case_%d_dx" % k],
                   dloss=dloss, kw=dict(gamma=gamma, alpha=alpha, scale=scale))


def level_case(fx):
    gamma, alpha, scale, dloss, fg = [float(v) for v in fx["lv_params"]]
    n = len(fx["lv_maps"])
    return dict(xs=[fx["lv_%d_x" % l].astype(np.float32) for l in range(n)],
                labels=[fx["lv_%d_labels" % l].astype(np.int32) for l in range(n)],
                ps=[fx["lv_%d_p" % l] for l in range(n)], dxs=[fx["lv_%d_dx" % l] for l in range(n)],
                loss=fx["lv_loss"], fg=fg, dloss=dloss, C=81, kw=dict(gamma=gamma, alpha=alpha, scale=scale))


def run(levels, fg, dloss, C_, kw):
    """forward + backward of one call -> (losses, probs, dxs) device tensors"""
    fgt, dl = scalar(fg), scalar(dloss)
    losses, probs = K.softmax_focal_loss_forward(levels, fgt, num_classes=C_, **kw)
    dxs = K.softmax_focal_loss_backward(levels, probs, fgt, dl, num_classes=C_, **kw)
    return losses, probs, dxs


def test_every_fixture_case(fx):
    worst = dict(p=0.0, dx=0.0, loss=0.0)
    for c in single_cases(fx):
        x, t = dev(c["x"]), dev(c["labels"])
        losses, probs, dxs = run([(x, t)], c["fg"], c["dloss"], c["C"], c["kw"])
        e = (within(probs[0], c["p"], c["name"] + " P"), within(dxs[0], c["dx"], c["name"] + " dX"),
             loss_close(losses[0], c["loss"], c["name"] + " loss"))
        print("%-16s P %.2e  dX %.2e  loss %.2e" % ((c["name"],) + e))
        worst = dict(p=max(worst["p"], e[0]), dx=max(worst["dx"], e[1]), loss=max(worst["loss"], e[2]))
    print("measured maxima (fraction of max|ref| / relative):", worst)


def test_all_ignore_is_exactly_zero_and_still_writes_p(fx):
    c = [c for c in single_cases(fx) if c["name"] == "s3_ignore"][0]
    x, t = dev(c["x"]), dev(c["labels"])
    assert int(t.max()) == -1
    probs = [torch.full_like(x, float("nan"))]
    out = [torch.full_like(x, float("nan"))]
    fg, dl = scalar(c["fg"]), scalar(1.0)
    losses, probs = K.softmax_focal_loss_forward([(x, t)], fg, num_classes=c["C"], probs=probs, **c["kw"])
    dxs = K.softmax_focal_loss_backward([(x, t)], probs, fg, dl, num_classes=c["C"], out=out, **c["kw"])
    assert float(losses[0]) == 0.0
    assert not bool(dxs[0].ne(0).any()) and not bool(torch.isnan(dxs[0]).any())
    within(probs[0], c["p"], "P of an all-ignore level")


@pytest.mark.parametrize("dset", ["s1_normal", "s2_normal", "s3_wide", "s4_normal"])
def test_drop_background_is_the_full_output_without_channel_0(fx, dset):
    x = dev(fx["x_" + dset].astype(np.float32))
    N, A, C_, H, W = [int(v) for v in fx["shape_" + dset]]
    full = K.group_spatial_softmax(x, C_)
    within(full, fx["p_" + dset], "GroupSpatialSoftmax " + dset)
    out = torch.full((N, A * (C_ - 1), H, W), -7.0, dtype=torch.float32, device="cuda")
    drop = K.group_spatial_softmax(x, C_, drop_background=True, out=out)
    assert drop is out
    want = full.view(N, A, C_, H, W)[:, :, 1:].reshape(N, A * (C_ - 1), H, W)
    assert torch.equal(drop, want)
    # the loss's own forward writes the same probabilities
    _, probs = K.softmax_focal_loss_forward([(x, torch.zeros((N, A, H, W), dtype=torch.int32, device="cuda"))],
                                            scalar(1.0), num_classes=C_)
    assert torch.equal(probs[0], full)


def test_softmax_gradient_against_fixture_and_autograd(fx):
    for dset in [str(s) for s in fx["sg_sets"]]:
        N, A, C_, H, W = [int(v) for v in fx["shape_" + dset]]
        y = dev(fx["p_" + dset])
        dy = dev(fx["sg_%s_dy" % dset].astype(np.float32))
        dx = K.group_spatial_softmax_grad(y, dy, C_)
        e = within(dx, fx["sg_%s_dx" % dset], "softmax gradient " + dset)
        # autograd of torch.softmax over the regrouped logits, in float64
        x = dev(fx["x_" + dset].astype(np.float32)).double().view(N, A, C_, H, W).requires_grad_(True)
        torch.softmax(x, dim=2).backward(dy.double().view(N, A, C_, H, W))
        e2 = within(dx, x.grad.reshape(N, A * C_, H, W).cpu().numpy(), "softmax gradient vs autograd " + dset)
        # and with the device's own probabilities as input (what the operator pair does)
        y2 = K.group_spatial_softmax(dev(fx["x_" + dset].astype(np.float32)), C_)
        within(K.group_spatial_softmax_grad(y2, dy, C_), x.grad.reshape(N, A * C_, H, W).cpu().numpy(),
               "softmax + gradient vs autograd " + dset)
        print("softmax gradient %-10s fixture %.2e  autograd %.2e" % (dset, e, e2))


def test_two_runs_are_bit_identical(fx):
    c = [c for c in single_cases(fx) if c["name"] == "s1_mixed"][0]
    x, t = dev(c["x"]), dev(c["labels"])
    a = run([(x, t)], c["fg"], c["dloss"], c["C"], c["kw"])
    b = run([(x, t)], c["fg"], c["dloss"], c["C"], c["kw"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0]) and torch.equal(a[2][0], b[2][0])


def test_five_level_call_equals_five_one_level_calls(fx):
    c = level_case(fx)
    levels = [(dev(x), dev(t)) for x, t in zip(c["xs"], c["labels"])]
    losses, probs, dxs = run(levels, c["fg"], c["dloss"], c["C"], c["kw"])
    assert tuple(losses.shape) == (5,)
    worst = dict(p=0.0, dx=0.0, loss=0.0)
    for l, lv in enumerate(levels):
        l1, p1, d1 = run([lv], c["fg"], c["dloss"], c["C"], c["kw"])
        assert torch.equal(l1[0], losses[l]) and torch.equal(p1[0], probs[l]) and torch.equal(d1[0], dxs[l]), l
        worst["p"] = max(worst["p"], within(probs[l], c["ps"][l], "level %d P" % l))
        worst["dx"] = max(worst["dx"], within(dxs[l], c["dxs"][l], "level %d dX" % l))
        worst["loss"] = max(worst["loss"], loss_close(losses[l], c["loss"][l], "level %d loss" % l))
    print("five-level call, measured maxima:", worst)
    # one dloss per level (stride 1) scales each level's gradient by its own value
    fg = scalar(c["fg"])
    dl = torch.tensor([1.0, 2.0, 0.5, 4.0, 0.25], dtype=torch.float32, device="cuda")
    per = K.softmax_focal_loss_backward(levels, probs, fg, dl, num_classes=c["C"], **c["kw"])
    for l in range(5):
        one = K.softmax_focal_loss_backward([levels[l]], [probs[l]], fg, dl[l:l + 1], num_classes=c["C"], **c["kw"])
        assert torch.equal(per[l], one[0])
        assert torch.equal(per[l], dxs[l] * dl[l])        # powers of two: exact


def test_launcher_rejections_leave_the_outputs_untouched():
    L = K.lib()
    N, A, C_, H, W = 1, 2, 5, 3, 4
    x = torch.randn((N, A * C_, H, W), device="cuda")
    t = torch.zeros((N, A, H, W), dtype=torch.int32, device="cuda")
    SENT = -123.0
    p, out, loss = torch.full_like(x, SENT), torch.full_like(x, SENT), torch.full((1,), SENT, device="cuda")
    fg, dl = scalar(1.0), scalar(1.0)
    nb = L.ssad_softmax_focal_loss_workspace_bytes(1)
    assert nb > 0 and L.ssad_softmax_focal_loss_workspace_bytes(5) >= nb
    ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    st = K._stream()
    BAD, WS = -1, -2          # SSAD_E_BADARG, SSAD_E_WORKSPACE

    def level(**kw):
        d = dict(logits=x.data_ptr(), labels=t.data_ptr(), prob=p.data_ptr(), out=loss.data_ptr(), N=N, D=A * C_, H=H, W=W)
        d.update(kw)
        return (K.SoftmaxFocalLevel * 1)(K.SoftmaxFocalLevel(**d))

    def fwd(arr, n=1, fgp=fg, P=None, wsp=ws, wsb=nb):
        P = P or K.FocalParams(2.0, 0.25, C_, 1.0)
        return L.ssad_softmax_focal_loss_forward(arr, n, K._ptr(fgp), C.byref(P) if P is not False else None,
                                                 K._ptr(wsp), wsb, st)

    def bwd(arr, n=1, fgp=fg, dlp=dl, stride=0, P=None):
        P = P or K.FocalParams(2.0, 0.25, C_, 1.0)
        return L.ssad_softmax_focal_loss_backward(arr, n, K._ptr(fgp), K._ptr(dlp), stride, C.byref(P), st)

    assert fwd(level(logits=0)) == BAD and fwd(level(labels=0)) == BAD and fwd(level(prob=0)) == BAD
    assert fwd(level(out=0)) == BAD and fwd(level(), fgp=None) == BAD and fwd(None) == BAD
    assert fwd(level(D=A * C_ + 1)) == BAD                                   # D % C != 0
    assert fwd(level(), P=K.FocalParams(2.0, 0.25, 1, 1.0)) == BAD           # C out of range
    assert fwd(level(D=129), P=K.FocalParams(2.0, 0.25, 129, 1.0)) == BAD
    for k in ("N", "D", "H", "W"):
        assert fwd(level(**{k: 0})) == BAD and fwd(level(**{k: -1})) == BAD  # non-positive extent
    assert fwd(level(), P=K.FocalParams(2.0, 0.25, C_, -1.0)) == BAD         # scale < 0
    assert fwd(level(), wsb=8 * 1 - 1) == WS and fwd(level(), wsp=None) == WS    # workspace too small / null
    assert fwd(level(), n=K.MAX_LEVELS + 1) == BAD and fwd(level(), n=-1) == BAD
    assert fwd(level(), n=0) == 0                                            # zero-sized call: nothing is launched
    out_level = level(out=out.data_ptr())
    assert bwd(level(prob=0, out=out.data_ptr())) == BAD and bwd(level(out=0)) == BAD
    assert bwd(out_level, dlp=None) == BAD and bwd(out_level, stride=-1) == BAD and bwd(out_level, fgp=None) == BAD
    assert bwd(level(out=out.data_ptr(), D=A * C_ + 1)) == BAD and bwd(level(out=out.data_ptr(), H=0)) == BAD
    assert bwd(out_level, n=K.MAX_LEVELS + 1) == BAD and bwd(out_level, n=0) == 0
    assert bwd(out_level, P=K.FocalParams(2.0, 0.25, 200, 1.0)) == BAD
    y = torch.full_like(x, SENT)
    gs, gg = L.ssad_group_spatial_softmax, L.ssad_group_spatial_softmax_grad
    assert gs(None, K._ptr(y), N, A, C_, H, W, 0, st) == BAD and gs(K._ptr(x), None, N, A, C_, H, W, 0, st) == BAD
    assert gs(K._ptr(x), K._ptr(y), N, A, 1, H, W, 0, st) == BAD and gs(K._ptr(x), K._ptr(y), N, A, 129, H, W, 0, st) == BAD
    for dims in ((0, A, H, W), (N, 0, H, W), (N, A, -3, W), (N, A, H, 0)):
        assert gs(K._ptr(x), K._ptr(y), dims[0], dims[1], C_, dims[2], dims[3], 1, st) == BAD
        assert gg(K._ptr(x), K._ptr(x), K._ptr(y), dims[0], dims[1], C_, dims[2], dims[3], st) == BAD
    assert gg(None, K._ptr(x), K._ptr(y), N, A, C_, H, W, st) == BAD and gg(K._ptr(x), None, K._ptr(y), N, A, C_, H, W, st) == BAD
    assert gg(K._ptr(x), K._ptr(x), None, N, A, C_, H, W, st) == BAD and gg(K._ptr(x), K._ptr(x), K._ptr(y), N, A, 0, H, W, st) == BAD
    torch.cuda.synchronize()
    for buf in (p, out, loss, y):
        assert bool((buf == SENT).all())
    # and the same arguments, valid, do run
    assert fwd(level()) == 0 and bwd(out_level) == 0 and gs(K._ptr(x), K._ptr(y), N, A, C_, H, W, 0, st) == 0
    torch.cuda.synchronize()
    assert not bool((p == SENT).any()) and not bool((out == SENT).any()) and torch.equal(y, p)
    # wrapper-level shape checks
    with pytest.raises(K.KernelError):
        K.group_spatial_softmax(x, 3)
    with pytest.raises(K.KernelError):
        K.softmax_focal_loss_forward([(x, t[:, :, :, :3].contiguous())], fg, num_classes=C_)


# ---------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------

@pytest.fixture
def fresh_workspace():
    dyndep.InitOpsLibrary()
    workspace.ResetWorkspace()
    yield
    workspace.ResetWorkspace()


def feed(name, arr):
    workspace.FeedBlob(name, arr, device_option=GPU)


def test_softmax_focal_loss_net_equals_the_wrappers(fx, fresh_workspace):
    c = [c for c in single_cases(fx) if c["name"] == "s3_mixed_g15"][0]
    feed("logits", c["x"]); feed("labels", c["labels"]); feed("fg", np.array(c["fg"], np.float32))
    with core.DeviceScope(GPU):
        net = core.Net("softmax_focal")
        loss, prob = net.SoftmaxFocalLoss(["logits", "labels", "fg"], ["fl", "retnet_prob"], num_classes=c["C"], **c["kw"])
        grad_map = net.AddGradientOperators([loss])
    ops = list(net.Proto().op)
    assert [op.type for op in ops] == ["SoftmaxFocalLoss", "ConstantFill", "SoftmaxFocalLossGradient"]
    assert list(ops[2].input) == ["logits", "labels", "fg", "retnet_prob", "fl_autogen_grad"]
    workspace.CreateNet(net)
    workspace.RunNet(net)
    x, t = dev(c["x"]), dev(c["labels"])
    losses, probs, dxs = run([(x, t)], c["fg"], 1.0, c["C"], c["kw"])
    got_loss, got_p, got_dx = workspace.FetchBlob("fl"), workspace.FetchBlob("retnet_prob"), workspace.FetchBlob(grad_map["logits"])
    assert got_loss.shape == () and got_p.shape == c["x"].shape and got_dx.shape == c["x"].shape
    assert got_loss.tobytes() == losses[0].cpu().numpy().tobytes()
    assert got_p.tobytes() == probs[0].cpu().numpy().tobytes()
    assert got_dx.tobytes() == dxs[0].cpu().numpy().tobytes()
    within(got_p, c["p"], "operator P")
    # defaults of the reference: gamma 1, alpha 0.25, num_classes 81, scale 1
    c81 = [c for c in single_cases(fx) if c["name"] == "s2_mixed"][0]
    feed("x81", c81["x"]); feed("t81", c81["labels"])
    with core.DeviceScope(GPU):
        op = core.CreateOperator("SoftmaxFocalLoss", ["x81", "t81", "fg"], ["l81", "p81"])
    workspace.RunOperatorOnce(op)
    want, _ = K.softmax_focal_loss_forward([(dev(c81["x"]), dev(c81["labels"]))], scalar(c["fg"]), gamma=1.0, alpha=0.25,
                                           num_classes=81, scale=1.0)
    assert workspace.FetchBlob("l81").tobytes() == want[0].cpu().numpy().tobytes()
    feed("badlabels", np.zeros((2, 3, 13, 20), np.int32))
    with core.DeviceScope(GPU):
        bad = core.CreateOperator("SoftmaxFocalLoss", ["logits", "badlabels", "fg"], ["l2", "p2"], num_classes=5)
    with pytest.raises(Exception, match="labels must be"):
        workspace.RunOperatorOnce(bad)


def test_group_spatial_softmax_net_equals_the_wrappers(fx, fresh_workspace):
    dset = "s3_normal"
    C_ = int(fx["shape_" + dset][2])
    x = fx["x_" + dset].astype(np.float32)
    dy = fx["sg_%s_dy" % dset].astype(np.float32)
    feed("x", x); feed("dy", dy)
    with core.DeviceScope(GPU):
        net = core.Net("group_softmax")
        y = net.GroupSpatialSoftmax("x", "y", num_classes=C_)
        grad_map = net.AddGradientOperators({y: "dy"})
    assert [op.type for op in net.Proto().op] == ["GroupSpatialSoftmax", "GroupSpatialSoftmaxGradient"]
    workspace.CreateNet(net)
    workspace.RunNet(net)
    yk = K.group_spatial_softmax(dev(x), C_)
    dxk = K.group_spatial_softmax_grad(yk, dev(dy), C_)
    assert workspace.FetchBlob("y").tobytes() == yk.cpu().numpy().tobytes()
    assert workspace.FetchBlob(grad_map["x"]).tobytes() == dxk.cpu().numpy().tobytes()
    within(workspace.FetchBlob("y"), fx["p_" + dset], "operator softmax")


def test_softmax_student_graph_end_to_end(fx, fresh_workspace):
    """Towers, cls_pred, SoftmaxFocalLoss, SelectSmoothL1Loss and their gradients at the five small maps, built by
    modeling.retinanet_heads with softmax=True and run through CreateNet / RunNet; the gradient that reaches the
    cls_pred logits is the fixture-checked kernel's, applied to the fetched logits."""
    from ssad_amd import synth
    maps = [tuple(int(v) for v in m) for m in fx["lv_maps"]]
    cfg = rh.HeadConfig(softmax=True, fpn_dim=32, num_convs=1, num_gpus=8)
    levels = list(cfg.levels())
    with core.DeviceScope(GPU):
        student = rh.HeadModel(cfg, train=True, name="softmax_student")
        rh.add_fpn_retinanet_outputs(student, ["fpn_%d" % l for l in reversed(levels)], cfg.fpn_dim)
        loss_grads = rh.add_fpn_retinanet_losses(student)
        grad_map = student.net.AddGradientOperators(loss_grads)
    types = [op.type for op in student.net.Proto().op]
    for want in ("Conv", "Relu", "SoftmaxFocalLoss", "SelectSmoothL1Loss", "SoftmaxFocalLossGradient",
                 "SelectSmoothL1LossGradient", "ConvGradient"):
        assert want in types, want
    assert "SigmoidFocalLoss" not in types
    rng = np.random.default_rng(61)
    N = 2
    for name, shape, (filler, kw) in student.params:
        if filler == "GivenTensorFill":
            v = np.asarray(kw["values"], np.float32).reshape(shape)
        elif filler == "GaussianFill":
            v = rng.standard_normal(shape).astype(np.float32) * 0.05
        else:
            v = np.full(shape, kw.get("value", 0.0), np.float32)
        feed(name, v)
    labels = [fx["lv_%d_labels" % i].astype(np.int32) for i in range(5)]
    tg = [synth.bbox_targets(rng, l) for l in labels]
    fg = np.float32(max(1, sum(t[0].shape[0] for t in tg)))
    feed("retnet_fg_num", np.array(fg, np.float32))
    for i, l in enumerate(levels):
        h, w = maps[i]
        feed("fpn_%d" % l, rng.standard_normal((N, cfg.fpn_dim, h, w)).astype(np.float32))
        feed("retnet_cls_labels_fpn%d" % l, labels[i])
        feed("retnet_roi_bbox_targets_fpn%d" % l, tg[i][0])
        feed("retnet_roi_fg_bbox_locs_fpn%d" % l, tg[i][1])
    workspace.CreateNet(student.net)
    workspace.RunNet(student.net)
    kw = dict(gamma=cfg.focal_gamma, alpha=cfg.focal_alpha, scale=cfg.loss_scale, num_classes=cfg.num_classes)
    for i, l in enumerate(levels):
        logits = workspace.FetchBlob("retnet_cls_pred_fpn%d" % l)
        assert logits.shape == (N, 9 * 81) + maps[i] and np.isfinite(logits).all()
        x, t = dev(logits), dev(labels[i])
        losses, probs = K.softmax_focal_loss_forward([(x, t)], scalar(fg), **kw)
        dxs = K.softmax_focal_loss_backward([(x, t)], probs, scalar(fg), scalar(1.0), **kw)
        assert workspace.FetchBlob("fl_fpn%d" % l).tobytes() == losses[0].cpu().numpy().tobytes()
        assert workspace.FetchBlob("retnet_prob_fpn%d" % l).tobytes() == probs[0].cpu().numpy().tobytes()
        got = workspace.FetchBlob(grad_map["retnet_cls_pred_fpn%d" % l])
        assert got.tobytes() == dxs[0].cpu().numpy().tobytes()
        assert np.abs(got).max() > 0
    for name in ("retnet_cls_pred_fpn3_w", "retnet_cls_pred_fpn3_b", "retnet_cls_conv_n0_fpn3_w",
                 "retnet_bbox_pred_fpn3_w"):
        g = workspace.FetchBlob(grad_map[name])
        assert np.isfinite(g).all() and np.abs(g).max() > 0, name
    # the bias gradient of cls_pred is the sum of the logits' gradients over images, positions and levels
    db = sum(workspace.FetchBlob(grad_map["retnet_cls_pred_fpn%d" % l]).astype(np.float64).sum(axis=(0, 2, 3))
             for l in levels)
    got = workspace.FetchBlob(grad_map["retnet_cls_pred_fpn3_b"])
    assert np.abs(got - db).max() <= GATE * np.abs(db).max()


# ---------------------------------------------------------------------------
# detector
# ---------------------------------------------------------------------------

def test_softmax_detector_from_logits():
    from ssad_amd.roi_data.retinanet import RetinanetDetector
    shapes = [(20, 28), (10, 14), (5, 7)]
    rng = np.random.default_rng(71)
    A, C_ = 9, 81
    logits, deltas = [], []
    for h, w in shapes:
        x = rng.standard_normal((1, A, C_, h, w)).astype(np.float32)
        x[:, :, 0] += 3.0                                                     # background mostly wins
        hot = rng.random((1, A, h, w)) < 0.05                                 # a few confident cells
        cls = rng.integers(1, C_, (1, A, h, w))
        boost = np.zeros_like(x)
        np.put_along_axis(boost, cls[:, :, None], 8.0 * hot[:, :, None], axis=2)
        logits.append(dev((x + boost).reshape(1, A * C_, h, w)))
        deltas.append(dev((rng.standard_normal((1, 36, h, w)) * 0.4).astype(np.float32)))
    soft = RetinanetDetector(shapes, softmax=True)
    plain = RetinanetDetector(shapes)
    got = soft(logits, deltas, 150, 210, 1.0, from_logits=True).cpu().numpy()
    assert 0 < got.shape[0] <= 100 and got[:, 5].min() >= 1          # classes 1.., the background is never reported
    probs = [K.group_spatial_softmax(x, C_, drop_background=True) for x in logits]
    want = plain(probs, deltas, 150, 210, 1.0).cpu().numpy()
    assert got.tobytes() == want.tobytes()
    # probabilities in the dropped-background layout are accepted as they are
    assert soft(probs, deltas, 150, 210, 1.0).cpu().numpy().tobytes() == want.tobytes()
    # torch's softmax with column 0 removed
    tprobs = [torch.softmax(x.view(1, A, C_, h, w), dim=2)[:, :, 1:].reshape(1, A * (C_ - 1), h, w).contiguous()
              for x, (h, w) in zip(logits, shapes)]
    tdet = plain(tprobs, deltas, 150, 210, 1.0).cpu().numpy()
    if all(torch.equal(a, b) for a, b in zip(probs, tprobs)):
        assert tdet.tobytes() == want.tobytes()
    else:
        for a, b in zip(probs, tprobs):
            within(a, b.cpu().numpy(), "softmax vs torch")
        assert tdet.shape == want.shape

        def key(d):
            return sorted((int(r[5]), tuple(np.round(r[:4], 2))) for r in d)
        assert key(tdet) == key(want)                                         # the same detections ...
        order = lambda d: d[np.lexsort((d[:, 0], d[:, 1], d[:, 5]))]          # noqa: E731
        assert np.abs(order(tdet)[:, 4] - order(want)[:, 4]).max() <= GATE * want[:, 4].max()   # ... scores within the gate
    with pytest.raises(K.KernelError):
        plain(logits, deltas, 150, 210, 1.0, from_logits=True)
    with pytest.raises(K.KernelError):
        soft(probs, deltas, 150, 210, 1.0, from_logits=True)                  # not A*(C+1) channels


def test_offsets_past_2_to_31():
    """N*A*C*H*W = 2.16e9 floats: the far end of the tensor is addressed with 64-bit offsets."""
    A, C_, H, W = 9, 81, 1720, 1720
    need = 4 * (A * C_ + A * (C_ - 1)) * H * W + (1 << 30)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs %.0f GB of free device memory" % (need / 2 ** 30))
    assert A * C_ * H * W > 2 ** 31
    x = torch.empty((1, A * C_, H, W), dtype=torch.float32, device="cuda")
    x.normal_()
    y = K.group_spatial_softmax(x, C_, drop_background=True)
    for a in (0, A - 1):                                                      # first and last (image, anchor) slab
        rows = slice(H - 2, H)
        ref = torch.softmax(x[0, a * C_:(a + 1) * C_, rows].double(), dim=0)[1:]
        got = y[0, a * (C_ - 1):(a + 1) * (C_ - 1), rows].double()
        assert float((got - ref).abs().max()) <= GATE * float(ref.max())
    del x, y
    torch.cuda.empty_cache()
