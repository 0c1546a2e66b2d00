"""The softmax RetinaNet head (RETINANET.SOFTMAX) without a GPU: the fixture against an independent float64
restatement, the graph builder, the detector's argument checks and the weights file."""
import os
import pickle

import numpy as np
import pytest
import torch

import ssad_amd  # noqa: F401
from ssad_amd import kernels as K
from ssad_amd.caffe2_hip import core
from ssad_amd.modeling import retinanet_heads as rh
from ssad_amd.roi_data.retinanet import RetinanetDetector
from ssad_amd.utils import net

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLT_MIN = float(np.finfo(np.float32).tiny)


def load_fixture():
    """The three fixture files as one dict (the five-level call is spread over two of them for size)."""
    out = {}
    for n in ("softmax_focal_ref.npz", "softmax_focal_ref_levels_a.npz", "softmax_focal_ref_levels_b.npz"):
        with np.load(os.path.join(GOLDEN, n)) as z:
            out.update({k: z[k] for k in z.files})
    return out


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


# ---------------------------------------------------------------------------
# float64 restatement of the two operators (written from the formulas, not from the kernels)
# ---------------------------------------------------------------------------

def softmax64(x, C):
    """The difference x - max is taken in float32, as any float32 implementation must (for logits 120 apart its
    rounding alone is 4e-6 of the tiny probability it produces); everything after it in float64."""
    N, D, H, W = x.shape
    g = x.astype(np.float32).reshape(N, D // C, C, H, W)
    e = np.exp((g - g.max(axis=2, keepdims=True)).astype(np.float64))
    return (e / e.sum(axis=2, keepdims=True)).reshape(x.shape)


def focal64(p, t, fg, gamma, alpha, scale, dloss, C):
    """Loss and dX from the probabilities (the gradient op consumes the forward's P)."""
    N, D, H, W = p.shape
    A = D // C
    pg = p.astype(np.float64).reshape(N, A, C, H, W)
    t = t.astype(np.int64)
    keep = t >= 0
    pl = np.take_along_axis(pg, np.clip(t, 0, C - 1)[:, :, None], axis=2)[:, :, 0]
    Np = max(float(fg), 1.0)
    z = np.where(t == 0, (1.0 - alpha) / Np, np.where(t >= 1, alpha / Np, 0.0))
    logp = np.log(np.maximum(pl, FLT_MIN))
    with np.errstate(all="ignore"):
        loss = np.where(keep, -(1.0 - pl) ** gamma * logp * z, 0.0)
        w = np.where(keep, (-(1.0 - pl) ** gamma + gamma * (1.0 - pl) ** (gamma - 1.0) * pl * logp) * z, 0.0)
    onehot = (np.arange(C).reshape(1, 1, C, 1, 1) == t[:, :, None]).astype(np.float64)
    dx = scale * dloss * w[:, :, None] * (onehot - pg) * keep[:, :, None]
    return loss.sum() * scale, dx.reshape(p.shape)


def rel_err(got, ref, floor):
    """max |got - ref| / max(|ref|, floor): elementwise relative error with a floor for the subnormal range."""
    return float(np.max(np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), floor)))


def test_fixture_matches_a_float64_restatement(fx):
    """P from the logits, loss and dX from the stored P, to 1e-6 relative.  Loss and dX hold it element by
    element (values below FLT_MIN have fewer than 24 significant bits, so the relative error is taken against
    max(|ref|, 1e3 FLT_MIN)).  P holds it as the relative L2 error of each tensor, and element by element
    within the worst case of the float formats: the reference adds the C exponentials in class order in float32,
    background (the largest, exp(0) = 1 under the head's prior) first, so the sum carries up to (C - 1) / 2 ulp and
    with one exp (1 ulp) and the division (half an ulp) an element may differ from float64 by (C + 2) 2^-24 --
    4.9e-6 at C = 81; measured on these files: 1.1e-6 on a background probability of 0.997, 3e-7 in L2."""
    floor = 1e3 * FLT_MIN
    worst = {"p": 0.0, "loss": 0.0, "dx": 0.0}
    for name in sorted(k[2:] for k in fx if k.startswith("x_")):
        x = fx["x_" + name].astype(np.float32)
        C = int(fx["shape_" + name][2])
        assert x.shape[1] == fx["shape_" + name][1] * C
        ref = softmax64(x, C)
        assert rel_err(fx["p_" + name], ref, floor) <= (C + 2) * 2.0 ** -24, name
        worst["p"] = max(worst["p"], float(np.linalg.norm(fx["p_" + name] - ref) / np.linalg.norm(ref)))
    for k, (cname, dset) in enumerate(zip(fx["case_names"], fx["case_sets"])):
        gamma, alpha, scale, dloss = [float(v) for v in fx["case_%d_params" % k]]
        C = int(fx["shape_" + str(dset)][2])
        loss, dx = focal64(fx["p_" + str(dset)], fx["case_%d_labels" % k], fx["case_%d_fg" % k][0], gamma, alpha,
                           scale, dloss, C)
        got = float(fx["case_%d_loss" % k][0])
        worst["loss"] = max(worst["loss"], abs(got - loss) / max(abs(loss), floor))
        worst["dx"] = max(worst["dx"], rel_err(fx["case_%d_dx" % k], dx, floor))
        if str(cname).endswith("ignore"):
            assert got == 0.0 and not fx["case_%d_dx" % k].any()
    gamma, alpha, scale, dloss, fg = [float(v) for v in fx["lv_params"]]
    for l, (H, W) in enumerate(fx["lv_maps"]):
        x = fx["lv_%d_x" % l].astype(np.float32)
        assert x.shape == (2, 9 * 81, H, W)
        ref = softmax64(x, 81)
        assert rel_err(fx["lv_%d_p" % l], ref, floor) <= 83 * 2.0 ** -24, l
        worst["p"] = max(worst["p"], float(np.linalg.norm(fx["lv_%d_p" % l] - ref) / np.linalg.norm(ref)))
        loss, dx = focal64(fx["lv_%d_p" % l], fx["lv_%d_labels" % l], fg, gamma, alpha, scale, dloss, 81)
        worst["loss"] = max(worst["loss"], abs(float(fx["lv_loss"][l]) - loss) / abs(loss))
        worst["dx"] = max(worst["dx"], rel_err(fx["lv_%d_dx" % l], dx, floor))
    for dset in fx["sg_sets"]:
        y = fx["p_" + str(dset)].astype(np.float64)
        dy = fx["sg_%s_dy" % dset].astype(np.float64)
        C = int(fx["shape_" + str(dset)][2])
        N, D, H, W = y.shape
        s = (y * dy).reshape(N, D // C, C, H, W).sum(axis=2, keepdims=True)
        ref = (y.reshape(N, D // C, C, H, W) * (dy.reshape(N, D // C, C, H, W) - s)).reshape(y.shape)
        # dY - s cancels where a cell's probability mass sits on one class (the head's prior puts 0.99 on the
        # background), so the float32 rounding of s, ~1e-7 |dY|, is what remains: relative to max |Y| |dY| = max |dY|
        err = np.abs(fx["sg_%s_dx" % dset] - ref).max() / np.abs(dy).max()
        assert err <= 1e-6, (dset, err)
    print("fixture vs float64:", worst)
    assert worst["p"] <= 1e-6 and worst["loss"] <= 1e-6 and worst["dx"] <= 1e-6, worst


def test_fixture_covers_the_cases_it_must(fx):
    shapes = {tuple(int(v) for v in fx[k]) for k in fx if k.startswith("shape_")}
    assert {(2, 9, 81, 5, 7), (1, 9, 81, 1, 1), (2, 3, 5, 13, 21), (1, 1, 2, 3, 3)} <= shapes
    assert [tuple(m) for m in fx["lv_maps"]] == [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
    params = np.stack([fx["case_%d_params" % k] for k in range(len(fx["case_names"]))])
    assert {(2.0, 0.25), (1.5, 0.5), (1.0, 0.25), (0.5, 0.25)} <= {(float(g), float(a)) for g, a, _, _ in params}
    assert {1.0, 0.125} <= {float(s) for _, _, s, _ in params}
    assert {0.0, 1.0, 37.5} <= {float(fx["case_%d_fg" % k][0]) for k in range(len(params))}
    for k, dset in enumerate(fx["case_sets"]):
        t = fx["case_%d_labels" % k]
        C = int(fx["shape_" + str(dset)][2])
        assert t.min() >= -1 and t.max() <= C - 1
        if float(params[k][0]) < 1.0:            # gamma < 1 only on logits with a spread of at most 8
            x = fx["x_" + str(dset)].astype(np.float32)
            assert x.max() - x.min() <= 8.0
    mixed = fx["case_%d_labels" % list(fx["case_names"]).index("s3_mixed")]
    assert (mixed == 4).any() and (mixed == -1).any() and (mixed == 0).mean() > 0.8     # incl. class C - 1


# ---------------------------------------------------------------------------
# graph builder
# ---------------------------------------------------------------------------

def _args(op):
    return {a.name: (a.i if a.HasField("i") else a.s if a.HasField("s") else a.f if a.HasField("f") else
                     list(a.floats) or list(a.ints)) for a in op.arg}


def _build(cfg, train):
    model = rh.HeadModel(cfg, train=train)
    blobs = ["fpn_%d" % lvl for lvl in range(cfg.k_max, cfg.k_min - 1, -1)]
    preds = rh.add_fpn_retinanet_outputs(model, blobs, cfg.fpn_dim)
    return model, preds


def test_softmax_builder_train_graph():
    cfg = rh.HeadConfig(softmax=True, num_convs=1, num_gpus=8)
    model, preds = _build(cfg, True)
    A, C = cfg.num_anchors, cfg.num_classes
    shapes = {n: s for n, s, _ in model.params}
    assert shapes["retnet_cls_pred_fpn3_w"] == [A * C, 256, 3, 3] and shapes["retnet_cls_pred_fpn3_b"] == [A * C]
    assert shapes["retnet_bbox_pred_fpn3_w"] == [4 * A, 256, 3, 3]
    filler, kw = dict((n, i) for n, _, i in model.params)["retnet_cls_pred_fpn3_b"]
    assert filler == "GivenTensorFill"
    bias = np.asarray(kw["values"], np.float32).reshape(A, C)
    assert np.all(bias[:, 1:] == 0.0)
    want = np.float32(np.log((C - 1) * (1 - cfg.prior_prob) / cfg.prior_prob))
    assert np.all(bias[:, 0] == want) and abs(float(want) - 8.9771) < 1e-3
    # softmax of the bias alone: every foreground class starts at prior_prob / (C - 1)
    p = np.exp(bias[0] - bias[0].max())
    p /= p.sum()
    assert abs(p[1:].sum() - cfg.prior_prob) < 1e-6
    assert not [op for op in model.net.Proto().op if op.type in ("Sigmoid", "GroupSpatialSoftmax")]

    n_fwd = len(model.net.Proto().op)
    grads = rh.add_fpn_retinanet_losses(model)
    ops = list(model.net.Proto().op)[n_fwd:]
    levels = list(cfg.levels())
    assert [op.type for op in ops] == (["SelectSmoothL1Loss"] * 5 + ["SoftmaxFocalLoss"] * 5 + ["ConstantFill"] * 10)
    for lvl, op in zip(levels, ops[5:10]):
        s = "fpn%d" % lvl
        assert list(op.input) == ["retnet_cls_pred_" + s, "retnet_cls_labels_" + s, "retnet_fg_num"]
        assert list(op.output) == ["fl_" + s, "retnet_prob_" + s]
        a = _args(op)
        assert set(a) == {"gamma", "alpha", "scale", "num_classes"}
        assert a["num_classes"] == C and a["gamma"] == 2.0 and a["alpha"] == 0.25 and a["scale"] == 0.125
    assert model.losses == ["retnet_loss_bbox_fpn%d" % l for l in levels] + ["fl_fpn%d" % l for l in levels]
    assert set(grads) == set(model.losses)                  # the probabilities get no gradient
    grad_map = model.net.AddGradientOperators(grads)
    gops = [op for op in model.net.Proto().op if op.type == "SoftmaxFocalLossGradient"]
    assert len(gops) == 5
    for op in gops:
        s = op.input[0][len("retnet_cls_pred_"):]
        assert list(op.input) == ["retnet_cls_pred_" + s, "retnet_cls_labels_" + s, "retnet_fg_num",
                                  "retnet_prob_" + s, "fl_%s_grad" % s]
        assert len(op.output) == 1 and _args(op)["num_classes"] == C
    assert "retnet_cls_pred_fpn3_w" in grad_map and "retnet_cls_pred_fpn3_b" in grad_map
    with pytest.raises(rh.SoftmaxDistillError):
        rh.add_distill_loss(model)


def test_softmax_builder_test_graph():
    cfg = rh.HeadConfig(softmax=True, num_convs=1)
    model, preds = _build(cfg, False)
    ops = list(model.net.Proto().op)
    sm = [op for op in ops if op.type == "GroupSpatialSoftmax"]
    assert not [op for op in ops if op.type == "Sigmoid"]
    assert [list(op.input) + list(op.output) for op in sm] == [
        ["retnet_cls_pred_fpn%d" % l, "retnet_cls_prob_fpn%d" % l] for l in cfg.levels()]
    assert all(_args(op) == {"num_classes": cfg.num_classes} for op in sm)
    # each level's softmax follows that level's cls_pred convolution directly, where the Sigmoid sits otherwise
    ref_model, _ = _build(rh.HeadConfig(num_convs=1), False)
    assert [op.type.replace("GroupSpatialSoftmax", "Sigmoid") for op in ops] == \
        [op.type for op in ref_model.net.Proto().op]
    # the gradient maker of the inference op: (Y, dY) -> dX
    net_ = core.Net("g")
    y = net_.GroupSpatialSoftmax("x", "y", num_classes=5)
    gm = net_.AddGradientOperators({y: "y_grad_in"})
    g = list(net_.Proto().op)[-1]
    assert g.type == "GroupSpatialSoftmaxGradient" and list(g.input) == ["y", "y_grad_in"]
    assert list(g.output) == [gm["x"]] and _args(g) == {"num_classes": 5}


@pytest.mark.parametrize("train", [True, False])
def test_softmax_false_is_todays_graph(train):
    def serialized(cfg):
        model, _ = _build(cfg, train)
        if train:
            grads = rh.add_fpn_retinanet_losses(model)
            grads.update(rh.add_distill_loss(model))
            model.net.AddGradientOperators(grads)
        return [op.SerializeToString() for op in model.net.Proto().op], model.params, model.losses

    a = serialized(rh.HeadConfig())
    b = serialized(rh.HeadConfig(softmax=False))
    assert a[0] == b[0] and len(a[0]) > 40
    assert repr(a[1]) == repr(b[1]) and a[2] == b[2]
    types = {core.caffe2_pb2.OperatorDef().ParseFromString(s).type for s in a[0]}
    assert "SigmoidFocalLoss" in types or not train
    assert not types & {"SoftmaxFocalLoss", "GroupSpatialSoftmax"}


# ---------------------------------------------------------------------------
# detector arguments (checked before the library is touched)
# ---------------------------------------------------------------------------

def test_detector_softmax_argument_checks():
    assert RetinanetDetector._softmax_args(False, False) is False
    assert RetinanetDetector._softmax_args(True, False) is True
    assert RetinanetDetector._softmax_args(True, True) is True
    with pytest.raises(K.KernelError, match="softmax=True"):
        RetinanetDetector._softmax_args(False, True)
    with pytest.raises(K.KernelError):
        RetinanetDetector._softmax_args("yes", False)
    with pytest.raises(K.KernelError):
        RetinanetDetector._softmax_args(True, 1)


# ---------------------------------------------------------------------------
# weights file
# ---------------------------------------------------------------------------

def test_softmax_head_weights_file_round_trip(tmp_path):
    cfg = rh.HeadConfig(softmax=True, num_convs=1)
    A, C = cfg.num_anchors, cfg.num_classes
    bad_name = "retnet_cls_pred_fpn3_w"
    st = net.HeadParamStore(cfg)
    assert tuple(st.params["retnet_cls_pred_fpn3_w"].shape) == (A * C, 256, 3, 3)
    assert st.fillers["retnet_cls_pred_fpn3_b"][0] == "GivenTensorFill"
    st.fill(seed=3)
    b = st.params["retnet_cls_pred_fpn3_b"].numpy().reshape(A, C)
    assert np.all(b[:, 1:] == 0) and np.all(b[:, 0] == np.float32(np.log((C - 1) * 99.0)))
    assert abs(float(st.params[bad_name].std()) - 0.01) < 1e-3 and not st.params["retnet_bbox_pred_fpn3_b"].any()
    st = net.HeadParamStore(cfg)
    rng = np.random.default_rng(7)
    blobs = {}
    for name, shape, _, _ in st.params.specs:
        blobs[name] = rng.standard_normal(shape).astype(np.float32)
        blobs[name + "_momentum"] = rng.standard_normal(shape).astype(np.float32)
    blobs["conv1_w"] = rng.standard_normal((64, 3, 7, 7)).astype(np.float32)
    path = str(tmp_path / "softmax_head.pkl")
    with open(path, "wb") as f:
        pickle.dump(dict(blobs=blobs, cfg=""), f, protocol=2)

    bad = "retnet_cls_pred_fpn3_w"
    # told nothing: a softmax-shaped cls_pred is rejected, as it is by a sigmoid head's store
    loaded, missing = net.initialize_from_weights_file(st, path)
    assert not missing and bad not in loaded and "retnet_cls_pred_fpn3_b" not in loaded
    assert float(st.params[bad].abs().sum()) == 0.0 and float(st.moms[bad].abs().sum()) == 0.0
    assert "retnet_bbox_pred_fpn3_w" in loaded
    # told the head is softmax
    st = net.HeadParamStore(cfg)
    loaded, missing = net.initialize_from_weights_file(st, path, softmax=True)
    assert not missing and sorted(loaded) == sorted(n for n, _, _, _ in st.params.specs)
    for name, _, _, _ in st.params.specs:
        assert np.array_equal(st.params[name].numpy(), blobs[name])
        assert np.array_equal(st.moms[name].numpy(), blobs[name + "_momentum"])
    assert list(st.preserved) == ["conv1_w"]
    out = str(tmp_path / "saved.pkl")
    net.save_model_to_weights_file(out, st)
    saved = pickle.load(open(out, "rb"))["blobs"]
    assert set(saved) == set(blobs)
    for k, v in blobs.items():
        assert np.array_equal(saved[k], v), k
    # a sigmoid store cannot be told it is softmax, and still skips the softmax-shaped blob
    sig = net.HeadParamStore(rh.HeadConfig(num_convs=1))
    assert tuple(sig.params[bad].shape) == (A * (C - 1), 256, 3, 3)
    with pytest.raises(ValueError):
        net.initialize_from_weights_file(sig, path, softmax=True)
    loaded, _ = net.initialize_from_weights_file(sig, path)
    assert bad not in loaded and float(sig.params[bad].abs().sum()) == 0.0
