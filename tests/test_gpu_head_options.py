"""RETINANET.SHARE_CLS_BBOX_TOWER and RETINANET.CLASS_SPECIFIC_BBOX on the device.

1. The subnet step (head_pipeline.DistillHeads) with either switch, both, a softmax head and a thin student, against
   a float64 torch-autograd composition written here: the towers as torch convolutions, the loss formulas restated
   from oracle/ssad_oracle.c (SigmoidFocalLoss, SelectSmoothL1Loss, PowSum + SigmoidAdaptiveDistillLoss) and, for
   the softmax head, from softmax_focal_loss_op.cu as tests/test_gpu_softmax_step.py restates it.  Every loss at
   LOSS_RTOL, every parameter gradient and the gradient w.r.t. the FPN levels per element at CONV_RTOL / CONV_FLOOR
   (tests/test_gpu_kernels.py), on a problem whose tower biases keep every pre-activation of the reference at least
   1e-2 of its layer's range from zero (far above the 1e-5 the engines' round-off could move it), so no ReLU mask
   can differ; the masks are counted all the same and a seed with a flipped one is skipped, never excused.
2. The class-specific labeller bit for bit against the reference's own Python
   (tests/golden/anchor_labels_class_specific_ref.npz).
3. The class-specific detector against a numpy restatement of core/test_retinanet.py:108-206 whose box deltas are
   indexed the way the training loss addresses them (UNPINNED by the reference: DESIGN.md).
4. Both new entry points in a guarded arena (tests/guarded.py).
5. The builder's net with both switches through CreateNet / RunNet against the native program.

The tests print the figures they assert on."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

import ssad_amd  # noqa: E402,F401
from oracle import anchors as OA  # noqa: E402
from oracle import detect as OD  # noqa: E402
from ssad_amd import kernels as K_  # noqa: E402
from ssad_amd.caffe2_hip import caffe2_pb2, core, dyndep, workspace  # noqa: E402
from ssad_amd.head_pipeline import DistillHeads, head_param_specs, head_towers  # noqa: E402
from ssad_amd.modeling import retinanet_heads as rh  # noqa: E402
from ssad_amd.modeling.generate_anchors import AnchorConfig, cell_anchors  # noqa: E402
from test_anchor_labels import DETECT_BOX_TOL  # noqa: E402
from test_gpu_isolation_detect import arena_run, p, past, same  # noqa: E402
from test_gpu_kernels import CONV_FLOOR, CONV_RTOL, LOSS_RTOL, close  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GPU = core.DeviceOption(caffe2_pb2.CUDA, 0)
FLT_MIN = float(np.finfo(np.float32).tiny)
SHAPES = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]
I32 = torch.int32


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    K_.lib()
    return K_


# ---------------------------------------------------------------------------
# the problem and its float64 reference
# ---------------------------------------------------------------------------

def t64(a):
    return torch.from_numpy(np.asarray(a)).to(torch.float64)


def tower_names(cfg, tower):
    return ["retnet_%s_conv_n%d_fpn%d" % (tower, i, cfg.k_min) for i in range(cfg.num_convs)]


def make_params(rng, cfg, dim):
    S = {}
    for name, shape, is_bias, _ in head_param_specs(dataclasses.replace(cfg, fpn_dim=dim)):
        S[name] = np.zeros(shape, np.float32) if is_bias else (rng.standard_normal(shape) * 0.03).astype(np.float32)
    cp = "retnet_cls_pred_fpn%d_b" % cfg.k_min
    if cfg.softmax:
        S[cp] = (np.asarray(rh.retinanet_bias_init(cfg)[1]["values"], np.float32).reshape(-1) * 0.25)
    else:
        S[cp][:] = -1.0
    return S


def mask_safe(cfg, S, fs):
    """tests/test_gpu_operators.make_mask_safe for the towers this head owns, in float64: per layer and output channel
    a bias of +-1.5 x max|conv output|, the layer rescaled to O(1) activations.  -> the smallest |pre-activation|
    as a fraction of its layer's range."""
    margin = np.inf
    for tower in head_towers(cfg):
        xs = [t64(f) for f in fs]
        for name in tower_names(cfg, tower):
            w = t64(S[name + "_w"])
            zs = [F.conv2d(x, w, None, padding=1) for x in xs]
            top = torch.stack([z.abs().amax(dim=(0, 2, 3)) for z in zs]).amax(0)
            sign = 1.0 - 2.0 * (torch.arange(top.numel()) % 2).to(torch.float64)
            b = (1.5 * top * sign).to(torch.float32).to(torch.float64)
            pre = [z + b.view(1, -1, 1, 1) for z in zs]
            k = np.float32(2.0 / max(float(q.abs().max()) for q in pre))
            S[name + "_w"] = (S[name + "_w"] * k).astype(np.float32)
            S[name + "_b"] = (b.numpy() * k).astype(np.float32)
            # the pre-activations of the parameters as stored (fp32 values, float64 arithmetic)
            w2, b2 = t64(S[name + "_w"]), t64(S[name + "_b"])
            pre = [F.conv2d(x, w2, b2, padding=1) for x in xs]
            margin = min(margin, min(float(q.abs().min() / q.abs().max()) for q in pre))
            xs = [q.clamp_min(0).to(torch.float32).to(torch.float64) for q in pre]
    return margin


def make_labels(rng, cfg, N, shapes):
    labs = []
    A, nfg = cfg.num_anchors, cfg.num_classes - 1
    for h, w in shapes:
        u = rng.random((N, A, h, w))
        lab = np.zeros((N, A, h, w), np.int32)
        lab[u < 0.05] = -1
        fg = u > 0.88
        lab[fg] = rng.integers(1, nfg + 1, size=int(fg.sum()))
        flat = lab.reshape(-1)
        need = 8 - int((flat > 0).sum())
        if need > 0:                                       # at least 8 foreground rows wherever the level has room
            idx = rng.choice(np.nonzero(flat <= 0)[0], size=need, replace=False)
            flat[idx] = rng.integers(1, nfg + 1, size=need)
        labs.append(lab)
    return labs


def make_targets(rng, cfg, lab):
    """SelectSmoothL1Loss rows of one level: (n, channel, y, x) with the channel the labeller writes -- 4 * anchor, or
    4 * (label - 1) + 4 * (num_classes - 1) * anchor for a class-specific head -- and targets of order 1."""
    n, a, y, x = np.nonzero(lab > 0)
    ch = 4 * a
    if cfg.class_specific_bbox:
        ch = 4 * (lab[n, a, y, x] - 1) + 4 * (cfg.num_classes - 1) * a
    L = np.stack([n, ch, y, x], axis=1).astype(np.float32)
    Y = rng.standard_normal((L.shape[0], 4)).astype(np.float32)
    return Y, L


def make_problem(kw, distill, seed, shapes=SHAPES, N=2, teacher_dim=None):
    rng = np.random.default_rng(seed)
    cfg = rh.HeadConfig(num_gpus=1, **kw)
    dim, tdim = cfg.fpn_dim, teacher_dim or cfg.fpn_dim
    S = make_params(rng, cfg, dim)
    fs = [rng.standard_normal((N, dim, h, w)).astype(np.float32) for h, w in shapes]
    margin = mask_safe(cfg, S, fs)
    T = ft = None
    if distill:
        T = make_params(rng, cfg, tdim)
        ft = [rng.standard_normal((N, tdim, h, w)).astype(np.float32) for h, w in shapes]
        mask_safe(cfg, T, ft)
    labs = make_labels(rng, cfg, N, shapes)
    tg = [make_targets(rng, cfg, lab) for lab in labs]
    fg = np.array([float(sum(t[0].shape[0] for t in tg))], np.float32)
    return dict(cfg=cfg, S=S, T=T, fs=fs, ft=ft, labs=labs, tg=tg, fg=fg, margin=margin, distill=distill, tdim=tdim)


def class_masks(lab, A, Cn):
    """(positive, negative) masks [N][A*Cn][H][W] of SigmoidFocalLoss and the label per element."""
    N, _, H, W = lab.shape
    t = torch.from_numpy(lab).view(N, A, 1, H, W).expand(N, A, Cn, H, W)
    d = torch.arange(Cn).view(1, 1, Cn, 1, 1)
    pos = (t == d + 1)
    neg = (t != -1) & ~pos
    return pos.reshape(N, A * Cn, H, W), neg.reshape(N, A * Cn, H, W), t.reshape(N, A * Cn, H, W)


def reference(pb, drop_bbox_from_shared=False):
    """One step in float64 with torch autograd.  -> losses, {param: grad}, {tower: [d_fpn per level]}, tower
    activations {tower: [depth][level]}, the predictions."""
    cfg, S = pb["cfg"], pb["S"]
    towers = head_towers(cfg)
    A, nl = cfg.num_anchors, len(pb["fs"])
    P = {k: t64(v).requires_grad_() for k, v in S.items()}
    xin = {t: [t64(f).requires_grad_() for f in pb["fs"]] for t in towers}
    acts, feat = {}, {}
    for t in towers:
        xs, acts[t] = xin[t], []
        for name in tower_names(cfg, t):
            xs = [F.relu(F.conv2d(x, P[name + "_w"], P[name + "_b"], padding=1)) for x in xs]
            acts[t].append(xs)
        feat[t] = xs
    cp, bp = "retnet_cls_pred_fpn%d" % cfg.k_min, "retnet_bbox_pred_fpn%d" % cfg.k_min
    logits = [F.conv2d(x, P[cp + "_w"], P[cp + "_b"], padding=1) for x in feat["cls"]]
    bfeat = feat[towers[-1]]
    if drop_bbox_from_shared:
        bfeat = [x.detach() for x in bfeat]
    bbox = [F.conv2d(x, P[bp + "_w"], P[bp + "_b"], padding=1) for x in bfeat]
    fgn = max(float(pb["fg"][0]), 1.0)
    scale = cfg.loss_scale
    out = dict(distill=[], focal=[], bbox=[])
    total = 0.0
    t_prob = None
    if pb["distill"]:
        T = {k: t64(v) for k, v in pb["T"].items()}
        xs = [t64(f) for f in pb["ft"]]
        for name in tower_names(cfg, "cls"):
            xs = [F.relu(F.conv2d(x, T[name + "_w"], T[name + "_b"], padding=1)) for x in xs]
        t_prob = [torch.sigmoid(F.conv2d(x, T[cp + "_w"], T[cp + "_b"], padding=1)) for x in xs]
        out["t_bbox"] = [F.conv2d(x, T[bp + "_w"], T[bp + "_b"], padding=1) for x in
                         (xs if cfg.share_cls_bbox_tower else teacher_bbox_feat(cfg, T, pb["ft"]))]
        norm = sum((q ** cfg.logits_power).sum() for q in t_prob)
        out["normalizer"] = float(norm)
        Np = max(float(norm), 1.0)
    Cn = cfg.num_classes if cfg.softmax else cfg.num_classes - 1
    for l in range(nl):
        x, lab = logits[l], pb["labs"][l]
        if cfg.softmax:
            N, _, H, W = x.shape
            g = torch.from_numpy(lab).to(torch.int64)
            lp = F.log_softmax(x.view(N, A, Cn, H, W), dim=2)
            lpt = torch.gather(lp, 2, g.clamp_min(0).unsqueeze(2)).squeeze(2)
            pt = lpt.exp()
            zw = ((g > 0).to(torch.float64) * cfg.focal_alpha + (g == 0).to(torch.float64) * (1.0 - cfg.focal_alpha)) / fgn
            loss = scale * (-zw * (1.0 - pt) ** cfg.focal_gamma * torch.log(pt.clamp_min(FLT_MIN))).sum()
        else:
            pos, neg, t = class_masks(lab, A, Cn)
            logp, log1mp = F.logsigmoid(x), F.logsigmoid(-x)
            prob = torch.sigmoid(x)
            loss = scale * (-(pos * (1 - prob) ** cfg.focal_gamma * logp) * (cfg.focal_alpha / fgn)
                            - (neg * prob ** cfg.focal_gamma * log1mp) * ((1 - cfg.focal_alpha) / fgn)).sum()
            if pb["distill"]:
                q = t_prob[l]
                DL = -(q * logp + (1 - q) * log1mp)                       # + beta * entropy(q), beta = 0
                AT = 1.0 - torch.exp(-DL)
                ce = q * logp * (cfg.distill_alpha / Np) + (1 - q) * log1mp * ((1 - cfg.distill_alpha) / Np)
                dl = (scale * cfg.temperature ** 2) * (-(AT ** cfg.distill_gamma) * ce * (t != cfg.ignored_label)).sum()
                out["distill"].append(float(dl.detach()))
                total = total + dl
        out["focal"].append(float(loss.detach()))
        total = total + loss
        Y, L = pb["tg"][l]
        if Y.shape[0]:
            n, c, y, xx = [torch.from_numpy(L[:, k].astype(np.int64)) for k in range(4)]
            val = torch.stack([bbox[l][n, c + j, y, xx] for j in range(4)], dim=1) - t64(Y)
            a = val.abs()
            beta = cfg.bbox_reg_beta
            bl = (scale * cfg.bbox_reg_weight) * (torch.where(a < beta, 0.5 * val * val / beta, a - 0.5 * beta) / fgn).sum()
            total = total + bl
            out["bbox"].append(float(bl.detach()))
        else:
            out["bbox"].append(0.0)
    total.backward()
    grads = {k: v.grad.numpy() for k, v in P.items()}
    d_fpn = {t: [x.grad.numpy() for x in xin[t]] for t in towers}
    A_ = {t: [[a.detach().numpy() for a in lev] for lev in acts[t]] for t in towers}
    return dict(losses=out, grads=grads, d_fpn=d_fpn, acts=A_, logits=[x.detach().numpy() for x in logits],
                bbox=[x.detach().numpy() for x in bbox])


def teacher_bbox_feat(cfg, T, ft):
    xs = [t64(f) for f in ft]
    for name in tower_names(cfg, "bbox"):
        xs = [F.relu(F.conv2d(x, T[name + "_w"], T[name + "_b"], padding=1)) for x in xs]
    return xs


_CASES = {}


def case(key, kw, distill, shapes=SHAPES, N=2, teacher_dim=None, seeds=(7001, 7002, 7003), **heads_kw):
    """The problem, its reference and the native heads after one step without the update; computed once per key and
    left unchanged.  A seed whose native run has a tower activation on the other side of zero is skipped."""
    if key in _CASES:
        return _CASES[key]
    dev = torch.device("cuda", 0)
    to = lambda arrs: [torch.from_numpy(a).to(dev) for a in arrs]     # noqa: E731
    for seed in seeds:
        pb = make_problem(kw, distill, seed, shapes, N, teacher_dim)
        assert pb["margin"] > 1e-2, pb["margin"]     # no reference pre-activation within 1e-5 of zero, by a wide margin
        ref = reference(pb)
        heads = DistillHeads(pb["cfg"], N=N, shapes=shapes, device=dev, student_init=pb["S"], teacher_init=pb["T"],
                             distill=distill, teacher_fpn_dim=teacher_dim, **heads_kw)
        heads.step(to(pb["fs"]), to(pb["ft"]) if distill else None, to(pb["labs"]), update=False,
                   bbox_targets=[tuple(to(t)) for t in pb["tg"]], fg_num=torch.from_numpy(pb["fg"]).to(dev))
        torch.cuda.synchronize()
        flips = sum(int(((heads.act[t][d][l].cpu().numpy() > 0) != (a > 0)).sum())
                    for t, per_depth in ref["acts"].items() for d, per_level in enumerate(per_depth)
                    for l, a in enumerate(per_level))
        print("%s: seed %d, margin %.3e, flipped activations %d" % (key, seed, pb["margin"], flips))
        if flips == 0:
            _CASES[key] = dict(pb=pb, ref=ref, heads=heads)
            return _CASES[key]
    raise AssertionError("%s: every seed has a flipped ReLU mask" % key)


def worst(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    lim = CONV_RTOL * np.abs(ref) + CONV_FLOOR * np.abs(ref).max()
    return float((np.abs(got - ref) / np.maximum(lim, 1e-300)).max())


def check_step(key, c):
    pb, ref, heads = c["pb"], c["ref"], c["heads"]
    L = ref["losses"]
    got_focal, got_bbox = heads.focal_losses.cpu().numpy(), heads.bbox_losses.cpu().numpy()
    print("%s: focal %s | %s" % (key, got_focal, np.array(L["focal"])))
    print("%s: bbox  %s | %s" % (key, got_bbox, np.array(L["bbox"])))
    assert min(L["bbox"][:4]) > 1e-3 and min(L["focal"]) > 0          # the box loss is not negligible
    close(got_focal, L["focal"], LOSS_RTOL, 0, "focal losses")
    close(got_bbox, L["bbox"], LOSS_RTOL, 1e-9, "bbox losses")
    if pb["distill"]:
        print("%s: distill %s | %s" % (key, heads.losses.cpu().numpy(), np.array(L["distill"])))
        close(float(heads.normalizer[0]), L["normalizer"], 1e-5, 0, "normalizer")
        close(heads.losses.cpu().numpy(), L["distill"], LOSS_RTOL, 0, "distill losses")
    for l in range(len(ref["logits"])):
        close(heads.cls_logits[l].cpu().numpy(), ref["logits"][l], CONV_RTOL, CONV_FLOOR, "cls_pred %d" % l)
        close(heads.bbox_pred[l].cpu().numpy(), ref["bbox"][l], CONV_RTOL, CONV_FLOOR, "bbox_pred %d" % l)
    assert sorted(ref["grads"]) == sorted(n for n, _, _, _ in heads.params.specs)
    figures = {n: worst(heads.grads[n].cpu().numpy(), g) for n, g in ref["grads"].items()}
    for t, per_level in ref["d_fpn"].items():
        for l, g in enumerate(per_level):
            figures["d_fpn %s %d" % (t, l)] = worst(heads.d_fpn[t][l].cpu().numpy(), g)
    print("%s: worst error / limit: %s" % (key, {k: round(v, 3) for k, v in figures.items()}))
    for n, g in ref["grads"].items():
        assert np.abs(g).max() > 0, n
        close(heads.grads[n].cpu().numpy(), g, CONV_RTOL, CONV_FLOOR, "grad " + n)
    assert sorted(heads.d_fpn) == sorted(ref["d_fpn"])
    for t, per_level in ref["d_fpn"].items():
        for l, g in enumerate(per_level):
            close(heads.d_fpn[t][l].cpu().numpy(), g, CONV_RTOL, CONV_FLOOR, "d_fpn %s %d" % (t, l))


# ---------------------------------------------------------------------------
# 1. the subnet step
# ---------------------------------------------------------------------------

SHARED = dict(num_classes=4, share_cls_bbox_tower=True)
SPECIFIC = dict(num_classes=4, class_specific_bbox=True)


@pytest.mark.parametrize("distill", [True, False], ids=["distill", "student_only"])
def test_shared_tower_step(distill):
    key = "shared/%s" % distill
    c = case(key, SHARED, distill)
    assert list(c["heads"].d_fpn) == ["cls"] and len(c["heads"].params.specs) == 12
    check_step(key, c)
    # the last tower filter's gradient is the one obtained from the SUM of both heads: against a reference that
    # drops bbox_pred's contribution to the shared activation the same comparison fails
    dropped = reference(c["pb"], drop_bbox_from_shared=True)
    name = "retnet_cls_conv_n3_fpn3_w"
    got = c["heads"].grads[name].cpu().numpy()
    print("%s: %s against the reference without bbox_pred's part: error / limit %.1f" % (key, name, worst(got, dropped["grads"][name])))
    with pytest.raises(AssertionError):
        close(got, dropped["grads"][name], CONV_RTOL, CONV_FLOOR, "dropped")
    with pytest.raises(AssertionError):
        close(c["heads"].d_fpn["cls"][0].cpu().numpy(), dropped["d_fpn"]["cls"][0], CONV_RTOL, CONV_FLOOR, "dropped")


@pytest.mark.parametrize("distill", [True, False], ids=["distill", "student_only"])
def test_accumulate_epilogue_equals_the_two_pass_form(distill):
    """Bit-identical, every parameter gradient and the gradient w.r.t. the FPN levels.  Why: the epilogue adds what y
    held (cls_pred's data gradient, fp32) to this lane's inverse-transformed outputs AFTER they exist as fp32 values --
    the same two fp32 numbers the two-pass form stores and SUM_N adds, one rounding, and fp32 addition commutes; the
    mask picks the sum or +0 in both.  Everything downstream reads the same bits (the split engines' |max| word of the
    sum is measured after the last writer in both forms)."""
    acc = case("shared/%s" % distill, SHARED, distill)
    two = case("shared/two_pass/%s" % distill, SHARED, distill, shared_accumulate=False)
    assert acc["heads"].shared_form == "accumulate" and two["heads"].shared_form == "two_pass"
    check_step("shared/two_pass/%s" % distill, two)
    for l in range(len(SHAPES)):
        assert torch.equal(acc["heads"].dbuf["cls"][4][l], two["heads"].dbuf["cls"][4][l]), "shared gradient, level %d" % l
        assert torch.equal(acc["heads"].d_fpn["cls"][l], two["heads"].d_fpn["cls"][l]), "d_fpn level %d" % l
    assert float(acc["heads"].dbuf["cls"][4][0].abs().max()) > 0
    for name, _, _, _ in acc["heads"].params.specs:
        assert torch.equal(acc["heads"].grads[name], two["heads"].grads[name]), name


def test_both_switches_step_81_classes_one_level():
    """Shared tower with the 2880-wide bbox_pred: its data gradient runs on the split-operand engine, unmasked into
    its own buffer, and the two-pass form sums it with cls_pred's."""
    kw = dict(num_classes=81, share_cls_bbox_tower=True, class_specific_bbox=True, k_min=3, k_max=3)
    c = case("both/81", kw, False, shapes=[(8, 12)], N=1)
    h = c["heads"]
    assert h.shared_form == ("two_pass" if h.dgrad_engine["retnet_bbox_pred_fpn3"].name != "F24" else "accumulate")
    assert tuple(h.bbox_pred[0].shape) == (1, 2880, 8, 12) and list(h.d_fpn) == ["cls"]
    check_step("both/81", c)


@pytest.mark.parametrize("distill", [True, False], ids=["distill", "student_only"])
def test_class_specific_step(distill):
    key = "class_specific/%s" % distill
    c = case(key, SPECIFIC, distill)
    assert tuple(c["heads"].bbox_pred[0].shape) == (2, 108, 16, 24)
    locs = np.concatenate([t[1][:, 1] for t in c["pb"]["tg"]]).astype(int)
    assert {(ch % 12) // 4 for ch in locs} == {0, 1, 2}                  # every class's box is addressed
    check_step(key, c)


def test_both_switches_step():
    c = case("both", dict(num_classes=4, share_cls_bbox_tower=True, class_specific_bbox=True), True)
    assert list(c["heads"].d_fpn) == ["cls"] and tuple(c["heads"].bbox_pred[0].shape) == (2, 108, 16, 24)
    check_step("both", c)


def test_shared_tower_softmax_step():
    c = case("shared/softmax", dict(num_classes=4, share_cls_bbox_tower=True, softmax=True), False)
    assert tuple(c["heads"].cls_logits[0].shape) == (2, 36, 16, 24)
    check_step("shared/softmax", c)


def test_shared_tower_thin_student_step():
    """teacher_fpn_dim != fpn_dim: a half-width student under a full-width teacher, both with a shared tower"""
    c = case("shared/thin", dict(num_classes=4, share_cls_bbox_tower=True, fpn_dim=128), True, teacher_dim=256)
    h = c["heads"]
    assert h.D == 128 and h.Dt == 256 and tuple(h.teacher["retnet_cls_conv_n0_fpn3_w"].shape) == (256, 256, 3, 3)
    check_step("shared/thin", c)


def test_class_specific_step_81_classes_one_level():
    """2880 outputs: forward, data gradient and filter gradient on the engine the rule chose (the split-operand
    engine under the default switches); the teacher's bbox_pred shares the launch."""
    from ssad_amd.engines import Engine
    kw = dict(num_classes=81, class_specific_bbox=True, k_min=3, k_max=3)
    c = case("class_specific/81", kw, True, shapes=[(8, 12)], N=1)
    h = c["heads"]
    name = "retnet_bbox_pred_fpn3"
    print("class_specific/81: engines fwd %s dgrad %s" % (h.fwd_engine["student", name].name, h.dgrad_engine[name].name))
    assert tuple(h.bbox_pred[0].shape) == (1, 2880, 8, 12) and tuple(h.grads[name + "_w"].shape) == (2880, 256, 3, 3)
    if h.switches.split_conv & 3 == 3:
        assert h.fwd_engine["student", name] == h.fwd_engine["teacher", name] == h.dgrad_engine[name] == Engine.SPLIT
    check_step("class_specific/81", c)
    close(h.t_bbox[0].cpu().numpy(), c["ref"]["losses"]["t_bbox"][0].numpy(), CONV_RTOL, CONV_FLOOR, "teacher bbox_pred")


def test_native_model_feeds_the_backbone_from_the_one_tower():
    """NativeDistillModel over shared-tower heads: the gradient the student's backbone starts from is d_fpn["cls"]
    alone (a one-term record where separate towers are summed), and the whole model trains."""
    from ssad_amd.backbone_pipeline import NativeDistillModel
    N, HW = 1, (128, 128)
    shapes = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    pb = make_problem(dict(share_cls_bbox_tower=True), False, 7301, shapes=shapes, N=N)
    to = lambda a: torch.from_numpy(a).cuda()                     # noqa: E731
    labels, targets, fg_num = [to(a) for a in pb["labs"]], [(to(y), to(l)) for y, l in pb["tg"]], to(pb["fg"])
    images = torch.randn((N, 3) + HW, device="cuda", generator=torch.Generator(device="cuda").manual_seed(73))
    heads = DistillHeads(pb["cfg"], N=N, shapes=shapes, device="cuda", student_init=pb["S"], distill=False, lr=1e-3)
    model = NativeDistillModel(heads, "r50", None, N, HW, "cuda", lr=1e-3)
    assert [o.i[0] for o in model.sum_prog.ops] == [1] * 5 and list(heads.d_fpn) == ["cls"]
    p0, b0 = heads.params.flat.clone(), model.student.params_flat.clone()
    model.step(images, labels, targets, fg_num)
    torch.cuda.synchronize()
    # the one-term record is a copy (the backbone's backward has since written into its own buffers: run it again)
    model.sum_prog.run()
    torch.cuda.synchronize()
    for a, d in zip(heads.d_fpn["cls"], model.student.d_fpn):
        assert torch.equal(a, d) and float(a.abs().max()) > 0
    assert bool(torch.isfinite(heads.focal_losses).all()) and float(heads.bbox_losses.sum()) > 0
    assert bool(torch.isfinite(heads.params.flat).all()) and not torch.equal(heads.params.flat, p0)
    assert bool(torch.isfinite(model.student.params_flat).all()) and not torch.equal(model.student.params_flat, b0)


# ---------------------------------------------------------------------------
# 2. the labeller
# ---------------------------------------------------------------------------

def label_fixture():
    z = np.load(os.path.join(HERE, "golden", "anchor_labels_class_specific_ref.npz"))
    H, W = [int(v) for v in z["image_hw"]]
    gts = [(z["gt_boxes_%d" % i] * np.float32(z["scales"][i]), z["gt_classes_%d" % i]) for i in range(2)]
    Gmax = max(len(c) for _, c in gts)
    boxes, classes = np.zeros((2, Gmax, 4), np.float32), np.zeros((2, Gmax), np.int32)
    for i, (b, c) in enumerate(gts):
        boxes[i, :len(c)], classes[i, :len(c)] = b, c
    return z, H, W, Gmax, boxes, classes, np.array([len(c) for _, c in gts], np.int32)


def run_labeller(class_specific):
    from ssad_amd.roi_data.retinanet import RetinanetLabeler
    z, H, W, Gmax, boxes, classes, counts = label_fixture()
    lab = RetinanetLabeler(2, Gmax, H, W, class_specific_bbox=class_specific)
    blobs = lab(torch.as_tensor(boxes).cuda(), torch.as_tensor(classes).cuda(), torch.as_tensor(counts).cuda())
    return z, {k: v.cpu().numpy() for k, v in blobs.items()}


def test_class_specific_labeller_matches_the_reference_fixture():
    z, got = run_labeller(True)
    assert np.array_equal(got["retnet_fg_num"], z["blob_retnet_fg_num"].reshape(-1))
    assert np.array_equal(got["retnet_bg_num"], z["blob_retnet_bg_num"].reshape(-1))
    for lvl in range(3, 8):
        assert np.array_equal(got["retnet_cls_labels_fpn%d" % lvl], z["blob_retnet_cls_labels_fpn%d" % lvl]), lvl
        locs = got["retnet_roi_fg_bbox_locs_fpn%d" % lvl]
        assert locs.dtype == np.float32 and np.array_equal(locs, z["blob_retnet_roi_fg_bbox_locs_fpn%d" % lvl]), lvl
    # the switch changes column 1 and nothing else
    _, plain = run_labeller(False)
    offsets = set()
    for k in got:
        if "fg_bbox_locs" in k:
            assert np.array_equal(plain[k][:, [0, 2, 3]], got[k][:, [0, 2, 3]])
            assert np.array_equal(plain[k][:, 1], 4 * (got[k][:, 1] // 320))
            offsets |= set((got[k][:, 1] % 320).astype(int).tolist())
        else:
            assert np.array_equal(plain[k], got[k]), k
    assert {0, 4 * 79} <= offsets and len(offsets) > 2          # class 1, class 80 and classes in between


def test_class_specific_labeller_targets_are_unchanged():
    """The switch does not touch the regression targets: bit-identical to the class-agnostic labeller's on the same
    ground truth (test_class_specific_labeller_matches_the_reference_fixture), and against the reference fixture at
    the class-agnostic labeller's own bar, TARGET_TOL of tests/test_anchor_labels.py (the device's logf against
    numpy's float32 log)."""
    from test_anchor_labels import TARGET_TOL
    z, got = run_labeller(True)
    for lvl in range(3, 8):
        tg, ref = got["retnet_roi_bbox_targets_fpn%d" % lvl], z["blob_retnet_roi_bbox_targets_fpn%d" % lvl]
        assert tg.shape == ref.shape and tg.dtype == ref.dtype
        if tg.size:
            ulp = np.abs(tg.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64)).max(axis=0)
            print("targets level %d: %d rows, max difference per column %s ulp" % (lvl, tg.shape[0], ulp.tolist()))
        np.testing.assert_allclose(tg, ref, **TARGET_TOL)


# ---------------------------------------------------------------------------
# 3. the detector
# ---------------------------------------------------------------------------

class Cfg4(AnchorConfig):
    num_classes = 4


DET_SHAPES = [(10, 14), (5, 7), (3, 4)]
DET_A, DET_C = 9, 3
DET_IM = (80, 112)


def det_inputs(seed=7100):
    """Scores: distinct multiples of 2^-12 per level (ties are unspecified in the reference).  Deltas: every class's
    box of an anchor is moved by 0.9 anchor widths from the previous class's -- an overlap of at most 0.1 / 1.9, far
    below the NMS threshold and far above DETECT_BOX_TOL."""
    rng = np.random.default_rng(seed)
    probs, deltas = [], []
    for h, w in DET_SHAPES:
        n = DET_A * DET_C * h * w
        vals = (rng.permutation(n) + 1).astype(np.float64) * 2.0 ** -12
        probs.append(vals.astype(np.float32).reshape(1, DET_A * DET_C, h, w))
        d = (rng.standard_normal((1, DET_A, DET_C, 4, h, w)) * 0.1).astype(np.float32)
        d[:, :, :, 0] += (0.9 * np.arange(DET_C, dtype=np.float32)).reshape(1, 1, DET_C, 1, 1) - 0.9
        deltas.append(np.ascontiguousarray(d.reshape(1, DET_A * DET_C * 4, h, w)))
    return probs, deltas


def detect_restated(probs, deltas, cells, im_shape, scale, k_min=3, inference_th=0.05, pre_nms_topn=1000, nms_thresh=0.5,
                    dets_per_im=100):
    """core/test_retinanet.py:108-206 as oracle/detect.py restates it, with :151-158 for a class-specific head: the
    four deltas of candidate (a, c, y, x) are channels a*4*C + 4*c + k.  -> (detections, candidates [lvl a c y x box])"""
    k_max = k_min + len(probs) - 1
    boxes_all, cands = {}, []
    for li, lvl in enumerate(range(k_min, k_max + 1)):
        stride = 2. ** lvl
        ca = cells[li]
        A = ca.shape[0]
        cls_prob = probs[li]
        Cn = cls_prob.shape[1] // A
        cls_prob = cls_prob.reshape(1, A, Cn, cls_prob.shape[2], cls_prob.shape[3])
        box_pred = deltas[li].reshape(1, A, Cn, 4, deltas[li].shape[2], deltas[li].shape[3])
        ravel = cls_prob.ravel()
        cand = np.where(ravel > (inference_th if lvl < k_max else 0.0))[0]
        if len(cand) == 0:
            continue
        k = min(pre_nms_topn, len(cand))
        inds = cand[np.argpartition(ravel[cand], -k)[-k:]]
        i5 = np.array(np.unravel_index(inds, cls_prob.shape)).transpose()
        classes, a_ids, y, x = i5[:, 2], i5[:, 1], i5[:, 3], i5[:, 4]
        scores = cls_prob[0, a_ids, classes, y, x]
        boxes = np.column_stack((x, y, x, y)).astype(np.float32)
        boxes *= stride
        boxes += ca[a_ids, :]
        pred = OD.bbox_transform(boxes, box_pred[0, a_ids, classes, :, y, x])
        pred /= np.float32(scale)
        pred = OD.clip_tiled_boxes(pred, im_shape)
        for r in range(len(inds)):
            cands.append((lvl, a_ids[r], classes[r], y[r], x[r], pred[r].copy()))
        bs = np.zeros((pred.shape[0], 5))
        bs[:, 0:4], bs[:, 4] = pred, scores
        for cls in range(1, Cn + 1):
            sel = np.where(classes == cls - 1)[0]
            if len(sel) > 0:
                boxes_all.setdefault(cls, []).extend(bs[sel, :])
    dets = []
    for cls, boxes in boxes_all.items():
        cd = np.vstack(boxes).astype(np.float32)
        cd = cd[OD.nms(cd, nms_thresh), :]
        out = np.zeros((cd.shape[0], 6))
        out[:, 0:5] = cd
        out[:, 5].fill(cls)
        dets.append(out)
    dets = np.vstack(dets)
    return dets[np.argsort(-dets[:, 4])[0:dets_per_im], :].astype(np.float32), cands


def det_host_cells():
    return np.array([[OA.generate_cell64(l, a) for a in range(DET_A)] for l in range(3, 3 + len(DET_SHAPES))])


def assert_detections(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(got[:, 4], ref[:, 4])                # scores, in order
    assert np.array_equal(got[:, 5], ref[:, 5])                # classes
    np.testing.assert_allclose(got[:, :4], ref[:, :4], **DETECT_BOX_TOL)


def test_class_specific_detector_matches_the_restatement():
    from ssad_amd.roi_data.retinanet import RetinanetDetector
    probs, deltas = det_inputs()
    ref, cands = detect_restated(probs, deltas, det_host_cells(), DET_IM, 1.0)
    assert ref.shape[0] > 20 and set(ref[:, 5]) == {1.0, 2.0, 3.0}
    # candidates of one anchor and cell but different classes have different boxes
    by_cell, apart = {}, 0
    for lvl, a, c, y, x, box in cands:
        by_cell.setdefault((lvl, a, y, x), []).append((c, box))
    for group in by_cell.values():
        for i in range(len(group)):
            for j in range(i + 1, len(group)):
                apart += int(group[i][0] != group[j][0] and np.abs(group[i][1] - group[j][1]).max() > 2.0)
    assert apart > 100, apart       # (pairs the clip to the image has collapsed onto its border are not counted)
    det = RetinanetDetector(DET_SHAPES, cfg=Cfg4, class_specific_bbox=True)
    assert det.C == DET_C
    dp, dd = [torch.as_tensor(a).cuda() for a in probs], [torch.as_tensor(a).cuda() for a in deltas]
    got = det(dp, dd, DET_IM[0], DET_IM[1], 1.0).cpu().numpy()
    assert_detections(got, ref)
    # the class-agnostic detector on the deltas of class 0 alone answers another question: the indexing matters
    plain = RetinanetDetector(DET_SHAPES, cfg=Cfg4)
    d0 = [torch.as_tensor(np.ascontiguousarray(
        a.reshape(1, DET_A, DET_C, 4, a.shape[2], a.shape[3])[:, :, 0].reshape(1, DET_A * 4, a.shape[2], a.shape[3]))).cuda()
        for a in deltas]
    other = plain(dp, d0, DET_IM[0], DET_IM[1], 1.0).cpu().numpy()
    assert other.shape != ref.shape or not np.allclose(other[:, :4], ref[:, :4], **DETECT_BOX_TOL)
    with pytest.raises(K_.KernelError, match="A\\*4\\*C"):
        det(dp, d0, DET_IM[0], DET_IM[1], 1.0)
    # with the post-processing options the same indexing holds: hard Soft-NMS at the same threshold keeps the greedy set
    soft = RetinanetDetector(DET_SHAPES, cfg=Cfg4, class_specific_bbox=True, soft_nms=dict(method="hard"))
    got_soft = soft(dp, dd, DET_IM[0], DET_IM[1], 1.0).cpu().numpy()
    cand_boxes = np.stack([c[5] for c in cands])
    for row in got_soft:
        assert np.abs(cand_boxes - row[:4]).max(axis=1).min() <= 5e-3, row


# ---------------------------------------------------------------------------
# 4. isolation of the two new entry points
# ---------------------------------------------------------------------------

def test_guarded_class_specific_anchor_labels(K, monkeypatch):
    """ssad_retinanet_anchor_labels_ex(class_specific_bbox = 1) with every operand in one sentinel-filled arena: guards
    intact, inputs unchanged, rows below the counts written and rows past them untouched, the fixture reproduced."""
    from ssad_amd.modeling.generate_anchors import field_sizes
    z, H, W, Gmax, boxes, classes, counts = label_fixture()
    L = K.lib()
    L.ssad_retinanet_anchor_labels_workspace_bytes.restype = C.c_size_t
    IntArr, PtrArr = C.c_int * 5, C.c_void_p * 5
    fs_, h_, w_ = field_sizes(AnchorConfig), [H >> l for l in range(3, 8)], [W >> l for l in range(3, 8)]
    fs, h, w = IntArr(*fs_), IntArr(*h_), IntArr(*w_)
    nb = int(L.ssad_retinanet_anchor_labels_workspace_bytes(5, 9, 3, fs, 2, Gmax))
    assert nb > 0
    cells = np.ascontiguousarray(np.asarray(cell_anchors(AnchorConfig), np.float64))
    m = [z["blob_retnet_roi_fg_bbox_locs_fpn%d" % l].shape[0] for l in range(3, 8)]
    cap = max(m) + 7

    def fn(al):
        dc = al.inp("cells", cells)
        gb, gc, gn = al.inp("gt_boxes", boxes), al.inp("gt_classes", classes), al.inp("gt_counts", counts)
        labels = [al.out("labels%d" % l, (2, 9, h_[l], w_[l]), I32) for l in range(5)]
        locs = [al.out("locs%d" % l, (cap, 4)) for l in range(5)]
        targets = [al.out("targets%d" % l, (cap, 4)) for l in range(5)]
        counts_out, fg_bg = al.out("counts_out", (5,), I32), al.out("fg_bg", (2,))
        ws = al.ws(nb, "anchor_labels")
        assert ws.numel() == nb
        rc = L.ssad_retinanet_anchor_labels_ex(
            p(dc), 5, 9, 3, fs, h, w, p(gb), p(gc), p(gn), 2, Gmax, 81, C.c_float(0.5), C.c_float(0.4),
            PtrArr(*[t.data_ptr() for t in labels]), PtrArr(*[t.data_ptr() for t in locs]),
            PtrArr(*[t.data_ptr() for t in targets]), cap, p(counts_out), p(fg_bg), p(ws), C.c_size_t(nb), K._stream(), 1)
        assert rc == 0, rc
        res = dict(counts=counts_out, fg_bg=fg_bg)
        for l in range(5):
            res["labels%d" % l], res["locs%d" % l], res["targets%d" % l] = labels[l], locs[l][:m[l]], targets[l][:m[l]]
        return res

    nan_ok = {}
    for l in range(5):
        nan_ok["locs%d" % l] = nan_ok["targets%d" % l] = past(m[l], cap)
    got, arena = arena_run(K, monkeypatch, fn, nan_ok=nan_ok)
    assert list(got["counts"]) == m
    for l in range(5):
        for name in ("locs%d" % l, "targets%d" % l):
            u = arena.untouched(name)
            assert u[m[l]:].all() and not u[:m[l]].any(), name
        assert np.array_equal(got["labels%d" % l], z["blob_retnet_cls_labels_fpn%d" % (3 + l)])
        assert same(got["locs%d" % l], z["blob_retnet_roi_fg_bbox_locs_fpn%d" % (3 + l)]), l
    assert got["fg_bg"][0] == z["blob_retnet_fg_num"].reshape(-1)[0]


def test_guarded_class_specific_detect(K, monkeypatch):
    """ssad_retinanet_detect_class_specific in the arena, twice on one workspace (refilled with the sentinel in
    between): guards intact, inputs unchanged, every output row written, both calls bit-equal, the restatement met."""
    from guarded import SENTINEL
    probs, deltas = det_inputs(7200)
    TOPN, KEEP = 50, 120
    ref, _ = detect_restated(probs, deltas, det_host_cells(), DET_IM, 1.0, pre_nms_topn=TOPN, dets_per_im=KEEP)
    L = K.lib()
    n = len(DET_SHAPES)
    IntArr, PtrArr = C.c_int * n, C.c_void_p * n
    H, W = IntArr(*[h for h, _ in DET_SHAPES]), IntArr(*[w for _, w in DET_SHAPES])
    nb = int(L.ssad_retinanet_detect_ex_workspace_bytes(n, DET_A, DET_C, H, W, TOPN, None))
    assert nb > 0 and nb % 4 == 0
    cells = np.ascontiguousarray(np.asarray(cell_anchors(AnchorConfig), np.float64)[:n])

    def fn(al):
        dc = al.inp("cells", cells)
        tp = [al.inp("prob%d" % l, a) for l, a in enumerate(probs)]
        td = [al.inp("delta%d" % l, a) for l, a in enumerate(deltas)]
        ws = al.ws(nb, "detect")
        assert ws.numel() == nb
        res = {}
        for call in (1, 2):
            out, count = al.out("dets%d" % call, (KEEP, 6)), al.out("count%d" % call, (1,), I32)
            if call == 2:
                ws.view(I32).fill_(SENTINEL)
            rc = L.ssad_retinanet_detect_class_specific(
                PtrArr(*[t.data_ptr() for t in tp]), PtrArr(*[t.data_ptr() for t in td]), p(dc), n, DET_A, DET_C, 3, H, W,
                C.c_float(0.05), TOPN, C.c_float(0.5), KEEP, C.c_float(1.0), DET_IM[0], DET_IM[1],
                C.c_float(float(np.log(1000. / 16.))), p(out), p(count), p(ws), C.c_size_t(nb), K._stream(), None, 1)
            assert rc == 0, rc
            res["dets%d" % call], res["count%d" % call] = out, count
        return res

    got, _ = arena_run(K, monkeypatch, fn)
    count = int(got["count1"][0])
    assert 0 < count <= KEEP
    assert not got["dets1"].view(np.int32)[count:].any(), "rows from count on are +0.0"
    assert same(got["dets2"], got["dets1"]) and same(got["count2"], got["count1"])
    assert_detections(got["dets1"][:count], ref)


@pytest.mark.parametrize("shape", [(2, 36, 256, 5, 7), (1, 36, 256, 16, 24), (2, 20, 130, 3, 9)],
                         ids=lambda s: "N%d_K%d_M%d_%dx%d" % s)
def test_guarded_accumulate_epilogue(K, monkeypatch, shape):
    """ssad_conv3x3_forward_wino24 with SSAD_CONV_ACCUM_AUX in the arena: y = aux > 0 ? y + acc : 0 with acc = what y
    held.  Guards intact, dy / mask / pack unchanged, y fully written; bit-identical to the engine's own unmasked
    output added to acc in fp32 and masked (the two-pass form), and within CONV_RTOL / CONV_FLOOR of float64.
    Ragged maps (scalar edge stores), a channel tail (130 outputs), the sub-patch-pair and whole-patch kernels."""
    N, Kc, M, H, W = shape
    rng = np.random.default_rng(7400 + sum(shape))
    dy = rng.standard_normal((N, Kc, H, W)).astype(np.float32)
    wt = (rng.standard_normal((Kc, M, 3, 3)) * 0.05).astype(np.float32)          # the layer: M inputs -> Kc outputs
    acc = rng.standard_normal((N, M, H, W)).astype(np.float32)
    mask = rng.standard_normal((N, M, H, W)).astype(np.float32)
    _, pd = K.conv_wino24_pack_filter(torch.from_numpy(wt).cuda(), want_dgrad=True)
    plain = K.conv3x3_forward_wino24([torch.from_numpy(dy).cuda()], pd, None, M)[0]
    two_pass = torch.where(torch.from_numpy(mask).cuda() > 0, plain + torch.from_numpy(acc).cuda(),
                           torch.zeros((), device="cuda"))
    ref = F.conv_transpose2d(t64(dy), t64(wt), padding=1).numpy()                # the data gradient, float64
    ref = np.where(mask > 0, ref + acc.astype(np.float64), 0.0)
    pd_host = pd.cpu().numpy()

    def fn(al):
        x, a, pk = al.inp("dy", dy), al.inp("mask", mask), al.inp("pack", pd_host)
        y = al.inp("y", acc)
        K.conv3x3_forward_wino24([x], pk, None, M, out=[y], mask_by=[a], accumulate=True)
        return dict(y=y)

    got, _ = arena_run(K, monkeypatch, fn, modified=("y",))
    assert np.array_equal(got["y"].view(np.int32), two_pass.cpu().numpy().view(np.int32)), "differs from the two-pass form"
    assert (got["y"][mask <= 0] == 0).all()
    print("accumulate epilogue %s: worst error / limit %.3f" % (shape, worst(got["y"], ref)))
    close(got["y"], ref, CONV_RTOL, CONV_FLOOR, "accumulated, masked data gradient")
    with pytest.raises(K.KernelError):
        K.conv3x3_forward_wino24([torch.from_numpy(dy).cuda()], pd, None, M, accumulate=True)


# ---------------------------------------------------------------------------
# 5. the operator surface
# ---------------------------------------------------------------------------

def test_both_switches_through_the_operator_surface():
    """The builder's net with both switches on, differentiated by AddGradientOperators, through CreateNet / RunNet at
    N = 1 against the native program: losses and the two prediction layers' filter gradients."""
    kw = dict(num_classes=4, share_cls_bbox_tower=True, class_specific_bbox=True)
    c = case("both/N1", kw, False, N=1)
    pb, heads = c["pb"], c["heads"]
    cfg = pb["cfg"]
    dyndep.InitOpsLibrary()
    workspace.ResetWorkspace()
    try:
        levels = list(cfg.levels())
        with core.DeviceScope(GPU):
            student = rh.HeadModel(cfg, train=True, name="head_options")
            rh.add_fpn_retinanet_outputs(student, ["fpn_%d" % l for l in reversed(levels)], cfg.fpn_dim)
            loss_grads = rh.add_fpn_retinanet_losses(student)
            grad_map = student.net.AddGradientOperators(loss_grads)
        assert not [op for op in student.net.Proto().op if "bbox_conv" in "".join(op.output)]

        def feed(name, arr):
            workspace.FeedBlob(name, arr, device_option=GPU)
        for name, shape, _ in student.params:
            assert tuple(shape) == pb["S"][name].shape, name
            feed(name, pb["S"][name])
        feed("retnet_fg_num", np.array(pb["fg"][0], np.float32))
        for i, l in enumerate(levels):
            feed("fpn_%d" % l, pb["fs"][i])
            feed("retnet_cls_labels_fpn%d" % l, pb["labs"][i])
            feed("retnet_roi_bbox_targets_fpn%d" % l, pb["tg"][i][0])
            feed("retnet_roi_fg_bbox_locs_fpn%d" % l, pb["tg"][i][1])
        workspace.CreateNet(student.net)
        workspace.RunNet(student.net)
        fl = np.array([workspace.FetchBlob("fl_fpn%d" % l) for l in levels], np.float64)
        bl = np.array([workspace.FetchBlob("retnet_loss_bbox_fpn%d" % l) for l in levels], np.float64)
        print("operator surface: focal %s bbox %s" % (fl, bl))
        close(heads.focal_losses.cpu().numpy(), fl, LOSS_RTOL, 0, "focal losses vs operators")
        close(heads.bbox_losses.cpu().numpy(), bl, LOSS_RTOL, 1e-9, "bbox losses vs operators")
        for name in ("retnet_cls_pred_fpn3_w", "retnet_bbox_pred_fpn3_w"):
            want = workspace.FetchBlob(grad_map[name])
            print("operator surface: %s error / limit %.3f" % (name, worst(heads.grads[name].cpu().numpy(), want)))
            close(heads.grads[name].cpu().numpy(), want, CONV_RTOL, CONV_FLOOR, name + "_grad")
        # and the shared activation's gradient went through the Sum: the deepest tower filter agrees too
        name = "retnet_cls_conv_n3_fpn3_w"
        close(heads.grads[name].cpu().numpy(), workspace.FetchBlob(grad_map[name]), CONV_RTOL, CONV_FLOOR, name + "_grad")
    finally:
        workspace.ResetWorkspace()
