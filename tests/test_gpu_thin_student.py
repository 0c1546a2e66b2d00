"""Thin students on the GPU (RESNETS.CHANNEL_RATIO < 1): the native backbone at half and quarter width against the
float64 torch network (tests/torch_ref_thin.py) under the bounds of tests/test_gpu_backbone.py, the subnets at
FPN dimension 128 and 64 against the CPU oracle under tests/test_gpu_kernels.py's CONV_RTOL / CONV_FLOOR, the whole
distillation step with a half-width student under a full-width teacher under the bounds of
tests/test_gpu_native_model.py, and weights files of a thin model."""
import numpy as np
import pytest
import torch

import ssad_amd  # noqa: F401
from ssad_amd import synth
from ssad_amd.modeling.retinanet_heads import HeadConfig
from oracle import head_step

from torch_ref import RefResNetFPN
from torch_ref_thin import RefThinResNetFPN
from test_gpu_operators import make_mask_safe, close_1e4
from test_gpu_kernels import close, CONV_RTOL, CONV_FLOOR

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


# ---------------------------------------------------------------------------------------------------------------
# 1. backbone alone
# ---------------------------------------------------------------------------------------------------------------

def _run_backbone(ratio, mask_safe):
    from ssad_amd.backbone_pipeline import NativeResNetFPN
    N, hw = 1, (128, 256)
    gen = torch.Generator(device="cuda").manual_seed(5)
    images = torch.randn((N, 3) + hw, device="cuda", generator=gen)
    ref = RefThinResNetFPN("r50", ratio, seed=11)
    if mask_safe:
        ref.calibrate(images)
    nat = NativeResNetFPN("r50", N, hw, "cuda", train=True, src=ref.state_dict(), lr=0.01,
                          affine_scales=ref.scales, channel_ratio=ratio)
    nat.pack()
    got = nat.forward(images)
    want = ref(images)
    assert [tuple(t.shape) for t in got] == [tuple(t.shape) for t in want]
    assert got[0].shape[1] == int(256 * ratio)
    fwd = [rel(g, w.detach()) for g, w in zip(got, want)]
    print("ratio %g mask_safe %s forward rel %s" % (ratio, mask_safe, ["%.2e" % e for e in fwd]))
    assert max(fwd) < 2e-5, fwd
    d_fpn = [torch.randn(t.shape, device="cuda", generator=gen) for t in want]
    torch.autograd.backward(want, [d.double() for d in d_fpn])
    nat.backward(d_fpn)
    torch.cuda.synchronize()
    errs = {}
    for name, p in ref.p.items():
        lname, kind = name.rsplit(".", 1)
        layer = nat._layers[lname]
        g = layer.gw if kind == "weight" else layer.gb
        if not p.requires_grad:
            assert g is None and p.grad is None, name
            continue
        errs[name] = rel(g, p.grad)
    assert len(errs) == sum(1 + (l.gb is not None) for l in nat._layers.values() if l.train)
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
    print("ratio %g mask_safe %s worst gradients %s" % (ratio, mask_safe, [(k, "%.2e" % v) for k, v in worst]))
    return nat, ref, errs


def _engines(nat):
    """3x3 / stride 1 forward engines of the program's launch records: 0 direct, 1 F(2x2), 2 F(2x4), 3 split-operand."""
    from ssad_amd import program as PR
    return {(int(o.i[1]), int(o.i[2])): int(o.i[4]) for o in nat.prog.ops if o.code == PR.CONV3X3}


ENGINES = {     # (Cout, Cin) of the 3x3 layers -> engine, by the width rules measured at ratio 1
    0.5: {(32, 32): 1, (64, 64): 1, (128, 128): 2, (256, 256): 3},                # res2, res3, res4 + FPN outputs, res5
    0.25: {(16, 16): 0, (32, 32): 1, (64, 64): 1, (128, 128): 2},                 # res2, res3, res4 + FPN outputs, res5
}


@pytest.mark.parametrize("ratio", [0.5, 0.25])
def test_thin_backbone_forward_backward_sgd_vs_torch(ratio):
    """tests/test_gpu_backbone.py::test_native_backbone_forward_backward_vs_torch at ratio 0.5 / 0.25: FPN outputs
    2e-5, the FPN's own gradients 2e-5, free-running body gradients 1e-2 (a flipped ReLU mask, see there), the SGD
    update with the s^2 rows.  Between them the two ratios run a 3x3 layer on each of the four engines."""
    nat, ref, errs = _run_backbone(ratio, mask_safe=False)
    assert _engines(nat) == ENGINES[ratio]
    fpn = [v for k, v in errs.items() if k.split(".")[0] in ("lat", "out", "p6")]
    assert max(fpn) < 2e-5, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    worst = max(errs, key=errs.get)
    assert errs[worst] < 1e-2, (worst, errs[worst])
    p0, g0 = nat.params_flat.clone(), nat.grads_flat.clone()
    nat.sgd_step()
    want = torch.empty_like(p0)
    scaled = 0
    for off, n, is_bias, row_len, s2 in nat.segments:
        g = g0[off:off + n]
        if s2 is not None:
            g = (g.view(-1, row_len) * s2.view(-1, 1)).reshape(-1)
            scaled += 1
        want[off:off + n] = p0[off:off + n] - 0.01 * (2.0 * g if is_bias else g + 1e-4 * p0[off:off + n])
    assert scaled == sum(1 for l in nat._layers.values() if l.train and l.affine)
    assert sum(n for _, n, _, _, _ in nat.segments) == nat.params_flat.numel()
    assert float(nat._layers["res3.0.c3"].s2[0]) == pytest.approx(0.0625)
    assert torch.allclose(nat.params_flat, want, rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("ratio", [0.5, 0.25])
def test_thin_backbone_meets_1e4_when_masks_cannot_flip(ratio):
    """Every gradient at 1e-4 once no pre-activation of the trainable part sits within round-off of zero
    (tests/test_gpu_backbone.py::test_native_backbone_meets_1e4_when_masks_cannot_flip)."""
    nat, _, errs = _run_backbone(ratio, mask_safe=True)
    worst = max(errs, key=errs.get)
    assert errs[worst] < 1e-4, sorted(errs.items(), key=lambda kv: -kv[1])[:5]


# ---------------------------------------------------------------------------------------------------------------
# 2. subnets alone at FPN dimension 128 and 64
# ---------------------------------------------------------------------------------------------------------------

HEAD_SHAPES = [(5, 7), (3, 4)]


@pytest.mark.parametrize("dim", [128, 64])
def test_subnets_at_thin_fpn_dimension_vs_oracle(dim):
    """N = 2, two ragged levels: predictions (forward through the four tower layers, cls_pred D -> 720, bbox_pred
    D -> 36), the gradient w.r.t. both levels (data gradients) and every filter / bias gradient (summed over the
    levels) against the CPU oracle, element by element at CONV_RTOL / CONV_FLOOR.  ReLU masks are flip-proof
    (make_mask_safe), so what is compared is arithmetic."""
    from ssad_amd.head_pipeline import DistillHeads
    from ssad_amd import program as PR
    N = 2
    rng = np.random.default_rng(40 + dim)
    cfg = HeadConfig(num_gpus=1, fpn_dim=dim)
    S, T = synth.head_params(rng, dim=dim), synth.head_params(rng, dim=dim)
    for P in (S, T):
        for k in P:
            if k.endswith("_w"):
                P[k] = (P[k] * 3).astype(np.float32)          # gradients well above fp32 noise (small_problem)
    fs = synth.fpn_features(rng, N, HEAD_SHAPES, dim=dim)
    ft = synth.fpn_features(rng, N, HEAD_SHAPES, dim=dim)
    S = make_mask_safe(cfg, S, fs)
    labs = []
    for h, w in HEAD_SHAPES:
        lab = synth.distill_inputs(rng, N, 9, 80, h, w)[2]
        u = rng.random(lab.shape)
        lab[u < 0.1] = rng.integers(1, 81, size=int((u < 0.1).sum()))
        labs.append(lab)
    tg = [synth.bbox_targets(rng, l) for l in labs]
    fg = np.array([float(sum(t[0].shape[0] for t in tg))], np.float32)
    ref = head_step.head_step(S, T, fs, ft, labs, scale=1.0, bbox_targets=tg, fg_num=fg)

    heads = DistillHeads(cfg, N=N, shapes=HEAD_SHAPES, device="cuda", student_init=S, teacher_init=T)
    assert heads.D == heads.Dt == dim and heads.params["retnet_cls_pred_fpn3_w"].shape == (720, dim, 3, 3)
    # the towers run on the split-operand engine forward and backward; the filter gradients of >= 128 outputs too
    fwd = [o for o in heads.prog.ops if o.code == PR.CONV3X3 and (o.i[1], o.i[2]) == (dim, dim)]
    assert len(fwd) == 8 and all(o.i[4] == 3 for o in fwd)
    wg = {int(o.i[1]): int(o.i[4]) for o in heads.prog.ops if o.code == PR.CONV3X3_WGRAD}
    assert wg == {720: 1, 36: 0, dim: 1 if dim >= 128 else 0}
    to = lambda a: torch.from_numpy(a).cuda()
    heads.step([to(a) for a in fs], [to(a) for a in ft], [to(a) for a in labs], update=False,
               bbox_targets=[(to(y), to(l)) for y, l in tg], fg_num=to(fg))
    torch.cuda.synchronize()
    for l in range(len(HEAD_SHAPES)):
        close(heads.cls_logits[l].cpu().numpy(), ref["cls_logits"][l], CONV_RTOL, CONV_FLOOR, "cls_logits %d" % l)
        close(heads.bbox_pred[l].cpu().numpy(), ref["bbox_pred"][l], CONV_RTOL, CONV_FLOOR, "bbox_pred %d" % l)
        close(heads.t_prob[l].cpu().numpy(), ref["t_prob"][l], CONV_RTOL, CONV_FLOOR, "teacher prob %d" % l)
        for t in ("cls", "bbox"):
            close(heads.d_fpn[t][l].cpu().numpy(), ref["d_fpn"][t][l], CONV_RTOL, CONV_FLOOR, "d_fpn %s %d" % (t, l))
    for name, g in ref["grads"].items():
        close(heads.grads[name].cpu().numpy(), g, CONV_RTOL, CONV_FLOOR, name)


# ---------------------------------------------------------------------------------------------------------------
# 3.-5. the whole step: half-width R-50 student under a full-width R-50 teacher
# ---------------------------------------------------------------------------------------------------------------

N, HW = 1, (128, 128)
SHAPES = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
LR, MU, WD = 1e-4, 0.9, 1e-4
_cache = {}


def _problem(ratio=0.5, seed=3):
    """Computed once per (ratio, seed) and shared; nothing in it is modified afterwards (the reference networks
    are rebuilt from the seed by whoever trains them)."""
    key = (ratio, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        gen = torch.Generator(device="cuda").manual_seed(seed)
        images = torch.randn((N, 3) + HW, device="cuda", generator=gen)
        dim = int(256 * ratio)
        ref_s = RefThinResNetFPN("r50", ratio, seed=11).calibrate(images)
        ref_t = RefResNetFPN("r50", seed=12)
        with torch.no_grad():
            fs = [f.float().cpu().numpy() for f in ref_s(images)]
        cfg = HeadConfig(num_gpus=1, fpn_dim=dim)
        S = make_mask_safe(cfg, synth.head_params(rng, dim=dim), fs)
        T = synth.head_params(rng)
        labs = [synth.distill_inputs(rng, N, 9, 80, h, w)[2] for h, w in SHAPES]
        tg = [synth.bbox_targets(rng, l) for l in labs]
        fg = np.array([max(1, sum(t[0].shape[0] for t in tg))], np.float32)
        _cache[key] = (cfg, images, ref_s.state_dict(), dict(ref_s.scales), ref_t, S, T, labs, tg, fg)
    cfg, images, sd, scales, ref_t, S, T, labs, tg, fg = _cache[key]
    ref_s = RefThinResNetFPN("r50", ratio, seed=11)
    with torch.no_grad():
        for k, v in sd.items():
            ref_s.p[k].copy_(v)
    return cfg, images, ref_s, ref_t, dict(S), T, labs, tg, fg


def _reference(cfg, images, ref_s, ref_t, S, T, labs, tg, fg):
    ref_s.zero_grad()
    f_s = ref_s(images)
    with torch.no_grad():
        f_t = ref_t(images)
    fs = [f.detach().float().cpu().numpy() for f in f_s]
    ft = [f.float().cpu().numpy() for f in f_t]
    out = head_step.head_step(S, T, fs, ft, labs, scale=cfg.loss_scale * cfg.temperature ** 2,
                              loss_scale=cfg.loss_scale, bbox_targets=tg, fg_num=fg)
    d_fpn = [out["d_fpn"]["cls"][l].astype(np.float64) + out["d_fpn"]["bbox"][l] for l in range(len(fs))]
    torch.autograd.backward(f_s, [torch.from_numpy(d).to(images.device) for d in d_fpn])
    out["fpn_student"], out["fpn_teacher"], out["d_fpn_sum"] = fs, ft, d_fpn
    out["backbone_grads"] = {k: v.grad.detach().clone() for k, v in ref_s.named_parameters()}
    return out


def _model(cfg, ref_s, ref_t, S, T, overlap, ratio=0.5, **kw):
    from ssad_amd.head_pipeline import DistillHeads
    from ssad_amd.backbone_pipeline import NativeDistillModel
    heads = DistillHeads(cfg, N=N, shapes=SHAPES, device="cuda", student_init=S, teacher_init=T, lr=LR,
                         momentum=MU, weight_decay=WD, overlap_wgrad=overlap, teacher_fpn_dim=256)
    return NativeDistillModel(heads, "r50", "r50", N, HW, "cuda", lr=LR, momentum=MU, weight_decay=WD,
                              two_streams=overlap, overlap_wgrad=overlap, student_src=ref_s.state_dict(),
                              teacher_src=ref_t.state_dict(), student_scales=ref_s.scales, **kw)


def _inputs(labs, tg, fg):
    to = lambda a: torch.from_numpy(a).cuda()
    return [to(a) for a in labs], [(to(y), to(l)) for y, l in tg], to(fg)


def _check_gradients(model, ref, tag):
    h, st = model.heads, model.student
    for l in range(len(SHAPES)):
        close_1e4(st.fpn[l].cpu().numpy(), ref["fpn_student"][l], "%s student P%d" % (tag, l + 3))
        close_1e4(model.teacher.fpn[l].cpu().numpy(), ref["fpn_teacher"][l], "%s teacher P%d" % (tag, l + 3))
        if l != 3:      # P6's buffer also receives P7's gradient through relu(P6) in place (FPN.py:193-224)
            close_1e4(st.d_fpn[l].cpu().numpy(), ref["d_fpn_sum"][l], "%s d_fpn P%d" % (tag, l + 3))
    np.testing.assert_allclose(h.losses.cpu().numpy(), ref["losses"], rtol=1e-4)
    np.testing.assert_allclose(h.focal_losses.cpu().numpy(), ref["focal_losses"], rtol=1e-4)
    np.testing.assert_allclose(h.bbox_losses.cpu().numpy(), ref["bbox_losses"], rtol=1e-4)
    for name, g in ref["grads"].items():
        close_1e4(h.grads[name].cpu().numpy(), g, "%s %s" % (tag, name))
    seen = 0
    for name, g in ref["backbone_grads"].items():
        lname, kind = name.rsplit(".", 1)
        layer = st._layers[lname]
        mine = layer.gw if kind == "weight" else layer.gb
        assert mine is not None, name
        close_1e4(mine.cpu().numpy(), g.cpu().numpy(), "%s %s" % (tag, name))
        seen += 1
    assert seen == sum(1 + (l.gb is not None) for l in st._layers.values() if l.train)


def _expected_update(model, ref, p_heads, p_body, m_heads, m_body):
    h, st = model.heads, model.student
    want_h = torch.empty_like(p_heads)
    for name, shape, is_bias, _ in h.params.specs:
        off, n = h.params.offsets[name], int(np.prod(shape))
        g = torch.from_numpy(np.asarray(ref["grads"][name], np.float64)).reshape(-1).cuda()
        w = p_heads[off:off + n].double()
        gg = 2.0 * g if is_bias else g + WD * w
        want_h[off:off + n] = (LR * gg + MU * m_heads[off:off + n].double()).float()
    want_b = torch.empty_like(p_body)
    for lname, layer in st._layers.items():
        if not layer.train:
            continue
        off = (layer.w.data_ptr() - st.params_flat.data_ptr()) // 4
        n = layer.w.numel()
        g = ref["backbone_grads"][lname + ".weight"].reshape(layer.cout, -1)
        if layer.s2 is not None:
            g = g * layer.s2.double().view(-1, 1)
        w = p_body[off:off + n].double()
        want_b[off:off + n] = (LR * (g.reshape(-1) + WD * w) + MU * m_body[off:off + n].double()).float()
        if layer.gb is not None:
            ob = (layer.b.data_ptr() - st.params_flat.data_ptr()) // 4
            gb = ref["backbone_grads"][lname + ".bias"]
            want_b[ob:ob + layer.cout] = (LR * 2.0 * gb + MU * m_body[ob:ob + layer.cout].double()).float()
    return want_h, want_b


def test_half_width_student_under_full_width_teacher_two_updates_vs_composed_reference():
    """tests/test_gpu_native_model.py's first test with student_channel_ratio = 0.5: losses, every subnet and
    backbone gradient at 1e-4, two updates (momentum in play) at its bounds."""
    cfg, images, ref_s, ref_t, S, T, labs, tg, fg = _problem()
    labels, targets, fg_num = _inputs(labs, tg, fg)
    model = _model(cfg, ref_s, ref_t, S, T, overlap=True, student_channel_ratio=0.5)
    h, st = model.heads, model.student
    assert st.D == 128 and model.teacher.D == 256 and h.D == 128 and h.Dt == 256
    assert st.fpn[0].shape == (N, 128, 16, 16) and model.teacher.fpn[0].shape == (N, 256, 16, 16)
    assert st._layers["res5.0.c2"].cout == 256 and model.teacher._layers["res5.0.c2"].cout == 512

    ref1 = _reference(cfg, images, ref_s, ref_t, S, T, labs, tg, fg)
    model.step(images, labels, targets, fg_num, update=False)
    torch.cuda.synchronize()
    _check_gradients(model, ref1, "step 1")

    p_h0, p_b0 = h.params.flat.clone(), st.params_flat.clone()
    z_h, z_b = torch.zeros_like(p_h0), torch.zeros_like(p_b0)
    model.step(images, labels, targets, fg_num)
    torch.cuda.synchronize()
    want_h, want_b = _expected_update(model, ref1, p_h0, p_b0, z_h, z_b)
    m_h1, m_b1 = h.moms.flat.clone(), st.moms_flat.clone()
    print("update 1 rel", rel(m_h1, want_h), rel(m_b1, want_b))
    assert rel(m_h1, want_h) < 1e-4 and rel(m_b1, want_b) < 1e-4, (rel(m_h1, want_h), rel(m_b1, want_b))
    assert torch.equal(h.params.flat, p_h0 - m_h1) and torch.equal(st.params_flat, p_b0 - m_b1)
    assert torch.equal(st._layers["res3.0.c1"].b.cpu(), ref_s.p["res3.0.c1.bias"].float().cpu())
    assert torch.equal(st._layers["res2.0.c1"].w.cpu(), ref_s.p["res2.0.c1.weight"].float().cpu())

    with torch.no_grad():
        for lname, layer in st._layers.items():
            if layer.train:
                ref_s.p[lname + ".weight"].copy_(layer.w.double())
                if layer.gb is not None:
                    ref_s.p[lname + ".bias"].copy_(layer.b.double())
    S2 = {name: h.params[name].cpu().numpy().copy() for name in S}
    ref2 = _reference(cfg, images, ref_s, ref_t, S2, T, labs, tg, fg)
    p_h1, p_b1 = h.params.flat.clone(), st.params_flat.clone()
    model.step(images, labels, targets, fg_num)
    torch.cuda.synchronize()
    np.testing.assert_allclose(h.losses.cpu().numpy(), ref2["losses"], rtol=1e-4)
    want_h, want_b = _expected_update(model, ref2, p_h1, p_b1, m_h1, m_b1)
    print("update 2 rel", rel(h.moms.flat, want_h), rel(st.moms_flat, want_b))
    assert rel(h.moms.flat, want_h) < 1e-4 and rel(st.moms_flat, want_b) < 1e-4, \
        (rel(h.moms.flat, want_h), rel(st.moms_flat, want_b))
    new_b, want_new_b = st.moms_flat - MU * m_b1, want_b - MU * m_b1
    assert rel(new_b, want_new_b) < 2e-4, rel(new_b, want_new_b)
    assert torch.equal(st.params_flat, p_b1 - st.moms_flat)


def test_half_width_step_overlapped_and_on_one_stream_agree_bit_for_bit():
    """The same two steps with the teacher on a second stream and the filter gradients on the auxiliary streams,
    and on one stream: identical bits (a missing dependency shows up as a difference)."""
    cfg, images, ref_s, ref_t, S, T, labs, tg, fg = _problem(seed=4)
    labels, targets, fg_num = _inputs(labs, tg, fg)
    a = _model(cfg, ref_s, ref_t, S, T, overlap=True, student_channel_ratio=0.5)
    b = _model(cfg, ref_s, ref_t, S, T, overlap=False, student_channel_ratio=0.5)
    assert a.side is not None and b.side is None and b.student._wstreams == [0] and b.heads._wstream == 0
    for it in range(2):
        for m in (a, b):
            if it == 0:
                m.student.poison()
                m.teacher.poison()
            m.step(images, labels, targets, fg_num)
        torch.cuda.synchronize()
        for name in ("losses", "focal_losses", "bbox_losses"):
            assert torch.equal(getattr(a.heads, name), getattr(b.heads, name)), (it, name)
        assert torch.isfinite(a.heads.losses).all()
        for x, y, what in ((a.heads.params.flat, b.heads.params.flat, "subnet parameters"),
                           (a.heads.moms.flat, b.heads.moms.flat, "subnet momentum"),
                           (a.student.params_flat, b.student.params_flat, "backbone parameters"),
                           (a.student.moms_flat, b.student.moms_flat, "backbone momentum"),
                           (a.student.grads_flat, b.student.grads_flat, "backbone update")):
            assert torch.isfinite(x).all(), (it, what)
            assert torch.equal(x, y), (it, what, float((x - y).abs().max()))
        for l in range(len(SHAPES)):
            assert torch.equal(a.student.d_fpn[l], b.student.d_fpn[l]), (it, "d_fpn", l)
            assert torch.equal(a.teacher.fpn[l], b.teacher.fpn[l]), (it, "teacher fpn", l)


def test_ratio_one_passed_explicitly_changes_no_bit():
    """student_channel_ratio=1.0 / channel_ratio=1.0 and the default constructors: the same launch records and,
    after one step, bit-identical parameters."""
    from ssad_amd.head_pipeline import DistillHeads
    from ssad_amd.backbone_pipeline import NativeDistillModel
    rng = np.random.default_rng(8)
    S, T = synth.head_params(rng), synth.head_params(rng)
    labs = [synth.distill_inputs(rng, N, 9, 80, h, w)[2] for h, w in SHAPES]
    tg = [synth.bbox_targets(rng, l) for l in labs]
    fg = np.array([max(1, sum(t[0].shape[0] for t in tg))], np.float32)
    labels, targets, fg_num = _inputs(labs, tg, fg)
    images = torch.randn((N, 3) + HW, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
    models = []
    for kw_h, kw_m in (({}, {}), (dict(teacher_fpn_dim=256), dict(student_channel_ratio=1.0))):
        heads = DistillHeads(HeadConfig(num_gpus=1), N=N, shapes=SHAPES, device="cuda", student_init=S,
                             teacher_init=T, lr=LR, **kw_h)
        m = NativeDistillModel(heads, "r50", "r50", N, HW, "cuda", lr=LR, **kw_m)
        m.step(images, labels, targets, fg_num)
        models.append(m)
    torch.cuda.synchronize()
    a, b = models
    sig = lambda prog: [(int(o.code), [int(v) for v in o.i]) for o in prog.ops]
    assert sig(a.student.prog) == sig(b.student.prog) and sig(a.heads.prog) == sig(b.heads.prog)
    assert torch.isfinite(a.student.params_flat).all()
    assert torch.equal(a.student.params_flat, b.student.params_flat)
    assert torch.equal(a.student.moms_flat, b.student.moms_flat)
    assert torch.equal(a.heads.params.flat, b.heads.params.flat)
    assert torch.equal(a.heads.losses, b.heads.losses)


def test_thin_model_weights_file_reloads_bit_for_bit(tmp_path):
    """A half-width model (random initialisation, one update so that momentum exists) saved in the reference's blob
    layout and loaded into a fresh model: same blobs at the scaled dims, same parameters, momentum and forward
    outputs, bit for bit (the folded scales of the initialisation are powers of two: un-fold / fold is exact)."""
    from ssad_amd.head_pipeline import DistillHeads
    from ssad_amd.backbone_pipeline import NativeDistillModel
    from ssad_amd.utils import net
    rng = np.random.default_rng(9)
    cfg = HeadConfig(num_gpus=1, fpn_dim=128)
    S, T = synth.head_params(rng, dim=128), synth.head_params(rng)
    labs = [synth.distill_inputs(rng, N, 9, 80, h, w)[2] for h, w in SHAPES]
    tg = [synth.bbox_targets(rng, l) for l in labs]
    fg = np.array([max(1, sum(t[0].shape[0] for t in tg))], np.float32)
    labels, targets, fg_num = _inputs(labs, tg, fg)
    images = torch.randn((N, 3) + HW, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))

    def heads():
        return DistillHeads(cfg, N=N, shapes=SHAPES, device="cuda", lr=1e-3, teacher_fpn_dim=256)
    h0 = DistillHeads(cfg, N=N, shapes=SHAPES, device="cuda", student_init=S, teacher_init=T, lr=1e-3,
                      teacher_fpn_dim=256)
    a = NativeDistillModel(h0, "r50", "r50", N, HW, "cuda", student_channel_ratio=0.5)
    a.step(images, labels, targets, fg_num)
    torch.cuda.synchronize()
    assert float(a.student.moms_flat.abs().max()) > 0
    path = str(tmp_path / "thin.pkl")
    net.save_model_to_weights_file(path, a)
    blobs, _ = net._blobs_and_cfg(net.load_object(path))
    assert blobs["res5_2_branch2b_w"].shape == (256, 256, 3, 3) and blobs["fpn_6_w"].shape == (128, 1024, 3, 3)
    assert blobs["teacher/res5_2_branch2b_w"].shape == (512, 512, 3, 3)
    assert blobs["retnet_cls_pred_fpn3_w"].shape == (720, 128, 3, 3)
    assert blobs["teacher/retnet_cls_pred_fpn3_w"].shape == (720, 256, 3, 3)
    assert blobs["res4_0_branch2a_w_momentum"].shape == (128, 256, 1, 1)

    b, loaded, missing = net.native_model_from_weights_files(heads(), path, student_arch="r50", teacher_arch="r50",
                                                             N=N, image_hw=HW, student_channel_ratio=0.5)
    assert not missing
    assert torch.equal(b.student.params_flat, a.student.params_flat)
    assert torch.equal(b.student.frozen_flat, a.student.frozen_flat)
    assert torch.equal(b.student.moms_flat, a.student.moms_flat)
    assert torch.equal(b.heads.params.flat, a.heads.params.flat) and torch.equal(b.heads.teacher.flat, a.heads.teacher.flat)
    for m in (a, b):
        m.step(images, labels, targets, fg_num, update=False)
    torch.cuda.synchronize()
    for l in range(len(SHAPES)):
        assert torch.equal(a.student.fpn[l], b.student.fpn[l]), l
        assert torch.equal(a.teacher.fpn[l], b.teacher.fpn[l]), l
        assert torch.equal(a.heads.cls_logits[l], b.heads.cls_logits[l]) and torch.equal(a.heads.bbox_pred[l], b.heads.bbox_pred[l])
    assert torch.equal(a.heads.losses, b.heads.losses)
    # and a full-width model refuses the file by name
    with pytest.raises(net.WeightsWidthError):
        net.native_model_from_weights_files(DistillHeads(HeadConfig(num_gpus=1), N=N, shapes=SHAPES, device="cuda"),
                                            path, student_arch="r50", teacher_arch="r50", N=N, image_hw=HW)
