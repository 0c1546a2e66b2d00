"""The softmax RetinaNet head on the native step, without a GPU: parameter specs and program records of
DistillHeads(HeadConfig(softmax=True), distill=False), the two refusals, the unchanged sigmoid programs, and the
new C entry points' argument checks (they return before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

import ssad_amd  # noqa: F401
from ssad_amd import kernels as K, program as PR
from ssad_amd.head_pipeline import DistillHeads, DistillHeadsF16, head_param_specs
from ssad_amd.modeling import retinanet_heads as rh
from ssad_amd.modeling.retinanet_heads import HeadConfig

SHAPES = [(10, 14), (5, 7), (3, 4), (2, 2), (1, 1)]


def _codes(h, lo, hi):
    return [o.code for o in h.prog.ops[h.prog.marks[lo]:h.prog.marks[hi]]]


def test_softmax_specs_and_program_records():
    cfg = HeadConfig(softmax=True, num_gpus=1)
    h = DistillHeads(cfg, N=1, shapes=SHAPES, device="cpu", distill=False)
    A = cfg.num_anchors
    assert tuple(h.params["retnet_cls_pred_fpn3_w"].shape) == (A * 81, 256, 3, 3)
    assert tuple(h.params["retnet_cls_pred_fpn3_b"].shape) == (A * 81,)
    assert tuple(h.grads["retnet_cls_pred_fpn3_w"].shape) == (A * 81, 256, 3, 3)
    assert [tuple(x.shape) for x in h.cls_logits] == [(1, A * 81, a, b) for a, b in SHAPES]
    assert [tuple(x.shape) for x in h.d_cls_logits] == [(1, A * 81, a, b) for a, b in SHAPES]
    assert tuple(h.params["retnet_bbox_pred_fpn3_w"].shape) == (4 * A, 256, 3, 3)       # the box subnet is the same
    assert _codes(h, "losses", "backward") == [PR.SOFTMAX_FOCAL_FUSED, PR.SMOOTH_L1]
    assert PR.SOFTMAX_FOCAL_FUSED == 83
    rec = h.prog.ops[h.prog.marks["losses"]]
    # the record: level count, the table, fg_num, dloss 1.0 on the host, the parameters, the losses, the workspace
    assert rec.i[0] == len(SHAPES) and rec.f[0] == 1.0
    tab = ctypes.cast(rec.p[0], ctypes.POINTER(K.SoftmaxFocalLevel))
    assert rec.p[0] == ctypes.addressof(h._label_tables[-1])
    for l, (a, b) in enumerate(SHAPES):
        assert (tab[l].N, tab[l].D, tab[l].H, tab[l].W) == (1, A * 81, a, b)
        assert tab[l].logits == h.cls_logits[l].data_ptr() and tab[l].out == h.d_cls_logits[l].data_ptr()
        assert tab[l].labels == h.labels[l].data_ptr() and not tab[l].prob           # P stays in registers
    assert rec.p[1] == h.fg_num.data_ptr() and rec.p[3] == h.focal_losses.data_ptr() and rec.p[4]
    fp = ctypes.cast(rec.p[2], ctypes.POINTER(K.FocalParams))[0]
    assert (fp.gamma, fp.alpha, fp.num_classes, fp.scale) == (2.0, 0.25, 81, 1.0)
    assert rec.l[0] >= K.lib().ssad_softmax_focal_loss_fused_workspace_bytes(len(SHAPES)) > 0
    assert rec.klass == 17 and rec.klass in PR.KLASS and "softmax_focal_fused_kernel" in PR.KLASS[17]["name"]
    used = {o.klass for o in DistillHeads(HeadConfig(num_gpus=1), N=1, shapes=SHAPES[:2], device="cpu").prog.ops}
    assert 17 not in used                                                            # a class of its own
    # labels are rebound through the same table
    labs = [torch.zeros((1, A, a, b), dtype=torch.int32) for a, b in SHAPES]
    h._bind(labels=labs)
    assert [tab[l].labels for l in range(len(SHAPES))] == [g.data_ptr() for g in labs]
    # the default bias is the builder's GivenTensorFill vector; everything else starts at zero like the sigmoid head
    filler, kw = rh.retinanet_bias_init(cfg)
    assert filler == "GivenTensorFill"
    want = np.asarray(kw["values"], np.float32).reshape(-1)
    assert np.array_equal(h.params["retnet_cls_pred_fpn3_b"].numpy(), want) and want[0] > 8 and want[1] == 0
    assert float(h.params["retnet_cls_pred_fpn3_w"].abs().sum()) == 0.0
    # a caller's initialisation wins
    init = {"retnet_cls_pred_fpn3_b": np.full(A * 81, 0.5, np.float32)}
    h2 = DistillHeads(cfg, N=1, shapes=SHAPES[:2], device="cpu", distill=False, student_init=init)
    assert float(h2.params["retnet_cls_pred_fpn3_b"].min()) == 0.5
    # the prediction layer and its data gradient take the engines the width rules give a >= 128-wide layer
    fwd = [o for o in h.prog.ops[h.prog.marks["forward"]:h.prog.marks["losses"]] if o.code == PR.CONV3X3]
    assert [(o.i[1], o.i[4]) for o in fwd][4] == (A * 81, 3)
    wg = [o for o in h.prog.ops if o.code == PR.CONV3X3_WGRAD and o.i[1] == A * 81]
    assert len(wg) == 1
    # SGD and the all-reduce buckets follow from the specs
    assert h.params.flat.numel() == sum(int(np.prod(s)) for _, s, _, _ in head_param_specs(cfg))
    assert sum(b.numel() for b in h.grads.bucket.values()) == h.grads.flat.numel()


def test_softmax_refusals_come_before_any_device_use(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("allocated before refusing")
    monkeypatch.setattr(torch, "zeros", boom)
    monkeypatch.setattr(torch, "empty", boom)
    monkeypatch.setattr(torch, "full", boom)
    with pytest.raises(K.KernelError, match="does not take a softmax head.*sigmoid-shaped"):
        DistillHeads(HeadConfig(softmax=True), N=1, shapes=SHAPES, device="cuda")
    with pytest.raises(K.KernelError, match="DistillHeadsF16.*softmax"):
        DistillHeadsF16(HeadConfig(softmax=True), N=1, shapes=SHAPES, device="cuda", distill=False)
    with pytest.raises(K.KernelError, match="softmax"):
        DistillHeadsF16(HeadConfig(softmax=True), N=1, shapes=SHAPES, device="cuda")
    # the cited text is the builder's
    with pytest.raises(rh.SoftmaxDistillError, match="does not take a softmax head.*sigmoid-shaped"):
        rh.add_distill_loss(rh.HeadModel(HeadConfig(softmax=True), train=True))


@pytest.mark.parametrize("distill", [True, False])
def test_sigmoid_head_is_unchanged(distill):
    cfg = HeadConfig(num_gpus=1)
    specs = head_param_specs(cfg)
    assert specs[0] == ("retnet_cls_pred_fpn3_w", (720, 256, 3, 3), False, "late")
    assert specs[1] == ("retnet_cls_pred_fpn3_b", (720,), True, "late")
    assert len(specs) == 20 and specs[2][1] == (36, 256, 3, 3)
    h = DistillHeads(cfg, N=1, shapes=SHAPES[:2], device="cpu", distill=distill)
    want = [PR.POW_SUM, PR.CLS_LOSSES_FUSED, PR.SMOOTH_L1] if distill else [PR.FOCAL_FWD, PR.FOCAL_BWD, PR.SMOOTH_L1]
    assert _codes(h, "losses", "backward") == want
    assert PR.SOFTMAX_FOCAL_FUSED not in [o.code for o in h.prog.ops]
    assert h.C == 80 and tuple(h.cls_logits[0].shape) == (1, 720, 10, 14)
    assert float(h.params.flat.abs().sum()) == 0.0                  # default initialisation: zeros, as before
    fp = [o for o in h.prog.ops if o.code in (PR.FOCAL_FWD, PR.CLS_LOSSES_FUSED)][0]
    params = ctypes.cast(fp.p[2 if not distill else 4], ctypes.POINTER(K.FocalParams))[0]
    assert params.num_classes == 80


def test_fused_entry_points_are_exported_and_check_their_arguments():
    raw = ctypes.CDLL(K.LIB_PATH)
    assert hasattr(raw, "ssad_softmax_focal_loss_fused") and hasattr(raw, "ssad_softmax_focal_loss_fused_workspace_bytes")
    assert raw.ssad_kernels_abi_version() == 3
    L = K.lib()
    nb1, nb5 = (L.ssad_softmax_focal_loss_fused_workspace_bytes(n) for n in (1, 5))
    assert nb1 == L.ssad_softmax_focal_loss_workspace_bytes(1) and nb5 == 5 * nb1 and nb1 == 8 * 1024
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    N, A, Cn, H, W = 1, 2, 5, 3, 4
    BAD, WS = -1, -2

    def level(**kw):
        d = dict(logits=p.value, labels=p.value, prob=0, out=p.value, N=N, D=A * Cn, H=H, W=W)
        d.update(kw)
        return (K.SoftmaxFocalLevel * 1)(K.SoftmaxFocalLevel(**d))

    def run(arr, n=1, fg=p, Cc=Cn, scale=1.0, losses=p, ws=p, wsb=nb1):
        P = K.FocalParams(2.0, 0.25, Cc, scale)
        return L.ssad_softmax_focal_loss_fused(arr, n, fg, 1.0, ctypes.byref(P), losses, ws, wsb, None)

    assert run(None) == BAD                                                    # null table
    assert run(level(), Cc=1) == BAD and run(level(D=129 * A), Cc=129) == BAD  # C outside 2..128
    # 2 slabs x 1 chunk = 2 workgroups = 16 bytes
    assert run(level(), wsb=15) == WS and run(level(), ws=None) == WS
    assert run(level(logits=0)) == BAD and run(level(labels=0)) == BAD and run(level(out=0)) == BAD
    assert run(level(), fg=None) == BAD and run(level(), losses=None) == BAD
    assert run(level(D=A * Cn + 1)) == BAD and run(level(H=0)) == BAD and run(level(), scale=-1.0) == BAD
    assert run(level(), n=K.MAX_LEVELS + 1) == BAD and run(level(), n=-1) == BAD
    assert run(level(), n=0) == 0                                              # nothing to do, nothing launched
    # the existing pair still insists on its P pointer
    P = K.FocalParams(2.0, 0.25, Cn, 1.0)
    assert L.ssad_softmax_focal_loss_forward(level(), 1, p, ctypes.byref(P), p, nb1, None) == BAD
