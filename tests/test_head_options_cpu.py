"""RETINANET.SHARE_CLS_BBOX_TOWER and RETINANET.CLASS_SPECIFIC_BBOX without a GPU: the graph builder against the
reference's builder (tests/golden/head_graph_options.json, written by tests/golden/make_head_graph_options.py), the
parameter list, the records of the native program, the fp16 refusals, the engine rule for the wide bbox_pred, the
weights store, and the labeller fixture's shapes."""
import json
import os

import numpy as np
import pytest
import torch

import ssad_amd  # noqa: F401
from ssad_amd import kernels as K, program as PR
from ssad_amd.engines import Engine, Switches, subnet_engine, subnet_wgrad_split
from ssad_amd.head_pipeline import DistillHeads, DistillHeadsF16, head_param_specs
from ssad_amd.modeling import retinanet_heads as rh
from ssad_amd.modeling.retinanet_heads import HeadConfig

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]
SWITCHES = {"shared": dict(share_cls_bbox_tower=True), "class_specific": dict(class_specific_bbox=True),
            "both": dict(share_cls_bbox_tower=True, class_specific_bbox=True)}


def captures():
    return json.load(open(os.path.join(HERE, "golden", "head_graph_options.json")))


def op_signature(op):
    ja = op.to_jsonable()
    args = {a["name"]: a.get("f", a.get("i", a.get("s"))) for a in ja["arg"]}
    if op.engine:
        args["engine"] = op.engine
    return ja["type"], ja["input"], ja["output"], args


def same_args(mine, ref):
    if set(mine) != set(ref):
        return False
    for k, v in ref.items():
        if isinstance(v, str):
            if mine[k] != v:
                return False
        elif abs(float(mine[k]) - float(v)) > 1e-6 * max(1.0, abs(float(v))):
            return False
    return True


def build(kw, train=True, prefix=""):
    m = rh.HeadModel(HeadConfig(**kw), train=train)
    rh.add_fpn_retinanet_outputs(m, [prefix + "fpn_%d" % l for l in range(7, 2, -1)], 256, prefix)
    return m


# ---------------------------------------------------------------------------
# 1. the builder against the reference's
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(SWITCHES))
def test_builder_matches_the_reference_capture_op_by_op(key):
    g = captures()[key]
    kw = SWITCHES[key]
    assert (g["share_cls_bbox_tower"], g["class_specific_bbox"]) == (
        kw.get("share_cls_bbox_tower", False), kw.get("class_specific_bbox", False))
    m = build(kw)
    assert len(m.net.Proto().op) == g["student_head_op_count"]
    lg = rh.add_fpn_retinanet_losses(m)
    ops = m.net.Proto().op
    assert len(ops) == len(g["student_ops"])
    for mine, ref in zip(ops, g["student_ops"]):
        t, i, o, a = op_signature(mine)
        assert (t, i, o) == (ref["type"], ref["input"], ref["output"])
        assert same_args(a, ref["args"]), (t, a, ref["args"])
    assert lg == g["loss_gradients"] and m.losses == g["student_losses"]
    assert [p[0] for p in m.params] == [p["name"] for p in g["student_params"]]
    ref_params = {p["name"]: p for p in g["student_params"]}
    for name, shape, (filler, fkw) in m.params:
        assert shape == ref_params[name]["shape"] and filler == ref_params[name]["init"][0], name
        for k, v in ref_params[name]["init"][1].items():
            assert abs(fkw[k] - v) < 1e-6
    t = build(kw, train=False, prefix="teacher/")
    tops = t.net.Proto().op
    assert len(tops) == len(g["teacher_ops"])
    for mine, ref in zip(tops, g["teacher_ops"]):
        ty, i, o, a = op_signature(mine)
        assert (ty, i, o) == (ref["type"], ref["input"], ref["output"]) and same_args(a, ref["args"])


def test_builder_shapes_and_the_gradient_sum_of_the_shared_blob():
    cfg = HeadConfig(class_specific_bbox=True)
    assert cfg.bbox_regr_dim == 320 and HeadConfig().bbox_regr_dim == 4
    assert HeadConfig(num_classes=4, class_specific_bbox=True).bbox_regr_dim == 12
    m = build(SWITCHES["both"])
    names = [p[0] for p in m.params]
    assert not [n for n in names if "bbox_conv" in n] and len(names) == 12
    shapes = {p[0]: p[1] for p in m.params}
    assert shapes["retnet_bbox_pred_fpn3_w"] == [2880, 256, 3, 3] and shapes["retnet_bbox_pred_fpn3_b"] == [2880]
    by_out = {op.output[0]: op for op in m.net.Proto().op if op.type == "Conv"}
    for lvl in range(3, 8):
        assert by_out["retnet_bbox_pred_fpn%d" % lvl].input[0] == "retnet_cls_conv_n3_fpn%d" % lvl
    # the tower blob read by two convolutions gets the reference's gradient Sum
    lg = rh.add_fpn_retinanet_losses(m)
    n_fwd = len(m.net.Proto().op)
    grad_map = m.net.AddGradientOperators(lg)
    bwd = m.net.Proto().op[n_fwd:]
    hist = {}
    for op in bwd:
        hist[op.type] = hist.get(op.type, 0) + 1
    assert hist["ConvGradient"] == 30 and hist["ReluGradient"] == 20
    for lvl in range(3, 8):
        blob = "retnet_cls_conv_n3_fpn%d" % lvl
        s = [op for op in bwd if op.type == "Sum" and op.output == [blob + "_grad"]]
        assert len(s) == 1 and len(s[0].input) == 2, blob
    assert grad_map["fpn_3"] == "fpn_3_grad"
    # the defaults are today's graph
    d = build({})
    assert len(d.params) == 20 and {p[0]: p[1] for p in d.params}["retnet_bbox_pred_fpn3_w"] == [36, 256, 3, 3]


# ---------------------------------------------------------------------------
# 2. parameter list
# ---------------------------------------------------------------------------

def test_param_specs():
    default = head_param_specs(HeadConfig())
    assert len(default) == 20 and default[2] == ("retnet_bbox_pred_fpn3_w", (36, 256, 3, 3), False, "late")
    assert [s[0] for s in default[4:8]] == ["retnet_cls_conv_n3_fpn3_w", "retnet_cls_conv_n3_fpn3_b",
                                            "retnet_bbox_conv_n3_fpn3_w", "retnet_bbox_conv_n3_fpn3_b"]
    shared = head_param_specs(HeadConfig(share_cls_bbox_tower=True))
    assert len(shared) == 12 and not [s for s in shared if "bbox_conv" in s[0]]
    assert [s for s in shared if "bbox_conv" not in s[0]] == [s for s in default if "bbox_conv" not in s[0]]
    spec = head_param_specs(HeadConfig(class_specific_bbox=True))
    assert spec[2] == ("retnet_bbox_pred_fpn3_w", (2880, 256, 3, 3), False, "late")
    assert spec[3] == ("retnet_bbox_pred_fpn3_b", (2880,), True, "late")
    assert spec[:2] + spec[4:] == default[:2] + default[4:]
    both = head_param_specs(HeadConfig(num_classes=4, share_cls_bbox_tower=True, class_specific_bbox=True))
    assert len(both) == 12 and both[2][1] == (108, 256, 3, 3)
    # the graph builder and the native step own the same parameters
    for kw in SWITCHES.values():
        m = build(kw)
        assert sorted((p[0], tuple(p[1])) for p in m.params) == sorted((s[0], s[1]) for s in head_param_specs(HeadConfig(**kw)))


# ---------------------------------------------------------------------------
# 3. program structure
# ---------------------------------------------------------------------------

def record(o):
    return (o.code, o.klass, o.stream, tuple(o.i), tuple(o.f), tuple(o.l), tuple(bool(p) for p in o.p), o.work)


def tower_launches(h, lo, hi):
    ops = h.prog.ops[h.prog.marks[lo]:h.prog.marks[hi]]
    return [o for o in ops if o.code == PR.CONV3X3 and o.i[1] == h.D and o.i[2] == h.D]


@pytest.mark.parametrize("distill", [True, False], ids=["distill", "student_only"])
def test_switches_off_is_todays_program_record_for_record(distill):
    a = DistillHeads(N=2, shapes=SHAPES, device="cpu", distill=distill)
    b = DistillHeads(HeadConfig(share_cls_bbox_tower=False, class_specific_bbox=False), N=2, shapes=SHAPES, device="cpu",
                     distill=distill)
    assert [record(o) for o in a.prog.ops] == [record(o) for o in b.prog.ops]
    assert a.prog.marks == b.prog.marks and a._amax.next == b._amax.next
    assert [s[:2] for s in a.params.specs] == [s[:2] for s in b.params.specs]


@pytest.mark.parametrize("distill", [True, False], ids=["distill", "student_only"])
def test_shared_tower_program(distill):
    cfg = HeadConfig(num_classes=4, num_gpus=1)
    d = DistillHeads(cfg, N=2, shapes=SHAPES, device="cpu", distill=distill)
    s = DistillHeads(HeadConfig(num_classes=4, num_gpus=1, share_cls_bbox_tower=True), N=2, shapes=SHAPES, device="cpu",
                     distill=distill, shared_accumulate=False)
    assert s.shared_form == "two_pass" and d.shared_form is None
    # tower launches carry the classification problems only: half the rows, launch by launch
    for seg in (("forward", "losses"), ("backward", "sgd")):
        dl, sl = tower_launches(d, *seg), tower_launches(s, *seg)
        assert len(dl) == len(sl) == 4
        assert [o.i[0] for o in sl] == [o.i[0] // 2 for o in dl] and all(o.i[0] % 2 == 0 for o in dl)
    # buffers, filter packs and |max| words have no box tower
    for bufs in (s.act, s.dbuf, s.d_fpn):
        assert list(bufs) == ["cls"]
    if distill:
        assert list(s.t_buf) == ["cls"] and len(s.teacher.specs) == 12
    assert not [n for n in s.packed if "bbox_conv" in n] and len(s.packed) == 6 and len(d.packed) == 10

    def packed_entries(h):
        ops = h.prog.ops[h.prog.marks["pack"]:h.prog.marks["forward"]]
        return sum(o.i[0] for o in ops if o.code == PR.WINO_PACK_FILTERS) + sum(o.code == PR.PACK_FILTER for o in ops)
    assert packed_entries(d) - packed_entries(s) >= 4
    assert s._amax.next < d._amax.next
    own = {t.data_ptr() for group in (s.act["cls"] + s.dbuf["cls"] + [s.d_fpn["cls"], s.cls_logits, s.bbox_pred,
                                                                       s.d_cls_logits, s.d_bbox_pred, s.fpn_in,
                                                                       s.t_fpn_in]
                                      + ([b for b in s.t_buf["cls"]] + [s.t_prob, s.t_bbox] if distill else []))
           for t in group}
    assert {a for key in s._amax.word for a in key} <= own
    # bbox_pred reads the last classification activation, in the forward pass and in its filter gradient
    last = [t.data_ptr() for t in s.act["cls"][-1]]
    fwd = s.prog.ops[s.prog.marks["forward"]:s.prog.marks["losses"]]
    import ctypes
    bp = [o for o in fwd if o.code == PR.CONV3X3 and o.i[1] == 36]
    assert len(bp) == 1
    tab = ctypes.cast(bp[0].p[0], ctypes.POINTER(K.ConvLevel))
    assert [tab[l].x for l in range(5)] == last
    # backward: both prediction layers' data gradients unmasked into their own buffers, then Sum + ReluGradient per level
    bwd = s.prog.ops[s.prog.marks["backward"]:s.prog.marks["sgd"]]
    pred_dgrad = [o for o in bwd if o.code == PR.CONV3X3 and o.i[1] == s.D and o.i[2] in (27, 36)]
    assert [o.i[2] for o in pred_dgrad] == [27, 36] and all(o.i[3] & K.CONV_MASK_AUX == 0 for o in pred_dgrad)
    for o, t in zip(pred_dgrad, ("cls", "bbox")):
        tab = ctypes.cast(o.p[0], ctypes.POINTER(K.ConvLevel))
        assert [tab[l].y for l in range(5)] == [x.data_ptr() for x in s.d_shared[t]]
    sums = [o for o in bwd if o.code == PR.SUM_N]
    relus = [o for o in bwd if o.code == PR.RELU_GRAD]
    assert len(sums) == len(relus) == 5 and all(o.i[0] == 2 for o in sums)
    for l, (sm, rg) in enumerate(zip(sums, relus)):
        ptrs = ctypes.cast(sm.p[0], ctypes.POINTER(ctypes.c_void_p * 2))[0]
        assert list(ptrs) == [s.d_shared["cls"][l].data_ptr(), s.d_shared["bbox"][l].data_ptr()]
        assert sm.l[0] == rg.l[0] == s.d_shared["cls"][l].numel() and sm.p[1] == s.d_shared["sum"][l].data_ptr()
        assert (rg.p[0], rg.p[1], rg.p[2]) == (s.act["cls"][-1][l].data_ptr(), sm.p[1], s.dbuf["cls"][4][l].data_ptr())
        assert len({sm.p[1], rg.p[2]} | set(ptrs)) == 4                  # no operand of a launch aliases its output
    assert not [o for o in d.prog.ops if o.code in (PR.SUM_N, PR.RELU_GRAD)]
    assert 39 in PR.KLASS and {o.klass for o in sums + relus} == {39}
    # the first tower data gradient below reads the masked sum
    first = tower_launches(s, "backward", "sgd")[0]
    tab = ctypes.cast(first.p[0], ctypes.POINTER(K.ConvLevel))
    assert [tab[l].x for l in range(5)] == [t.data_ptr() for t in s.dbuf["cls"][4]]
    # SGD and the all-reduce buckets follow from the specs
    assert s.params.flat.numel() == sum(int(np.prod(sh)) for _, sh, _, _ in head_param_specs(s.cfg))
    assert sum(b.numel() for b in s.grads.bucket.values()) == s.grads.flat.numel()


@pytest.mark.parametrize("distill", [True, False], ids=["distill", "student_only"])
def test_shared_tower_accumulate_program(distill):
    """The default form where bbox_pred's data gradient runs on the F(2x4) engine: cls_pred's gradient lands unmasked
    (and without a |max| word: it is not final) in the buffer the tower's backward continues from, bbox_pred's adds itself
    under the mask in its epilogue; no SUM_N / RELU_GRAD records, no extra buffers."""
    import ctypes
    cfg = HeadConfig(num_classes=4, num_gpus=1, share_cls_bbox_tower=True)
    s = DistillHeads(cfg, N=2, shapes=SHAPES, device="cpu", distill=distill)          # the default (the A/B)
    two = DistillHeads(cfg, N=2, shapes=SHAPES, device="cpu", distill=distill, shared_accumulate=False)
    assert s.shared_form == "accumulate" and s.dgrad_engine["retnet_bbox_pred_fpn3"] == Engine.F24
    assert not hasattr(s, "d_shared") and not [o for o in s.prog.ops if o.code in (PR.SUM_N, PR.RELU_GRAD)]
    assert len(s.prog.ops) == len(two.prog.ops) - 10
    bwd = s.prog.ops[s.prog.marks["backward"]:s.prog.marks["sgd"]]
    c, b = [o for o in bwd if o.code == PR.CONV3X3 and o.i[1] == s.D and o.i[2] in (27, 36)]
    assert (c.i[2], c.i[3]) == (27, 0) and (b.i[2], b.i[3], b.i[4]) == (36, K.CONV_MASK_AUX | K.CONV_ACCUM_AUX, Engine.F24)
    out = [t.data_ptr() for t in s.dbuf["cls"][4]]
    for o in (c, b):
        tab = ctypes.cast(o.p[0], ctypes.POINTER(K.ConvLevel))
        assert [tab[l].y for l in range(5)] == out
    tab = ctypes.cast(b.p[0], ctypes.POINTER(K.ConvLevel))
    assert [tab[l].aux for l in range(5)] == [t.data_ptr() for t in s.act["cls"][-1]]
    assert bwd.index(c) < bwd.index(b)
    if c.i[4] == Engine.SPLIT:
        assert not c.p[5]                                  # no |max| word folded for the partial sum
    assert tuple(out) not in s._amax.word or s._amax.word[tuple(out)] is not None
    # a bbox_pred whose data gradient is on another engine keeps the two-pass form
    wide = DistillHeads(HeadConfig(num_gpus=1, share_cls_bbox_tower=True, class_specific_bbox=True), N=1, shapes=[(8, 12)],
                        device="cpu", distill=False, shared_accumulate=True)
    assert wide.dgrad_engine["retnet_bbox_pred_fpn3"] == Engine.SPLIT and wide.shared_form == "two_pass"
    # the flag is the F(2x4) launcher's alone and needs the mask
    L = K.lib()
    lv = (K.ConvLevel * 1)()
    assert L.ssad_conv3x3_forward_wino24(lv, 1, None, None, 256, 36, K.CONV_ACCUM_AUX, None) != 0
    assert L.ssad_conv3x3_forward_wino24(lv, 1, None, None, 256, 36, K.CONV_ACCUM_AUX | K.CONV_MASK_AUX | K.CONV_RELU, None) != 0


@pytest.mark.parametrize("kw", [dict(distill=False, softmax=True), dict(distill=True, teacher_fpn_dim=256, fpn_dim=128),
                                dict(distill=True, both=True), dict(distill=False, both=True)],
                         ids=["softmax", "thin_student", "both_distill", "both_student_only"])
def test_combinations_build(kw):
    cfg = HeadConfig(num_classes=4, num_gpus=1, share_cls_bbox_tower=True, softmax=kw.get("softmax", False),
                     class_specific_bbox=kw.get("both", False), fpn_dim=kw.get("fpn_dim", 256))
    h = DistillHeads(cfg, N=2, shapes=SHAPES, device="cpu", distill=kw["distill"], teacher_fpn_dim=kw.get("teacher_fpn_dim"))
    assert list(h.act) == ["cls"] and len(h.params.specs) == 12
    assert tuple(h.bbox_pred[0].shape) == (2, 9 * (12 if kw.get("both") else 4), 16, 24)
    if kw.get("teacher_fpn_dim"):
        assert h.Dt == 256 and h.D == 128 and tuple(h.teacher["retnet_bbox_pred_fpn3_w"].shape) == (36, 256, 3, 3)
        assert tuple(h.params["retnet_bbox_pred_fpn3_w"].shape) == (36, 128, 3, 3)


def test_class_specific_program_and_engine_rule():
    cfg = HeadConfig(num_gpus=1, class_specific_bbox=True)
    h = DistillHeads(cfg, N=1, shapes=[(8, 12)], device="cpu", distill=False)
    R = 2880
    assert tuple(h.params["retnet_bbox_pred_fpn3_w"].shape) == (R, 256, 3, 3)
    assert tuple(h.bbox_pred[0].shape) == tuple(h.d_bbox_pred[0].shape) == (1, R, 8, 12)
    wg = [o for o in h.prog.ops if o.code == PR.CONV3X3_WGRAD][:2]
    assert [(o.i[1], o.i[2]) for o in wg] == [(720, 256), (R, 256)]
    assert wg[1].klass == (40 if wg[1].i[4] else 7) and "split" in PR.KLASS[40]["name"]
    # the one place that decides: the wide layer goes where cls_pred goes, the 36-wide one stays where it was
    sw = Switches.read({}).for_subnets(True)
    name = "retnet_bbox_pred_fpn3"
    assert subnet_engine(sw, "student", name, 36, 256, "fwd") == Engine.F22
    assert subnet_engine(sw, "student", name, 36, 256, "dgrad") == Engine.F24
    assert subnet_engine(sw, "student", name, 108, 256, "fwd") == Engine.F22
    for who in ("student", "teacher"):
        assert subnet_engine(sw, who, name, R, 256, "fwd") == subnet_engine(sw, who, "retnet_cls_pred_fpn3", 720, 256, "fwd") \
            == Engine.SPLIT
    assert subnet_engine(sw, "student", name, R, 256, "dgrad") == Engine.SPLIT
    assert K.lib().ssad_conv_split_filter_floats(R, 256) > 0 and K.lib().ssad_conv_split_filter_floats(256, R) > 0
    assert subnet_wgrad_split(sw, R, 256) and not subnet_wgrad_split(sw, 36, 256)
    off = Switches.read({"SSAD_SPLIT_CONV": "0"}).for_subnets(True)
    assert subnet_engine(off, "student", name, R, 256, "fwd") == Engine.F24
    assert subnet_engine(Switches.read({"SSAD_CONV_ENGINE": "direct"}).for_subnets(True), "student", name, R, 256,
                         "fwd") == Engine.DIRECT
    assert h.fwd_engine["student", name] == Engine.SPLIT and h.dgrad_engine[name] == Engine.SPLIT
    fwd = [o for o in h.prog.ops[h.prog.marks["forward"]:h.prog.marks["losses"]] if o.code == PR.CONV3X3 and o.i[1] == R]
    assert len(fwd) == 1 and fwd[0].i[4] == Engine.SPLIT and fwd[0].klass == 31 and 31 in PR.KLASS and 30 in PR.KLASS


# ---------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------

def test_fp16_refusals_come_before_any_allocation(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("allocated before refusing")
    monkeypatch.setattr(torch, "zeros", boom)
    monkeypatch.setattr(torch, "empty", boom)
    monkeypatch.setattr(torch, "full", boom)
    for switch in ("share_cls_bbox_tower", "class_specific_bbox"):
        for distill in (True, False):
            with pytest.raises(K.KernelError, match="DistillHeadsF16.*%s" % switch):
                DistillHeadsF16(HeadConfig(**{switch: True}), N=1, shapes=SHAPES, device="cuda", distill=distill)


def test_detector_and_labeller_reject_non_boolean_switches():
    from ssad_amd.roi_data.retinanet import RetinanetDetector, RetinanetLabeler
    with pytest.raises(K.KernelError, match="class_specific_bbox"):
        RetinanetDetector([(2, 3)], class_specific_bbox=1, device="cpu")
    with pytest.raises(K.KernelError, match="class_specific_bbox"):
        RetinanetLabeler(1, 4, 64, 64, class_specific_bbox="yes", device="cpu")


def test_new_entry_points_check_their_arguments():
    import ctypes as C
    L = K.lib()
    assert L.ssad_kernels_abi_version() == 3
    fs = (C.c_int * 1)(8)
    # a switch value other than 0 / 1 is refused before anything is read
    rc = L.ssad_retinanet_anchor_labels_ex(None, 1, 9, 3, fs, fs, fs, None, None, None, 0, 0, 81, C.c_float(0.5),
                                           C.c_float(0.4), None, None, None, 0, None, None, None, C.c_size_t(0), None, 2)
    assert rc != 0
    H = (C.c_int * 1)(2)
    rc = L.ssad_retinanet_detect_class_specific(None, None, None, 1, 9, 3, 3, H, H, C.c_float(0.05), 10, C.c_float(0.5),
                                                5, C.c_float(1.0), 32, 32, C.c_float(4.0), None, None, None,
                                                C.c_size_t(0), None, None, 1)
    assert rc != 0


# ---------------------------------------------------------------------------
# 5. weights files
# ---------------------------------------------------------------------------

def test_weights_files_take_the_new_shapes(tmp_path):
    from ssad_amd.utils import net as nu
    sep = nu.HeadParamStore(HeadConfig(num_classes=4, fpn_dim=32)).fill(seed=3)
    shared = nu.HeadParamStore(HeadConfig(num_classes=4, fpn_dim=32, share_cls_bbox_tower=True))
    assert len(sep.params.specs) == 20 and len(shared.params.specs) == 12
    assert not [n for n, _, _, _ in shared.params.specs if "bbox_conv" in n]
    f = str(tmp_path / "separate.pkl")
    nu.save_model_to_weights_file(f, sep)
    # a separate-tower file into shared heads: everything the heads own is loaded, the box tower rides along
    loaded, missing = nu.initialize_from_weights_file(shared, f)
    assert sorted(loaded) == sorted(n for n, _, _, _ in shared.params.specs) and not missing
    kept = [k for k in shared.preserved if "bbox_conv" in k]
    assert len(kept) == 8 and np.array_equal(shared.preserved["retnet_bbox_conv_n2_fpn3_w"],
                                             sep.params["retnet_bbox_conv_n2_fpn3_w"].numpy())
    assert torch.equal(shared.params["retnet_bbox_pred_fpn3_w"], sep.params["retnet_bbox_pred_fpn3_w"])
    g = str(tmp_path / "shared.pkl")
    nu.save_model_to_weights_file(g, shared)
    again = nu.HeadParamStore(HeadConfig(num_classes=4, fpn_dim=32))
    loaded, missing = nu.initialize_from_weights_file(again, g)
    assert not missing and torch.equal(again.params["retnet_bbox_conv_n2_fpn3_w"], sep.params["retnet_bbox_conv_n2_fpn3_w"])
    # a class-specific head round trip, and the other layout's bbox_pred refused by name and both shapes
    spec = nu.HeadParamStore(HeadConfig(num_classes=4, fpn_dim=32, class_specific_bbox=True)).fill(seed=4)
    assert tuple(spec.params["retnet_bbox_pred_fpn3_w"].shape) == (108, 32, 3, 3)
    h = str(tmp_path / "specific.pkl")
    nu.save_model_to_weights_file(h, spec)
    back = nu.HeadParamStore(HeadConfig(num_classes=4, fpn_dim=32, class_specific_bbox=True))
    loaded, missing = nu.initialize_from_weights_file(back, h)
    assert not missing and torch.equal(back.params["retnet_bbox_pred_fpn3_w"], spec.params["retnet_bbox_pred_fpn3_w"])
    with pytest.raises(nu.BboxPredWidthError, match=r"retnet_bbox_pred_fpn3_w.*\(108, 32, 3, 3\).*\(36, 32, 3, 3\)"):
        nu.initialize_from_weights_file(nu.HeadParamStore(HeadConfig(num_classes=4, fpn_dim=32)), h)
    with pytest.raises(nu.BboxPredWidthError, match=r"retnet_bbox_pred_fpn3_w.*\(36, 32, 3, 3\).*\(108, 32, 3, 3\)"):
        nu.initialize_from_weights_file(back, f)
    # the native heads load the same files
    hd = DistillHeads(HeadConfig(num_classes=4, fpn_dim=32, share_cls_bbox_tower=True), N=1, shapes=SHAPES[2:], device="cpu",
                      distill=False)
    loaded, missing = nu.initialize_from_weights_file(hd, f)
    assert not missing and len(loaded) == 12 and len([k for k in hd.preserved if "bbox_conv" in k]) == 8


# ---------------------------------------------------------------------------
# 6. the labeller fixture (tests/golden/make_anchor_labels_class_specific.py)
# ---------------------------------------------------------------------------

def test_class_specific_labeller_fixture_shapes():
    z = np.load(os.path.join(HERE, "golden", "anchor_labels_class_specific_ref.npz"))
    C_ = int(z["num_classes"])
    H, W = [int(v) for v in z["image_hw"]]
    assert C_ == 81
    seen, rows = set(), 0
    for lvl in range(3, 8):
        lab = z["blob_retnet_cls_labels_fpn%d" % lvl]
        locs = z["blob_retnet_roi_fg_bbox_locs_fpn%d" % lvl]
        tg = z["blob_retnet_roi_bbox_targets_fpn%d" % lvl]
        assert lab.dtype == np.int32 and lab.shape == (2, 9, H >> lvl, W >> lvl)
        assert locs.dtype == tg.dtype == np.float32 and locs.shape == tg.shape and locs.shape[1] == 4
        rows += locs.shape[0]
        ch = locs[:, 1].astype(int)
        assert np.all(ch % 4 == 0) and np.all(ch < 4 * (C_ - 1) * 9)
        a, cls = ch // (4 * (C_ - 1)), ch % (4 * (C_ - 1)) // 4 + 1
        inside = (locs[:, 2] < lab.shape[2]) & (locs[:, 3] < lab.shape[3])
        for r, ai, ci in zip(locs[inside], a[inside], cls[inside]):
            assert lab[int(r[0]), ai, int(r[2]), int(r[3])] == ci        # the column addresses the anchor's class
        seen |= set(cls.tolist())
    assert rows > 100 and {1, C_ - 1} <= seen and len(seen - {1, C_ - 1}) >= 1
    assert z["blob_retnet_fg_num"].dtype == np.float32
