"""Thin students (RESNETS.CHANNEL_RATIO) without a GPU: the graph builder against captures of the imported
reference builder run at ratio 0.5 and 0.25 (tests/golden/make_thin_graph.py), the width arithmetic, the
scope errors, and weights files at the scaled dims (utils/net.py)."""
import json
import os
import pickle
from collections import OrderedDict

import numpy as np
import pytest
import torch

import ssad_amd  # noqa: F401
from ssad_amd import kernels as K
from ssad_amd.modeling import resnet_fpn as rf
from ssad_amd.modeling import retinanet_heads as rh
from ssad_amd.utils import net

from torch_ref_thin import reference_widths

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THIN = {0.5: "thin_graph_r50_fpn_ratio50.json", 0.25: "thin_graph_r50_fpn_ratio25.json"}


def _args(op):
    got = {}
    for a in op.arg:
        if a.HasField("i"):
            got[a.name] = a.i
        elif a.HasField("s"):
            got[a.name] = a.s.decode() if isinstance(a.s, bytes) else a.s
        elif a.HasField("f"):
            got[a.name] = a.f
    return got


def _same_ops(ops, ref_ops):
    assert len(ops) == len(ref_ops)
    for mine, ref in zip(ops, ref_ops):
        assert mine.type == ref["type"]
        assert list(mine.input) == ref["input"] and list(mine.output) == ref["output"], ref
        want = {k: (int(v) if isinstance(v, bool) else v) for k, v in ref["args"].items()}
        engine = want.pop("engine", "")          # a field of OperatorDef, not an argument
        assert (mine.engine or "") == engine
        assert _args(mine) == want, (ref, _args(mine))


def _plain(init):
    kw = {k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in init[1].items()}
    return [init[0], kw]


@pytest.mark.parametrize("ratio", [0.5, 0.25])
def test_thin_body_and_subnets_match_the_reference_capture(ratio):
    """Op for op, blob for blob and shape for shape what ResNet.py / FPN.py / retinanet_heads.py emit with
    RESNETS.CHANNEL_RATIO = ratio; the subnets take their width from the body (dim_in)."""
    g = json.load(open(os.path.join(GOLDEN, THIN[ratio])))
    assert g["channel_ratio"] == ratio
    body_cfg = rf.BodyConfig(channel_ratio=ratio)
    model = rf.BodyModel(body_cfg)
    blobs, dim, scales = rf.add_fpn_resnet_conv5_body(model)
    assert [str(b) for b in blobs] == g["fpn_blobs"] and dim == g["fpn_dim"] == int(256 * ratio)
    assert scales == g["spatial_scales"]
    _same_ops(model.net.Proto().op, g["ops"])
    assert [(n, s, [i[0], i[1]]) for n, s, i in model.params] == [(p["name"], p["shape"], p["init"]) for p in g["params"]]
    hcfg = rh.HeadConfig.for_body(body_cfg)
    assert hcfg.fpn_dim == dim
    heads = rh.HeadModel(hcfg, train=True)
    rh.add_fpn_retinanet_outputs(heads, [str(b) for b in blobs])
    _same_ops(heads.net.Proto().op, g["head_ops"])
    mine = [(n, list(s), _plain(i)) for n, s, i in heads.params]
    want = [(p["name"], p["shape"], p["init"]) for p in g["head_params"]]
    assert [(n, s) for n, s, _ in mine] == [(n, s) for n, s, _ in want]
    for (_, _, a), (_, _, b) in zip(mine, want):
        assert a[0] == b[0] and set(a[1]) == set(b[1])
        assert all(abs(a[1][k] - b[1][k]) <= 1e-6 * max(1.0, abs(b[1][k])) for k in b[1])


def test_ratio_one_passed_explicitly_is_the_existing_capture():
    g = json.load(open(os.path.join(GOLDEN, "backbone_graph_r50_fpn.json")))
    model = rf.BodyModel(rf.BodyConfig(channel_ratio=1.0))
    blobs, dim, scales = rf.add_fpn_resnet_conv5_body(model)
    assert [str(b) for b in blobs] == g["fpn_blobs"] and dim == g["fpn_dim"] and scales == g["spatial_scales"]
    _same_ops(model.net.Proto().op, g["ops"])
    assert [(n, s, [i[0], i[1]]) for n, s, i in model.params] == [(p["name"], p["shape"], p["init"]) for p in g["params"]]


@pytest.mark.parametrize("ratio", [0.25, 0.5, 0.75, 1.0])
def test_width_table_is_the_references_arithmetic(ratio):
    """Stem 64 unscaled; inner width truncated once, then doubled per stage; stage outputs and the FPN dimension
    truncated each -- in the builder's table and in the native backbone's layer table."""
    from ssad_amd.backbone_pipeline import NativeResNetFPN
    inner, stage, D = reference_widths(ratio)
    w = rf.channel_widths(ratio)
    assert w.stem == 64 and list(w.inner) == inner and list(w.stage) == stage and w.fpn_dim == D
    assert all(c > 0 and c % 16 == 0 for c in inner + stage + [D])
    sh = NativeResNetFPN.layer_shapes("r50", ratio)
    assert sh["stem.0"] == (64, 3, 7, 7)
    for si in range(4):
        pre = "res%d.0" % (si + 2)
        cin = 64 if si == 0 else stage[si - 1]
        assert sh[pre + ".c1"] == (inner[si], cin, 1, 1)
        assert sh[pre + ".c2"] == (inner[si], inner[si], 3, 3)
        assert sh[pre + ".c3"] == (stage[si], inner[si], 1, 1)
        assert ((pre + ".proj") in sh) == (si > 0 or cin != stage[si])
        assert sh["res%d.1.c1" % (si + 2)] == (inner[si], stage[si], 1, 1)
    assert sh["lat.0"] == (D, stage[3], 1, 1) and sh["lat.1"] == (D, stage[2], 1, 1) and sh["lat.2"] == (D, stage[1], 1, 1)
    assert sh["out.0"] == sh["out.2"] == sh["p7"] == (D, D, 3, 3) and sh["p6"] == (D, stage[3], 3, 3)


def test_truncation_happens_once_for_the_inner_width():
    """ResNet.py:99 truncates the inner width once and doubles it per stage: at 0.3, res5's inner width is
    int(64 * 0.3) * 8 = 152, where truncating per stage would give int(512 * 0.3) = 153."""
    w = rf.channel_widths(0.3, check=False)
    assert w.inner == (19, 38, 76, 152) and w.stage == (76, 153, 307, 614) and w.fpn_dim == 76


def test_unsupported_ratios_raise_before_the_library_is_touched(monkeypatch):
    from ssad_amd import backbone_pipeline as BP
    from ssad_amd.backbone_f16 import NativeResNetFPNF16

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(K, "lib", no_lib)
    with pytest.raises(rf.ChannelRatioError, match="0.3"):
        rf.add_fpn_resnet_conv5_body(rf.BodyModel(rf.BodyConfig(channel_ratio=0.3)))
    for bad in (0.3, 0.125, 0.0, 2.0):
        with pytest.raises(K.KernelError, match="multiple of 16"):
            BP.NativeResNetFPN("r50", 1, (128, 128), "cpu", channel_ratio=bad)
    with pytest.raises(K.KernelError, match="fp16"):
        NativeResNetFPNF16("r50", 1, (128, 128), "cpu", channel_ratio=0.5)
    with pytest.raises(K.KernelError, match="grouped"):
        BP.NativeResNetFPN("x101-64x4d", 1, (128, 128), "cpu", train=False, channel_ratio=0.5)

    class FakeHeads(object):
        F16, blocked_io, distill, D, Dt = True, True, True, 128, 256
        lr = torch.zeros(1)
    with pytest.raises(K.KernelError, match="fp16"):
        BP.NativeDistillModel(FakeHeads(), "r50", "r50", 1, (128, 128), "cpu", student_channel_ratio=0.5)
    FakeHeads.F16 = False
    with pytest.raises(K.KernelError, match="multiple of 16"):
        BP.NativeDistillModel(FakeHeads(), "r50", "r50", 1, (128, 128), "cpu", student_channel_ratio=0.3)
    with pytest.raises(K.KernelError, match="FPN dimension 128"):
        BP.NativeDistillModel(FakeHeads(), "r50", "r50", 1, (128, 128), "cpu", student_channel_ratio=0.25)


def test_quarter_width_reference_quirk_is_pinned():
    """ResNet.py:173-175 tells the first stage by dim_in == 64; at ratio 0.25 res2 leaves 64 channels too, so
    the reference's res3_0 has stride 1 and res2_0 no projection.  The graph builder restates the capture; the
    native backbone strides by stage index (its levels stay at strides 8..128, where the anchors are)."""
    from ssad_amd.backbone_pipeline import NativeResNetFPN
    g = json.load(open(os.path.join(GOLDEN, THIN[0.25])))
    conv = {o["output"][0]: o for o in g["ops"] if o["type"] == "Conv"}
    assert conv["res3_0_branch2a"]["args"]["stride"] == 1 and conv["res4_0_branch2a"]["args"]["stride"] == 2
    assert "res2_0_branch1" not in conv
    nat = NativeResNetFPN.__new__(NativeResNetFPN)
    nat.arch, nat.train = "r50", True
    from ssad_amd.backbone_pipeline import student_widths
    nat.widths = student_widths("r50", 0.25)
    nat.D, nat._layers = nat.widths.fpn_dim, OrderedDict()
    nat._define_layers()
    assert nat._layers["res3.0.c1"].stride == 2 and "res2.0.proj" not in nat._layers
    assert "res2.0.proj" not in net.backbone_blob_names("r50", 0.25)
    assert "res2.0.proj" in net.backbone_blob_names("r50", 0.5)


def _thin_blobs(ratio, rng):
    """A weights-file body in the REFERENCE's layout at the captured thin shapes (as tests/test_weights_file.py
    builds the full-width one)."""
    g = json.load(open(os.path.join(GOLDEN, THIN[ratio])))
    blobs = OrderedDict()
    for prm in g["params"]:
        name, shape = prm["name"], tuple(prm["shape"])
        if name.endswith("_bn_s"):
            v = rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape, p=[0.1, 0.9])
        elif name.endswith("_b"):
            v = rng.standard_normal(shape) * 0.05
        else:
            v = rng.standard_normal(shape) * np.sqrt(2.0 / int(np.prod(shape[1:])))
        blobs[name] = v.astype(np.float32)
        if name.startswith("fpn_") or (name.endswith("_w") and name[:4] in ("res3", "res4", "res5")):
            blobs[name + "_momentum"] = (rng.standard_normal(shape) * 1e-3).astype(np.float32)
    return blobs


@pytest.mark.parametrize("ratio", [0.5, 0.25])
def test_thin_weights_file_round_trip_cpu(tmp_path, ratio):
    """Reference layout at the scaled dims -> folded native parameters (W' = s W, m' = s m) -> file -> reference
    layout: names, AffineChannel blobs exactly, filters and momentum to the rounding of fold / un-fold."""
    from ssad_amd.backbone_pipeline import NativeResNetFPN
    blobs = _thin_blobs(ratio, np.random.default_rng(3))
    names = net.backbone_blob_names("r50", ratio)
    assert set(n for t in names.values() for n in t if n is not None) == \
        set(k for k in blobs if not k.endswith("_momentum"))
    state, scales, moms, missing = net.backbone_from_blobs(blobs, "r50", channel_ratio=ratio)
    assert not missing
    w, sc = blobs["res4_1_branch2b_w"], blobs["res4_1_branch2b_bn_s"]
    assert w.shape == (int(64 * ratio) * 4,) * 2 + (3, 3)
    assert np.array_equal(state["res4.1.c2.weight"].numpy(), w * sc.reshape(-1, 1, 1, 1))
    assert np.array_equal(moms["res4.1.c2.weight"].numpy(),
                          blobs["res4_1_branch2b_w_momentum"] * sc.reshape(-1, 1, 1, 1))
    nat = NativeResNetFPN("r50", 1, (128, 128), "cpu", train=True, src=state, affine_scales=scales,
                          channel_ratio=ratio)
    net.load_backbone(nat, blobs)
    assert not nat.missing_blobs
    l = nat._layers["res4.1.c2"]
    assert np.allclose(l.s2.numpy(), sc * sc, rtol=1e-6)
    off = (l.w.data_ptr() - nat.params_flat.data_ptr()) // 4
    assert np.array_equal(nat.moms_flat[off:off + l.w.numel()].view_as(l.w).numpy(), moms["res4.1.c2.weight"].numpy())
    path = str(tmp_path / "thin.pkl")
    with open(path, "wb") as f:
        pickle.dump(dict(blobs=dict(net.backbone_to_blobs(nat)), cfg=""), f, protocol=2)
    out, _ = net._blobs_and_cfg(net.load_object(path))
    assert set(out) == set(blobs)
    for k, v in blobs.items():
        assert out[k].shape == v.shape, k
        if k.endswith("_bn_s") or k.endswith("_b") or k.startswith("fpn_"):
            assert np.array_equal(out[k], v), k
        else:
            assert np.allclose(out[k], v, rtol=3e-7, atol=1e-12), k
    again = NativeResNetFPN("r50", 1, (128, 128), "cpu", train=True, src=state, affine_scales=scales,
                            channel_ratio=ratio)
    net.load_backbone(again, out)
    assert torch.equal(again.params_flat, nat.params_flat) and torch.equal(again.frozen_flat, nat.frozen_flat)
    assert torch.allclose(again.moms_flat, nat.moms_flat, rtol=3e-7, atol=1e-12)


def test_full_width_file_into_half_width_model_raises_the_named_error():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_weights_file import reference_backbone_blobs
    from ssad_amd.backbone_pipeline import NativeResNetFPN
    full, _ = reference_backbone_blobs("r50", np.random.default_rng(5))
    with pytest.raises(net.WeightsWidthError) as e:
        net.backbone_from_blobs(full, "r50", channel_ratio=0.5)
    msg = str(e.value)
    assert "res2_0_branch2a_w" in msg and "(64, 64, 1, 1)" in msg and "(32, 64, 1, 1)" in msg and "0.5" in msg
    half = _thin_blobs(0.5, np.random.default_rng(6))
    state, scales, _, _ = net.backbone_from_blobs(half, "r50", channel_ratio=0.5)
    nat = NativeResNetFPN("r50", 1, (128, 128), "cpu", train=True, src=state, affine_scales=scales, channel_ratio=0.5)
    before = nat.params_flat.clone()
    for strict in (False, True):
        with pytest.raises(net.WeightsWidthError):
            net.load_backbone(nat, full, strict=strict)
    assert torch.equal(nat.params_flat, before)
    with pytest.raises(net.WeightsWidthError, match=r"\(32, 64, 1, 1\).*\(64, 64, 1, 1\)"):
        net.backbone_from_blobs(half, "r50")                       # and a thin file into the full-width network
    assert issubclass(net.WeightsWidthError, ValueError)


def test_subnet_parameters_follow_the_fpn_dimension():
    from ssad_amd.head_pipeline import head_param_specs
    specs = dict((n, s) for n, s, _, _ in head_param_specs(rh.HeadConfig(fpn_dim=128)))
    assert specs["retnet_cls_pred_fpn3_w"] == (720, 128, 3, 3) and specs["retnet_bbox_pred_fpn3_w"] == (36, 128, 3, 3)
    assert specs["retnet_cls_conv_n0_fpn3_w"] == (128, 128, 3, 3)
