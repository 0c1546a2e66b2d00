"""ResNeXt-101-32x8d as a native teacher, the parts that need no device: the body graph against the reference
builder's capture (tests/golden/make_backbone_graph_32x8d.py), the network's layer shapes and weights-file names,
the grouped kernel's entry points at 64 channels per group, the refusals, and the program's records."""
import ctypes
import json
import os
from collections import Counter

import numpy as np
import pytest
import torch

import ssad_amd  # noqa: F401
from ssad_amd import backbone_pipeline as BP, kernels as K, program as PR
from ssad_amd.utils import net

from test_boundary_cpu import test_backbone_graph_matches_reference_capture as graph_matches_capture

ARCH = "x101-32x8d"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAPTURE = "backbone_graph_x101_32x8d_fpn.json"


@pytest.fixture(scope="module")
def capture():
    return json.load(open(os.path.join(GOLDEN, CAPTURE)))


def test_body_graph_matches_the_reference_capture(capture):
    """RESNETS.STRIDE_1X1 False, NUM_GROUPS 32, WIDTH_PER_GROUP 8 under add_fpn_ResNet101_conv5_body: op for op and
    parameter for parameter (the comparison of test_boundary_cpu's own test, on the new capture)."""
    assert capture["resnets"] == {"STRIDE_1X1": False, "NUM_GROUPS": 32, "WIDTH_PER_GROUP": 8}
    graph_matches_capture(CAPTURE, dict(block_counts=(3, 4, 23, 3), stride_1x1=False, num_groups=32,
                                        width_per_group=8))


def test_layer_shapes_agree_with_the_capture(capture):
    shapes = BP.NativeResNetFPN.layer_shapes(ARCH)
    names = net.backbone_blob_names(ARCH)
    ref = {p["name"]: tuple(p["shape"]) for p in capture["params"]}
    mine = [n for t in names.values() for n in t if n is not None]
    assert len(mine) == len(set(mine)) and set(mine) == set(ref)
    assert set(shapes) == set(names)
    for layer, (wn, sn, bn) in names.items():
        assert ref[wn] == shapes[layer], (layer, wn)
        assert ref[bn] == (shapes[layer][0],) and (sn is None or ref[sn] == (shapes[layer][0],))
    assert shapes["res5.0.c2"] == (2048, 64, 3, 3) and shapes["res2.0.c2"] == (256, 8, 3, 3)
    nat = BP.NativeResNetFPN.__new__(BP.NativeResNetFPN)
    nat.arch, nat.train, nat.D = ARCH, False, 256
    nat._layers = type(shapes)()
    nat._define_layers()
    l = nat._layers["res5.0.c2"]
    assert (l.group, l.stride, l.cin, l.cout) == (32, 2, 2048, 2048)
    assert nat._layers["res5.0.c1"].stride == 1 and nat._layers["res5.1.c2"].stride == 1
    assert sum(1 for l in nat._layers.values() if l.group > 1) == 33


def test_entry_points_at_64_channels_per_group_without_a_device():
    L = K.lib()
    assert L.ssad_grouped_conv3x3_filter_floats(2048, 32) == 2048 * 64 * 9
    assert L.ssad_grouped_conv3x3_filter_floats(128, 2) == 128 * 64 * 9
    assert L.ssad_grouped_conv3x3_filter_floats(256, 2) == -1           # cg 128
    assert L.ssad_grouped_conv3x3_filter_floats(24, 2) == -1            # cg 12
    assert L.ssad_grouped_conv3x3_filter_floats(256, 64) == 64 * 9 * 64
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd = L.ssad_grouped_conv3x3_forward
    assert fwd(None, p, None, 1, 128, 4, 4, 2, 1, 0, p, None) == -1     # no input
    assert fwd(p, None, None, 1, 128, 4, 4, 2, 1, 0, p, None) == -1     # no packed filter
    assert fwd(p, p, None, 1, 128, 4, 4, 2, 1, 0, None, None) == -1     # no output
    assert fwd(p, p, None, 1, 128, 4, 4, 2, 3, 0, p, None) == -1        # stride 3
    assert fwd(p, p, None, 1, 256, 4, 4, 2, 1, 0, p, None) == -1        # cg 128
    # more workgroups than a grid holds: refused, not wrapped
    # (2^22 images x 32 groups x 8 x 4 tiles = 2^32 >= 2^31, so nothing is launched on a machine with a device either)
    assert fwd(p, p, None, 1 << 22, 2048, 64, 64, 32, 1, 0, p, None) == -1
    assert L.ssad_grouped_conv3x3_pack_filter(None, 128, 2, p, None) == -1
    L.ssad_kernels_abi_version.restype = ctypes.c_int
    assert L.ssad_kernels_abi_version() == 3


def test_refusals_come_before_any_allocation(monkeypatch):
    from ssad_amd.backbone_f16 import NativeResNetFPNF16

    def boom(*a, **k):
        raise AssertionError("allocated before refusing")
    for fn in ("zeros", "empty", "full"):
        monkeypatch.setattr(torch, fn, boom)
    monkeypatch.setattr(K, "lib", boom)
    with pytest.raises(K.KernelError, match="x101-32x8d is forward only"):
        BP.NativeResNetFPN(ARCH, 1, (128, 128), "cpu", train=True)
    with pytest.raises(K.KernelError, match="channel_ratio 0.5 with the grouped architecture x101-32x8d"):
        BP.NativeResNetFPN(ARCH, 1, (128, 128), "cpu", train=False, channel_ratio=0.5)
    with pytest.raises(K.KernelError, match="x101-32x8d.*fp16 grouped kernel stops at 32-wide groups"):
        NativeResNetFPNF16(ARCH, 1, (128, 128), "cpu", train=False)
    with pytest.raises(K.KernelError, match=r"architectures \[.*'x101-32x8d'.*\]"):
        BP.NativeResNetFPN("x152", 1, (128, 128), "cpu", train=False)

    class Heads16(object):                 # what NativeDistillModel reads of fp16 subnets before it builds anything
        F16, blocked_io, distill, Dt, D = True, True, True, 256, 256
        lr = np.float32(1e-3)
    with pytest.raises(K.KernelError, match="x101-32x8d.*fp16 grouped kernel stops at 32-wide groups"):
        BP.NativeDistillModel(Heads16(), "r50", ARCH, N=1, image_hw=(128, 128), device="cpu", lr=1e-3)


def _random_blobs(capture, rng, prefix=""):
    return {prefix + p["name"]: rng.standard_normal(tuple(p["shape"])).astype(np.float32) for p in capture["params"]}


def test_weights_file_names_round_trip_and_the_other_resnext_is_told_apart(capture):
    rng = np.random.default_rng(32)
    for prefix in ("", "teacher/"):
        blobs = _random_blobs(capture, rng, prefix)
        state, scales, moms, missing = net.backbone_from_blobs(blobs, ARCH, prefix)
        assert not missing and not moms and len(scales) == 104          # one AffineChannel per body convolution
        shapes = BP.NativeResNetFPN.layer_shapes(ARCH)
        assert {k[:-7] for k in state if k.endswith(".weight")} == set(shapes)
        for layer, shape in shapes.items():
            assert tuple(state[layer + ".weight"].shape) == shape and tuple(state[layer + ".bias"].shape) == shape[:1]
        w, s = blobs[prefix + "res5_2_branch2b_w"], blobs[prefix + "res5_2_branch2b_bn_s"]
        assert np.array_equal(state["res5.2.c2.weight"].numpy(), w * s.reshape(-1, 1, 1, 1))
        with pytest.raises(net.WeightsWidthError) as e:
            net.backbone_from_blobs(blobs, "x101-64x4d", prefix)
        msg = str(e.value)
        assert prefix + "res2_0_branch2b_w" in msg and "(256, 8, 3, 3)" in msg and "(256, 4, 3, 3)" in msg
    # and the other way round: a 64x4d file into this network
    g64 = json.load(open(os.path.join(GOLDEN, "backbone_graph_x101_64x4d_fpn.json")))
    with pytest.raises(net.WeightsWidthError, match=r"res2_0_branch2b_w.*\(256, 4, 3, 3\).*\(256, 8, 3, 3\)"):
        net.backbone_from_blobs(_random_blobs(g64, rng), ARCH)
    assert net.backbone_from_blobs(_random_blobs(g64, rng), "x101-64x4d")[3] == []


def test_program_records_of_the_frozen_teacher():
    nat = BP.NativeResNetFPN(ARCH, 1, (128, 128), "cpu", train=False)
    P = nat.prog
    fwd = Counter(o.code for o in P.ops[P.marks["forward"]:P.marks["backward"]])
    assert fwd[PR.GROUPED_CONV3X3] == 33
    assert Counter(o.code for o in nat.prep.ops)[PR.GROUPED_PACK] == 33
    assert not any(o.code == PR.GROUPED_PACK for o in P.ops)           # frozen: packed once, not every step
    assert P.marks["backward"] == P.marks["end"] and "sgd" not in P.marks
    assert nat.params_flat.numel() == 0
    g = [o for o in P.ops if o.code == PR.GROUPED_CONV3X3]
    # (N, C, H, W, group, stride, relu): res5's first layer is the stride-2 one, on res4's 8 x 8 map
    assert [tuple(o.i)[:7] for o in g[-3:]] == [(1, 2048, 8, 8, 32, 2, 1), (1, 2048, 4, 4, 32, 1, 1),
                                            (1, 2048, 4, 4, 32, 1, 1)]
    assert nat._amax.next <= nat.AMAX_WORDS
