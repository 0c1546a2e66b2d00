"""The fp16-storage ResNeXt-101-32x8d teacher (wide_groups=True), the parts that need no device: the 64-wide entry
points' argument checks and pack size, the Python wrappers' refusals by name, what stays refused, and the records of
the teacher's program (res5 on GROUPED_F16_CG64, every narrower width on the records it always had)."""
import ctypes
from collections import Counter

import numpy as np
import pytest
import torch

import ssad_amd  # noqa: F401
from ssad_amd import backbone_pipeline as BP, kernels as K, program as PR

ARCH = "x101-32x8d"


def test_cg64_entry_points_check_their_arguments_without_a_device():
    L = K.lib()
    halves, pack, conv = (L.ssad_grouped_conv3x3_f16_cg64_filter_halves, L.ssad_grouped_conv3x3_f16_cg64_pack_filter,
                          L.ssad_grouped_conv3x3_f16_cg64)
    assert halves(2048, 32) == 2048 * 64 * 9
    assert halves(128, 2) == 128 * 64 * 9 and halves(64, 1) == 64 * 64 * 9
    assert halves(2048, 64) == 0                                        # 32-wide groups: the narrow entry points'
    for c, g in ((64, 2), (64, 4), (96, 1), (128, 3), (0, 1), (64, 0), (-64, -1)):
        assert halves(c, g) == 0, (c, g)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for c, g in ((64, 2), (64, 4), (96, 1), (128, 3)):
        assert conv(p, p, None, 1, c, 4, 4, g, 1, p, None) == -1, (c, g)
        assert pack(p, c, g, p, None) == -1, (c, g)
    assert conv(None, p, None, 1, 128, 4, 4, 2, 1, p, None) == -1       # no input
    assert conv(p, None, None, 1, 128, 4, 4, 2, 1, p, None) == -1       # no packed filter
    assert conv(p, p, None, 1, 128, 4, 4, 2, 1, None, None) == -1       # no output
    assert pack(None, 128, 2, p, None) == -1 and pack(p, 128, 2, None, None) == -1
    assert conv(p, p, None, -1, 128, 4, 4, 2, 1, p, None) == -1
    assert conv(p, p, None, 1, 128, 0, 4, 2, 1, p, None) == -1 and conv(p, p, None, 1, 128, 4, 0, 2, 1, p, None) == -1
    # 2^31 bytes and above: refused, not wrapped (2048 channels x 1024 x 1024 halves = 2^32 bytes)
    assert conv(p, p, None, 1, 2048, 1024, 1024, 32, 1, p, None) == -1
    assert conv(p, p, None, 0, 128, 4, 4, 2, 1, p, None) == 0           # no images: nothing to do
    # the narrow entry points keep refusing the width
    assert L.ssad_grouped_conv3x3_f16(p, p, None, 1, 128, 4, 4, 2, 1, p, None) == -1
    assert L.ssad_grouped_conv3x3_f16_pack_filter(p, 128, 2, p, None) == -1
    L.ssad_kernels_abi_version.restype = ctypes.c_int
    assert L.ssad_kernels_abi_version() == 3


def test_wrappers_refuse_a_bad_geometry_by_name_before_the_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("touched the library before refusing")
    monkeypatch.setattr(K, "lib", boom)
    x = torch.zeros((1, 16, 4, 4, 8), dtype=torch.float16)
    for c, g in ((64, 2), (64, 4), (96, 1), (128, 3), (2048, 64)):
        with pytest.raises(K.KernelError, match="grouped_conv3x3_f16_cg64: %d channels in %d groups" % (c, g)):
            K.grouped_conv3x3_f16_cg64(x, x, None, c, g)
        with pytest.raises(K.KernelError, match="grouped_conv3x3_f16_cg64_pack_filter: %d channels in %d groups" % (c, g)):
            K.grouped_conv3x3_f16_cg64_pack_filter(torch.zeros((c, 64, 3, 3)), g)
    with pytest.raises(K.KernelError, match=r"cg64_pack_filter: a \(128, 32, 3, 3\) filter"):
        K.grouped_conv3x3_f16_cg64_pack_filter(torch.zeros((128, 32, 3, 3)), 2)
    with pytest.raises(K.KernelError, match=r"cg64: x is .*blocked \[N\]\[32\]"):
        K.grouped_conv3x3_f16_cg64(x, x, None, 256, 4)


def test_refusals_come_before_any_allocation(monkeypatch):
    from ssad_amd.backbone_f16 import NativeResNetFPNF16

    def boom(*a, **k):
        raise AssertionError("allocated before refusing")
    for fn in ("zeros", "empty", "full"):
        monkeypatch.setattr(torch, fn, boom)
    monkeypatch.setattr(K, "lib", boom)
    # no fp16 grouped gradients: a grouped architecture stays forward only, with the message of before
    with pytest.raises(K.KernelError, match="x101-32x8d is forward only"):
        NativeResNetFPNF16(ARCH, 1, (128, 128), "cpu", train=True, wide_groups=True)
    with pytest.raises(K.KernelError, match="x101-64x4d is forward only"):
        NativeResNetFPNF16("x101-64x4d", 1, (128, 128), "cpu", train=True, wide_groups=True)
    # without the keyword (or with it off) nothing changed
    for kw in ({}, dict(wide_groups=False)):
        for train in (False, True):
            with pytest.raises(K.KernelError, match="x101-32x8d.*fp16 grouped kernel stops at 32-wide groups"):
                NativeResNetFPNF16(ARCH, 1, (128, 128), "cpu", train=train, **kw)
    with pytest.raises(K.KernelError, match="fp16 grouped kernel stops at 32-wide groups"):
        BP.check_f16_grouped(ARCH)
    BP.check_f16_grouped(ARCH, wide_groups=True)
    BP.check_f16_grouped("x101-64x4d", wide_groups=True)
    BP.check_f16_grouped("r50", wide_groups=True)
    with pytest.raises(K.KernelError, match="grouped_grad.*fp32 backbone"):
        NativeResNetFPNF16(ARCH, 1, (128, 128), "cpu", train=True, grouped_grad=True, wide_groups=True)

    class Heads16(object):                 # what NativeDistillModel reads of fp16 subnets before it builds anything
        F16, blocked_io, distill, Dt, D = True, True, True, 256, 256
        lr = np.float32(1e-3)
    with pytest.raises(K.KernelError, match="x101-32x8d.*fp16 grouped kernel stops at 32-wide groups"):
        BP.NativeDistillModel(Heads16(), "r50", ARCH, N=1, image_hw=(128, 128), device="cpu", lr=1e-3,
                              teacher_wide_groups=False)
    # the keyword is the TEACHER's: an fp16 ResNeXt student stays refused
    with pytest.raises(K.KernelError, match="x101-32x8d.*fp16 grouped kernel stops at 32-wide groups"):
        BP.NativeDistillModel(Heads16(), ARCH, "r50", N=1, image_hw=(128, 128), device="cpu", lr=1e-3,
                              teacher_wide_groups=True)


def test_teacher_program_puts_res5_on_the_new_records_and_nothing_else():
    from ssad_amd.backbone_f16 import NativeResNetFPNF16
    te = NativeResNetFPNF16(ARCH, 1, (128, 128), "cpu", train=False, wide_groups=True)
    assert te.wide_groups and te.params_flat.numel() == 0 and "sgd" not in te.prog.marks
    lo, hi = te.prog.marks["forward"], te.prog.marks["backward"]
    fw = Counter(o.code for o in te.prog.ops[lo:hi])
    assert fw[PR.GROUPED_F16] == 30 and fw[PR.GROUPED_F16_CG64] == 3
    wide = [o for o in te.prog.ops[lo:hi] if o.code == PR.GROUPED_F16_CG64]
    L = te._layers
    # (N, C, H, W, group, relu): res5.0 at stride 1 on res4's 8 x 8 map, then the even positions; the others at 4 x 4
    assert [tuple(o.i[:6]) for o in wide] == [(1, 2048, 8, 8, 32, 1), (1, 2048, 4, 4, 32, 1), (1, 2048, 4, 4, 32, 1)]
    assert [o.p[1] for o in wide] == [L["res5.%d.c2" % j].pf.data_ptr() for j in range(3)]
    assert all(o.klass == 61 for o in wide)
    for j in range(3):
        assert L["res5.%d.c2" % j].pf.numel() == 2048 * 64 * 9 and L["res5.%d.c2" % j].pf.dtype == torch.float16
    packs = Counter(o.code for o in te.prep.ops)                       # frozen: packed once, in the prep program
    assert packs[PR.GROUPED_F16_PACK] == 30 and packs[PR.GROUPED_F16_CG64_PACK] == 3
    assert all(tuple(o.i[:2]) == (2048, 32) for o in te.prep.ops if o.code == PR.GROUPED_F16_CG64_PACK)
    assert L["res5.0.c2"].stride == 2 and L["res3.0.c2"].stride == 2 and L["res5.1.c2"].stride == 1
    # no effect on any other architecture: the 64x4d teacher's program is record for record what it was
    a = NativeResNetFPNF16("x101-64x4d", 1, (128, 128), "cpu", train=False)
    b = NativeResNetFPNF16("x101-64x4d", 1, (128, 128), "cpu", train=False, wide_groups=True)
    sig = lambda net: [(o.code, o.klass, tuple(o.i), tuple(o.l)) for prog in (net.prep, net.prog) for o in prog.ops]
    assert sig(a) == sig(b)
    assert not any(o.code in (PR.GROUPED_F16_CG64, PR.GROUPED_F16_CG64_PACK) for o in b.prog.ops + b.prep.ops)
    assert (PR.GROUPED_F16_CG64, PR.GROUPED_F16_CG64_PACK) == (87, 88)
