"""A ResNeXt as the student of the native step (NativeResNetFPN(..., train=True, grouped_grad=True)), the parts that
need no device: the keyword and what stays refused, the records of the step program (one GROUPED_PACKS launch for the
30 trained grouped layers, their GROUPED_WGRAD / GROUPED_DGRAD records, the tensors c1's filter gradient reads in the
stride-2 blocks), programs that must not change, and the table launcher's refusals."""
import ctypes
from collections import Counter

import numpy as np
import pytest
import torch

import ssad_amd  # noqa: F401
from ssad_amd import backbone_pipeline as BP, kernels as K, program as PR

import make_program_fingerprints as mpf

RESNEXTS = ("x101-64x4d", "x101-32x8d")
HW, N = (128, 128), 1
STRIDED = ("res3.0", "res4.0", "res5.0")


@pytest.fixture(scope="module", params=RESNEXTS)
def student(request):
    return BP.NativeResNetFPN(request.param, N, HW, "cpu", train=True, grouped_grad=True)


def trained_grouped(nat):
    return [l for l in nat._layers.values() if l.group > 1 and l.train]


def test_refusals_come_before_any_allocation(monkeypatch):
    from ssad_amd.backbone_f16 import NativeResNetFPNF16

    def boom(*a, **k):
        raise AssertionError("allocated before refusing")
    for fn in ("zeros", "empty", "full"):
        monkeypatch.setattr(torch, fn, boom)
    monkeypatch.setattr(K, "lib", boom)
    for arch in RESNEXTS:
        # without the keyword: the message of before
        with pytest.raises(K.KernelError, match="%s is forward only" % arch):
            BP.NativeResNetFPN(arch, N, HW, "cpu", train=True)
        with pytest.raises(K.KernelError, match="%s is forward only" % arch):
            BP.NativeResNetFPN(arch, N, HW, "cpu", train=True, grouped_grad=False)
        with pytest.raises(K.KernelError, match="channel_ratio 0.5 with the grouped architecture %s" % arch):
            BP.NativeResNetFPN(arch, N, HW, "cpu", train=True, grouped_grad=True, channel_ratio=0.5)
        with pytest.raises(K.KernelError, match="grouped_grad.*fp32 backbone"):
            NativeResNetFPNF16(arch, N, HW, "cpu", train=True, grouped_grad=True)
    with pytest.raises(K.KernelError, match="grouped_grad.*fp32 backbone"):
        NativeResNetFPNF16("r50", N, HW, "cpu", train=True, grouped_grad=True)

    class Heads16(object):                 # what NativeDistillModel reads of fp16 subnets before it builds anything
        F16, blocked_io, distill, Dt, D = True, True, True, 256, 256
        lr = np.float32(1e-3)
    with pytest.raises(K.KernelError, match="student_grouped_grad.*fp32 backbone"):
        BP.NativeDistillModel(Heads16(), "x101-64x4d", "r50", N=N, image_hw=HW, device="cpu", lr=1e-3,
                              student_grouped_grad=True)


def test_student_builds_with_grouped_parameters_in_their_stage_buckets(student):
    nat = student
    cg = {"x101-64x4d": 4, "x101-32x8d": 8}[nat.arch]
    layers = trained_grouped(nat)
    assert len(layers) == 30 and all(l.name.endswith(".c2") for l in layers)
    assert sum(1 for l in nat._layers.values() if l.group > 1 and not l.train) == 3          # res2 stays frozen
    segs = {off: (n, isb, row_len, s2) for off, n, isb, row_len, s2 in nat.segments}
    p0 = nat.params_flat.data_ptr()
    for l in layers:
        stage = int(l.name[3])
        width = cg * 2 ** (stage - 2)
        assert tuple(l.w.shape) == tuple(l.gw.shape) == (l.cout, width, 3, 3) and l.gb is None
        off = (l.w.data_ptr() - p0) // 4
        n, isb, row_len, _ = segs[off]
        assert (n, isb, row_len) == (l.cout * width * 9, 0, width * 9)
        b = nat.bucket["res%d" % stage]
        lo = (b.data_ptr() - nat.grads_flat.data_ptr()) // 4
        assert lo <= off and off + n <= lo + b.numel()
        assert l.pf.numel() == K.lib().ssad_grouped_conv3x3_filter_floats(l.cout, l.group)
        assert l.pd.numel() == K.lib().ssad_grouped_conv3x3_dgrad_filter_floats(l.cout, l.group)
    assert sum(n for _, n, _, _, _ in nat.segments) == nat.params_flat.numel()
    assert nat._amax.next <= nat.AMAX_WORDS


def test_one_pack_record_for_every_trained_grouped_layer(student):
    nat, P = student, student.prog
    packs = [k for k, o in enumerate(P.ops) if o.code == PR.GROUPED_PACKS]
    assert len(packs) == 1 and P.marks["pack"] <= packs[0] < P.marks["forward"]
    o = P.ops[packs[0]]
    assert o.i[0] == 30 and o.klass == 77 and o.stream == 0
    tab = nat._grouped_pack_table
    assert ctypes.addressof(tab) == o.p[0] and len(tab) == 30 and any(t is tab for t in P.keep)
    layers = trained_grouped(nat)
    for e, l in zip(tab, layers):
        assert (e.w, e.pf, e.pd, e.C, e.group) == (l.w.data_ptr(), l.pf.data_ptr(), l.pd.data_ptr(), l.cout, l.group)
    # the frozen ones stay per layer in the prepare program; the step program packs none of them one by one
    assert Counter(o.code for o in nat.prep.ops)[PR.GROUPED_PACK] == 3
    assert not any(o.code == PR.GROUPED_PACK for o in P.ops)
    assert not any(o.code in (PR.GROUPED_PACKS, PR.GROUPED_WGRAD, PR.GROUPED_DGRAD) for o in nat.prep.ops)


def test_gradient_records_of_the_grouped_layers(student):
    nat, P = student, student.prog
    lib = K.lib()
    lo, hi = P.marks["backward"], P.marks["sgd"]
    assert not any(o.code in (PR.GROUPED_WGRAD, PR.GROUPED_DGRAD) for o in P.ops[:lo] + P.ops[hi:])
    wg = {o.p[2]: o for o in P.ops[lo:hi] if o.code == PR.GROUPED_WGRAD}
    dg = {o.p[1]: o for o in P.ops[lo:hi] if o.code == PR.GROUPED_DGRAD}
    assert len(wg) == len(dg) == 30
    assert sum(1 for o in P.ops if o.code == PR.GROUPED_WGRAD) == sum(1 for o in P.ops if o.code == PR.GROUPED_DGRAD) == 30
    for kl in (75, 76, 77):
        assert kl in PR.KLASS and kl < 128
    for l in trained_grouped(nat):
        pre = l.name[:-3]
        sv = nat.saved[pre]
        y1, y2, dz1, dz2 = sv["y1"], sv["y2"], sv["dz1"], sv["dz2"]
        stride = 2 if pre in STRIDED else 1
        assert l.stride == stride
        assert tuple(dz1.shape) == tuple(y1.shape) and tuple(dz2.shape) == tuple(y2.shape)
        assert y1.shape[2] == stride * y2.shape[2] and y1.shape[3] == stride * y2.shape[3]
        geo = (N, l.cout, y1.shape[2], y1.shape[3], l.group, stride)
        w = wg[l.gw.data_ptr()]
        assert tuple(w.i)[:6] == geo and w.klass == 76
        assert w.stream >= 1                                                     # an auxiliary stream
        assert w.l[0] == lib.ssad_grouped_conv3x3_wgrad_workspace_bytes(*geo) > 0
        assert (w.p[0], w.p[1]) == (y1.data_ptr(), dz2.data_ptr()) and w.p[3] == nat.wss[w.stream].data_ptr()
        assert nat.wss[w.stream].numel() >= w.l[0]
        d = dg[l.pd.data_ptr()]
        assert tuple(d.i)[:6] == geo and d.klass == 75 and d.stream == 0
        assert (d.p[0], d.p[2], d.p[3]) == (dz2.data_ptr(), y1.data_ptr(), dz1.data_ptr())


def test_c1_filter_gradient_reads_what_c1_read(student):
    nat, P = student, student.prog
    wg1 = {o.p[2]: o for o in P.ops if o.code == PR.CONV1X1_WGRAD}
    for (stage, j, cin, cmid, cout, stride, proj, tr) in nat.blocks:
        if not tr:
            continue
        pre = "res%d.%d" % (stage, j)
        sv = nat.saved[pre]
        o = wg1[nat._layers[pre + ".c1"].gw.data_ptr()]
        assert sv["c1_in"] is sv["x"]                  # the stride sits on the 3x3: c1 sees the full map
        assert o.p[0] == sv["x"].data_ptr() and o.p[1] == sv["dz1"].data_ptr()
        assert tuple(o.i)[:4] == (N, cin, sv["x"].shape[2] * sv["x"].shape[3], cmid)
        if pre in STRIDED:
            assert sv["xs"] is not sv["x"] and sv["x"].shape[2] == 2 * sv["xs"].shape[2]
            op = wg1[nat._layers[pre + ".proj"].gw.data_ptr()]
            assert op.p[0] == sv["xs"].data_ptr()      # the projection reads the subsampled map


def test_input_gradient_of_the_strided_projection_blocks_in_a_fixed_order(student):
    """res4.0 / res5.0: W1^T dz1 (full size) accumulates straight onto the previous stage's output gradient, then
    Wp^T dz (half size) is scattered onto it -- GEMM first, SUBSAMPLE_GRAD second, both on the main stream."""
    nat, P = student, student.prog
    for pre, cin in (("res4.0", 512), ("res5.0", 1024)):
        sv = nat.saved[pre]
        x = sv["x"]
        sub = [k for k, o in enumerate(P.ops) if o.code == PR.SUBSAMPLE_GRAD and o.i[5] == 1
               and tuple(o.i)[:5] == (N, cin, x.shape[2], x.shape[3], 2)]
        assert len(sub) == 1
        tgt = P.ops[sub[0]].p[1]
        gemms = [k for k, o in enumerate(P.ops[:sub[0]]) if o.code in (PR.GEMM_CONV, PR.GEMM_CONV_SPLIT)
                 and ctypes.cast(o.p[0], ctypes.POINTER(K.GemmConv)).contents.y == tgt]
        # the lateral's data gradient wrote the buffer first; c1's accumulates
        assert len(gemms) == 2
        d = ctypes.cast(P.ops[gemms[1]].p[0], ctypes.POINTER(K.GemmConv)).contents
        assert d.x == sv["dz1"].data_ptr() and (d.K, d.M) == (nat._layers[pre + ".c1"].cout, cin)
        assert all(P.ops[k].stream == 0 for k in gemms + sub)


def _listing(*a, **kw):
    return mpf.listing([BP.NativeResNetFPN(*a, **kw)])


def test_programs_that_do_not_train_a_grouped_layer_keep_their_words():
    for arch in RESNEXTS:
        a = _listing(arch, N, HW, "cpu", train=False)
        b = _listing(arch, N, HW, "cpu", train=False, grouped_grad=True)
        assert a == b and a[1] > 0
        nat = BP.NativeResNetFPN(arch, N, HW, "cpu", train=False, grouped_grad=True)
        assert Counter(o.code for o in nat.prep.ops)[PR.GROUPED_PACK] == 33
        assert not any(o.code in (PR.GROUPED_PACKS, PR.GROUPED_WGRAD, PR.GROUPED_DGRAD) for o in nat.prog.ops)
    for train in (True, False):
        assert _listing("r50", N, HW, "cpu", train=train) == _listing("r50", N, HW, "cpu", train=train, grouped_grad=True)


def test_table_launcher_refuses_before_it_launches():
    L = K.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    E = K.GroupedPackEntry
    fn = L.ssad_grouped_conv3x3_pack_filters
    good = E(p, p, p, 64, 16)
    assert fn(None, 1, None) == -1                                          # no table
    assert fn((E * 1)(good), 0, None) == -1 and fn((E * 1)(good), -3, None) == -1
    assert fn((E * 2)(good, E(p, p, p, 24, 2)), 2, None) == -1               # 12 channels per group
    assert fn((E * 2)(good, E(p, p, p, 65, 16)), 2, None) == -1              # C % group != 0
    assert fn((E * 2)(good, E(p, None, None, 64, 16)), 2, None) == -1        # neither pack
    assert fn((E * 2)(good, E(None, p, p, 64, 16)), 2, None) == -1           # no filter
    assert ctypes.sizeof(E) == 32
    L.ssad_kernels_abi_version.restype = ctypes.c_int
    assert L.ssad_kernels_abi_version() == 3
    with pytest.raises(K.KernelError, match="empty table"):
        K.grouped_conv3x3_pack_filters([])
