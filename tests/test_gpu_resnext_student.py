"""A ResNeXt as the student of the native step, on the GPU: the one-launch table pack of the grouped filters
(grouped_pack.hip) against the per-layer launchers, every trained grouped layer's two gradients inside the backbone
program against float64 products of the program's own tensors, the whole backward pass against the float64 torch
network, determinism, the model's step, and a weights round trip."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssad_amd  # noqa: F401
from guarded import SENTINEL
from test_gpu_kernels import CONV_FLOOR, CONV_RTOL, close, dev

pytestmark = pytest.mark.gpu
RESNEXTS = ("x101-64x4d", "x101-32x8d")
STRIDED = ("res3.0", "res4.0", "res5.0")
SHAPES_128 = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]


@pytest.fixture(scope="module")
def K():
    from ssad_amd import kernels
    kernels.lib()
    return kernels


def rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


def words(t):
    return t.detach().contiguous().view(torch.int32)


def trained_grouped(nat):
    return [l for l in nat._layers.values() if l.group > 1 and l.train]


# ---- 1. the pack launch ----------------------------------------------------------------------------------------------

# (C, group, forward pack?, data-gradient pack?): the five widths 4, 8, 16, 32, 64 mixed, one entry with each pack alone
MIXED = [(64, 16, True, True), (128, 16, True, True), (256, 16, True, True), (512, 16, True, True),
         (2048, 32, True, True), (128, 16, True, False), (256, 16, False, True)]


def filters(table, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((C, C // G, 3, 3)).astype(np.float32) for C, G, _, _ in table]


def per_layer(K, table, ws):
    """the parent's two launchers, filter by filter -> [(pf or None, pd or None)]"""
    return [(K.grouped_conv3x3_pack_filter(w, G) if f else None, K.grouped_conv3x3_pack_filter_dgrad(w, G) if d else None)
            for (C, G, f, d), w in zip(table, ws)]


def sentinel_outputs(K, table):
    out = []
    for C, G, f, d in table:
        n = K.lib().ssad_grouped_conv3x3_filter_floats(C, G)
        assert n == K.lib().ssad_grouped_conv3x3_dgrad_filter_floats(C, G) > 0
        out.append(tuple(torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32) if want else None
                         for want in (f, d)))
    return out


def test_one_launch_packs_a_mixed_table_bit_identically(K):
    assert sorted({C // G for C, G, _, _ in MIXED}) == [4, 8, 16, 32, 64]
    ws = [dev(w) for w in filters(MIXED, 41)]
    want = per_layer(K, MIXED, ws)
    outs = sentinel_outputs(K, MIXED)
    K.grouped_conv3x3_pack_filters([(w, G, pf, pd) for (C, G, _, _), w, (pf, pd) in zip(MIXED, ws, outs)])
    torch.cuda.synchronize()
    for k, (got, ref) in enumerate(zip(outs, want)):
        for g, r, what in zip(got, ref, ("forward", "data gradient")):
            if r is not None:
                assert torch.equal(words(g), words(r)), "entry %d, %s pack" % (k, what)


def test_a_70_entry_table_is_chunked(K):
    table = [((64, 16), (128, 16), (256, 16), (64, 2), (128, 2))[k % 5] + (k % 3 != 1, k % 3 != 2) for k in range(70)]
    assert len(table) > 64 and sorted({C // G for C, G, _, _ in table}) == [4, 8, 16, 32, 64]
    ws = [dev(w) for w in filters(table, 42)]
    want = per_layer(K, table, ws)
    outs = sentinel_outputs(K, table)
    K.grouped_conv3x3_pack_filters([(w, G, pf, pd) for (C, G, _, _), w, (pf, pd) in zip(table, ws, outs)])
    torch.cuda.synchronize()
    for k, (got, ref) in enumerate(zip(outs, want)):
        for g, r in zip(got, ref):
            assert (g is None) == (r is None)
            if r is not None:
                assert torch.equal(words(g), words(r)), "entry %d" % k


@pytest.mark.parametrize("bad", [(24, 2, "w", "pf", "pd"), (65, 16, "w", "pf", "pd"), (64, 16, None, "pf", "pd"),
                                 (64, 16, "w", None, None)], ids=["width12", "C_not_multiple", "no_w", "no_pack"])
def test_a_bad_entry_in_the_middle_leaves_every_output_untouched(K, bad):
    """The raw launcher (the wrapper would refuse first): 66 good entries around one bad one, so that a launcher
    which validated chunk by chunk would already have written the first 64."""
    table = [(64, 16, True, True)] * 66
    ws = [dev(w) for w in filters(table[:1], 43)] * 66
    outs = sentinel_outputs(K, table)
    tab = (K.GroupedPackEntry * 67)()
    rows = [K.GroupedPackEntry(w.data_ptr(), pf.data_ptr(), pd.data_ptr(), 64, 16) for w, (pf, pd) in zip(ws, outs)]
    Cb, Gb, w, pf, pd = bad
    spare = torch.full((4096,), SENTINEL, dtype=torch.int32, device="cuda")
    rows.insert(65, K.GroupedPackEntry(ws[0].data_ptr() if w else None, spare.data_ptr() if pf else None,
                                       spare.data_ptr() if pd else None, Cb, Gb))
    for k, r in enumerate(rows):
        tab[k] = r
    rc = K.lib().ssad_grouped_conv3x3_pack_filters(tab, 67, K._stream())
    torch.cuda.synchronize()
    assert rc == -1
    assert bool((spare == SENTINEL).all())
    for pf, pd in outs:
        assert bool((words(pf) == SENTINEL).all()) and bool((words(pd) == SENTINEL).all())


def test_guarded_table_pack(K, monkeypatch):
    """Guard bands intact, the filters unchanged, every pack written completely, the same bits as on ordinary
    allocations and as the per-layer launchers'."""
    from test_gpu_isolation import isolated
    table = [(64, 16, True, True), (48, 6, True, True), (64, 4, True, True), (64, 2, True, False), (128, 2, False, True)]
    Ws = filters(table, 44)
    L = K.lib()

    def fn(al):
        entries, res = [], {}
        for k, ((C, G, f, d), w) in enumerate(zip(table, Ws)):
            n = L.ssad_grouped_conv3x3_filter_floats(C, G)
            pf = al.out("pf%d" % k, n) if f else None
            pd = al.out("pd%d" % k, n) if d else None
            entries.append((al.inp("w%d" % k, w), G, pf, pd))
            res.update({name: t for name, t in (("pf%d" % k, pf), ("pd%d" % k, pd)) if t is not None})
        K.grouped_conv3x3_pack_filters(entries)
        return res

    got = isolated(K, monkeypatch, fn)
    for k, ((C, G, f, d), w) in enumerate(zip(table, Ws)):
        tw = dev(w)
        if f:
            assert np.array_equal(got["pf%d" % k].view(np.int32), K.grouped_conv3x3_pack_filter(tw, G).cpu().numpy().view(np.int32))
        if d:
            assert np.array_equal(got["pd%d" % k].view(np.int32),
                                  K.grouped_conv3x3_pack_filter_dgrad(tw, G).cpu().numpy().view(np.int32))


# ---- 2. wiring, layer by layer ---------------------------------------------------------------------------------------

def reference_net(arch, seed):
    if arch == "x101-32x8d":
        from torch_ref_x32 import RefX32ResNetFPN
        return RefX32ResNetFPN(seed=seed)
    from torch_ref import RefResNetFPN
    return RefResNetFPN(arch, seed=seed)


@pytest.mark.parametrize("arch", RESNEXTS)
def test_every_trained_grouped_layer_gets_its_own_products(arch):
    """Free of ReLU-mask sensitivity: each layer's gradients against float64 products of the tensors the program
    itself holds.  N = 2 at 128 x 128: res5's maps are 4 x 4, narrower than a 16-column tile."""
    from ssad_amd.backbone_pipeline import NativeResNetFPN
    N, hw = 2, (128, 128)
    ref = reference_net(arch, 21)
    nat = NativeResNetFPN(arch, N, hw, "cuda", train=True, grouped_grad=True, src=ref.state_dict(),
                          affine_scales=ref.scales)
    gen = torch.Generator(device="cuda").manual_seed(6)
    images = torch.randn((N, 3) + hw, device="cuda", generator=gen)
    nat.pack()
    fpn = nat.forward(images)
    nat.backward([torch.randn(t.shape, device="cuda", generator=gen) for t in fpn])
    torch.cuda.synchronize()
    layers = trained_grouped(nat)
    assert len(layers) == 30
    assert tuple(nat.saved["res5.2"]["y1"].shape[2:]) == (4, 4)
    for l in layers:
        pre = l.name[:-3]
        sv = nat.saved[pre]
        y1, dz1, dz2 = sv["y1"], sv["dz1"], sv["dz2"]
        assert l.stride == (2 if pre in STRIDED else 1)
        x = y1.double().requires_grad_(True)
        w = l.w.double().requires_grad_(True)
        F.conv2d(x, w, None, l.stride, 1, 1, l.group).backward(dz2.double())
        assert float(dz2.abs().max()) > 0 and bool(torch.isfinite(dz2).all())
        close(l.gw.cpu().numpy(), w.grad.cpu().numpy(), CONV_RTOL, CONV_FLOOR, l.name + " dW")
        want = torch.where(y1 > 0, x.grad, torch.zeros_like(x.grad))
        close(dz1.cpu().numpy(), want.cpu().numpy(), CONV_RTOL, CONV_FLOOR, l.name + " dX")
        assert bool((dz1[y1 <= 0] == 0).all()), l.name
        if pre in STRIDED:
            # c1 read the full-size map: its filter gradient is the product with that tensor, not the subsampled one
            xin, l1 = sv["x"], nat._layers[pre + ".c1"]
            assert sv["c1_in"] is xin and tuple(xin.shape[2:]) == tuple(y1.shape[2:]) != tuple(sv["xs"].shape[2:])
            want = torch.einsum("nmhw,nchw->mc", dz1.double(), xin.double())
            close(l1.gw.view(l1.cout, l1.cin).cpu().numpy(), want.cpu().numpy(), CONV_RTOL, CONV_FLOOR, l1.name + " dW")


# ---- 3. the whole backward pass against torch float64 ------------------------------------------------------------------

def _against_torch(arch, N, hw, seed):
    """-> (nat, {parameter: relative error of its gradient}, forward errors)"""
    from ssad_amd.backbone_pipeline import NativeResNetFPN
    gen = torch.Generator(device="cuda").manual_seed(5)
    images = torch.randn((N, 3) + hw, device="cuda", generator=gen)
    ref = reference_net(arch, seed)
    ref.calibrate(images)
    scales = dict(ref.scales)
    scales["res4.1.c2"] = 0.5                   # a grouped filter whose update carries an s^2 factor other than 1
    nat = NativeResNetFPN(arch, N, hw, "cuda", train=True, grouped_grad=True, src=ref.state_dict(), lr=0.01,
                          affine_scales=scales)
    nat.pack()
    got = nat.forward(images)
    want = ref(images)
    fwd = [rel(g, w.detach()) for g, w in zip(got, want)]
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
        assert tuple(g.shape) == tuple(p.grad.shape), name
        errs[name] = rel(g, p.grad)
    return nat, errs, fwd


@pytest.mark.parametrize("arch,N,hw", [("x101-64x4d", 2, (128, 256)), ("x101-32x8d", 1, (128, 128))],
                         ids=["x101-64x4d", "x101-32x8d"])
def test_resnext_student_backward_and_update_vs_torch(arch, N, hw):
    """Forward levels rel < 2e-5 (the ResNeXt teacher tests' bound), FPN parameters < 2e-5, every trained parameter
    gradient < 1e-4 with mask-safe biases (test_native_backbone_meets_1e4_when_masks_cannot_flip's bar), then the SGD
    update by the r50 test's formula.  Measured worst values: profiles/resnext_student.md."""
    nat, errs, fwd = _against_torch(arch, N, hw, 14)
    order = sorted(errs.items(), key=lambda kv: -kv[1])
    fpn = {k: v for k, v in errs.items() if k.split(".")[0] in ("lat", "out", "p6", "p7")}
    grouped = {k: v for k, v in errs.items() if k.endswith(".c2.weight")}
    print("%s forward rel P3..P7: %s" % (arch, " ".join("%.3e" % e for e in fwd)))
    print("%s worst gradient: %s %.3e; worst FPN %.3e; worst grouped filter %s %.3e" % (
        arch, order[0][0], order[0][1], max(fpn.values()), max(grouped, key=grouped.get), max(grouped.values())))
    assert len(grouped) == 30
    assert max(fwd) < 2e-5, fwd
    assert max(fpn.values()) < 2e-5, sorted(fpn.items(), key=lambda kv: -kv[1])[:5]
    assert order[0][1] < 1e-4, order[:5]
    # SGD: weights s^2 g + wd * w (s = the folded AffineChannel scale), biases 2 g (optimizer.py:115-130)
    p0, g0 = nat.params_flat.clone(), nat.grads_flat.clone()
    nat.sgd_step()
    want = torch.empty_like(p0)
    rows = {}
    for off, n, is_bias, row_len, s2 in nat.segments:
        g = g0[off:off + n]
        if s2 is not None:
            g = (g.view(-1, row_len) * s2.view(-1, 1)).reshape(-1)
            rows[off] = row_len
        want[off:off + n] = p0[off:off + n] - 0.01 * (2.0 * g if is_bias else g + 1e-4 * p0[off:off + n])
    l = nat._layers["res4.1.c2"]
    assert rows[(l.w.data_ptr() - nat.params_flat.data_ptr()) // 4] == l.wcin * 9 and l.group > 1
    assert float(l.s2[0]) == 0.25 and tuple(l.s2.shape) == (l.cout,)
    assert len(rows) == sum(1 for l in nat._layers.values() if l.train and l.affine)
    assert torch.allclose(nat.params_flat, want, rtol=1e-5, atol=1e-8)
    assert not torch.equal(l.w, p0[(l.w.data_ptr() - nat.params_flat.data_ptr()) // 4:][:l.w.numel()].view_as(l.w))


# ---- 4. determinism --------------------------------------------------------------------------------------------------

def test_same_bits_twice_and_without_the_auxiliary_streams():
    from ssad_amd.backbone_pipeline import NativeResNetFPN
    arch, N, hw = "x101-64x4d", 1, (128, 128)
    gen = torch.Generator(device="cuda").manual_seed(8)
    images = torch.randn((N, 3) + hw, device="cuda", generator=gen)
    nat = NativeResNetFPN(arch, N, hw, "cuda", train=True, grouped_grad=True)
    nat.pack()
    d_fpn = [torch.randn(t.shape, device="cuda", generator=gen) for t in nat.forward(images)]

    def once(net):
        net.poison()
        net.grads_flat.fill_(float("nan"))
        net.pack()
        net.forward(images)
        net.backward(d_fpn)
        torch.cuda.synchronize()
        return net.grads_flat.clone()

    a, b = once(nat), once(nat)
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    assert torch.equal(words(a), words(b))
    serial = NativeResNetFPN(arch, N, hw, "cuda", train=True, grouped_grad=True, overlap_wgrad=False)
    assert {o.stream for o in serial.prog.ops} == {0} and max(o.stream for o in nat.prog.ops) >= 1
    assert torch.equal(serial.params_flat, nat.params_flat)
    assert torch.equal(words(once(serial)), words(a))


# ---- 5. the model ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("teacher", [None, "r50"], ids=["teacherless", "r50_teacher"])
def test_model_trains_a_resnext_student(teacher):
    from ssad_amd import synth
    from ssad_amd.backbone_pipeline import NativeDistillModel
    from ssad_amd.head_pipeline import DistillHeads
    from ssad_amd.modeling.retinanet_heads import HeadConfig
    N, hw = 1, (128, 128)
    rng = np.random.default_rng(9)
    labs = [synth.distill_inputs(rng, N, 9, 80, h, w)[2] for h, w in SHAPES_128]
    tg = [synth.bbox_targets(rng, l) for l in labs]
    to = lambda a: torch.from_numpy(a).to("cuda")                   # noqa: E731
    labels, targets = [to(a) for a in labs], [(to(y), to(l)) for y, l in tg]
    fg = torch.tensor([float(max(1, sum(t[0].shape[0] for t in tg)))], device="cuda")
    images = torch.randn((N, 3) + hw, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))

    def run():
        torch.manual_seed(0)
        kw = dict(teacher_init=synth.head_params(np.random.default_rng(2))) if teacher else dict(distill=False)
        heads = DistillHeads(HeadConfig(num_gpus=1), N=N, shapes=SHAPES_128, device="cuda", lr=1e-3,
                             student_init=synth.head_params(np.random.default_rng(1)), **kw)
        m = NativeDistillModel(heads, "x101-64x4d", teacher, N=N, image_hw=hw, device="cuda",
                               student_grouped_grad=True)
        assert m.student.train and m.student.grouped_grad and (m.teacher is None) == (teacher is None)
        before = {l.name: l.w.clone() for l in trained_grouped(m.student)}
        losses = []
        for _ in range(2):
            m.step(images, labels, targets, fg)
            losses.append(m.heads.losses.clone())
        torch.cuda.synchronize()
        assert len(before) == 30
        for l in trained_grouped(m.student):
            assert bool(torch.isfinite(l.w).all()) and not torch.equal(l.w, before[l.name]), l.name
        return losses, m.student.params_flat.clone(), m.heads.params.flat.clone()

    a, b = run(), run()
    for la, lb in zip(a[0], b[0]):
        assert bool(torch.isfinite(la).all())
        assert torch.equal(words(la), words(lb))
    assert torch.equal(words(a[1]), words(b[1])) and torch.equal(words(a[2]), words(b[2]))


def test_model_without_the_keyword_refuses_as_before():
    from ssad_amd import kernels as K
    from ssad_amd.backbone_pipeline import NativeDistillModel
    from ssad_amd.head_pipeline import DistillHeads
    from ssad_amd.modeling.retinanet_heads import HeadConfig
    heads = DistillHeads(HeadConfig(num_gpus=1), N=1, shapes=SHAPES_128, device="cuda", lr=1e-3, distill=False)
    with pytest.raises(K.KernelError, match="x101-64x4d is forward only"):
        NativeDistillModel(heads, "x101-64x4d", None, N=1, image_hw=(128, 128), device="cuda")


# ---- 6. weights ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arch", RESNEXTS)
def test_a_stepped_resnext_student_round_trips_a_weights_file(arch):
    """Parameters, update history and the un-folded AffineChannel scales of a once-stepped student through the
    reference's blob layout and back, bit for bit (the folded scales here are powers of two: W' / s * s is exact)."""
    from ssad_amd.backbone_pipeline import NativeResNetFPN
    from ssad_amd.utils import net
    N, hw = 1, (128, 128)
    gen = torch.Generator(device="cuda").manual_seed(3)
    images = torch.randn((N, 3) + hw, device="cuda", generator=gen)
    scales = {"res3.1.c2": 0.5, "res5.0.c2": 2.0}
    nat = NativeResNetFPN(arch, N, hw, "cuda", train=True, grouped_grad=True, lr=0.01, affine_scales=scales)
    nat.pack()
    nat.backward([torch.randn(t.shape, device="cuda", generator=gen) for t in nat.forward(images)])
    nat.sgd_step()
    torch.cuda.synchronize()
    l = nat._layers["res5.0.c2"]
    off = (l.w.data_ptr() - nat.params_flat.data_ptr()) // 4
    assert float(nat.moms_flat[off:off + l.w.numel()].abs().max()) > 0
    blobs = net.backbone_to_blobs(nat)
    cg = l.wcin
    assert blobs["res5_0_branch2b_w"].shape == blobs["res5_0_branch2b_w_momentum"].shape == (l.cout, cg, 3, 3)
    assert np.array_equal(blobs["res5_0_branch2b_bn_s"], np.full(l.cout, 2.0, np.float32))
    assert np.array_equal(blobs["res5_0_branch2b_w"], (l.w / 2.0).cpu().numpy())
    state, sc, moms, missing = net.backbone_from_blobs(blobs, arch)
    assert not missing and "res5.0.c2.weight" in moms
    fresh = NativeResNetFPN(arch, N, hw, "cuda", train=True, grouped_grad=True, lr=0.01, src=state, affine_scales=sc)
    net.load_backbone(fresh, blobs, strict=True)
    assert torch.equal(words(fresh.params_flat), words(nat.params_flat))
    assert torch.equal(words(fresh.moms_flat), words(nat.moms_flat))
    assert torch.equal(words(fresh.frozen_flat), words(nat.frozen_flat))
    for name, lyr in nat._layers.items():
        if lyr.s2 is not None:
            assert torch.equal(fresh._layers[name].s2, lyr.s2), name
    for name, v in nat.affine_scale_values.items():
        back = fresh.affine_scale_values[name]
        assert torch.equal(back, v.expand_as(back)), name
    assert float(fresh._layers["res5.0.c2"].s2[0]) == 4.0 and float(fresh._layers["res3.1.c2"].s2[0]) == 0.25
