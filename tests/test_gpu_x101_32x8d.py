"""ResNeXt-101-32x8d as a native teacher, on the GPU: the grouped 3x3 kernel for 64-wide groups
(csrc/kernels/grouped_conv3x3.hip, grouped_conv3x3_cg64_kernel) against the oracle, against the reference's own
compiled operator, in the guarded arena, with a planted NaN; the narrower widths' bits; the network against
float64 torch; a weights file; the whole distillation step."""
import hashlib
import json
import os
import pickle

import numpy as np
import pytest
import torch

import ssad_amd  # noqa: F401
from oracle import oracle
import make_golden as mg
from test_gpu_kernels import CONV_FLOOR, CONV_RTOL, close, dev
from test_gpu_gemm_conv import _grouped_oracle

pytestmark = pytest.mark.gpu
ARCH = "x101-32x8d"
CG = 64
# the geometries of test_gpu_gemm_conv.test_grouped_conv3x3_vs_oracle: (N, cg, G, H, W, stride)
NARROW_GEOMS = [(2, 4, 16, 19, 23, 1), (2, 4, 16, 19, 23, 2), (1, 8, 8, 16, 32, 1), (2, 8, 4, 9, 17, 2),
                (2, 16, 4, 12, 24, 1), (1, 16, 64, 8, 16, 2), (1, 32, 2, 10, 21, 1), (2, 32, 3, 16, 24, 2)]


@pytest.fixture(scope="module")
def K():
    from ssad_amd import kernels
    kernels.lib()
    return kernels


def case(N, G, H, W, seed, cg=CG):
    rng = np.random.default_rng(seed)
    C = cg * G
    X = rng.standard_normal((N, C, H, W)).astype(np.float32)
    Wt = (rng.standard_normal((C, cg, 3, 3)) * (1.0 / np.sqrt(9 * cg))).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    return X, Wt, b


# ---- 1. the kernel against the oracle ----------------------------------------------------------------------------

@pytest.mark.parametrize("geom", [
    (2, 1, 9, 19, 1),        # ragged both ways, second image
    (1, 3, 16, 32, 1),       # exact tiles, group indexing
    (2, 2, 11, 21, 2),       # odd map at stride 2, chunked staging
    (1, 2, 16, 32, 2),
    (1, 32, 5, 7, 1),        # the real 2048 channels on a map smaller than one tile
], ids=lambda g: "N%d_G%d_%dx%d_s%d" % g)
def test_grouped64_vs_oracle(K, geom):
    N, G, H, W, s = geom
    X, Wt, b = case(N, G, H, W, 640 + sum(geom))
    ref = _grouped_oracle(X, Wt, b, G, s)
    got = K.grouped_conv3x3_forward(dev(X), dev(Wt), dev(b), group=G, stride=s)
    assert tuple(got.shape) == ref.shape
    close(got.cpu().numpy(), ref, CONV_RTOL, CONV_FLOOR, "Y")
    got = K.grouped_conv3x3_forward(dev(X), dev(Wt), None, group=G, stride=s, relu=True)
    close(got.cpu().numpy(), np.maximum(_grouped_oracle(X, Wt, None, G, s), 0), CONV_RTOL, CONV_FLOOR, "relu(Y)")


# ---- 2. against the reference's compiled operator ------------------------------------------------------------------

def test_grouped64_vs_reference_operator_golden(K, golden_dir):
    """tests/golden/grouped64_ref.npz (make_grouped64_golden.py): ConvOp<float, CPUContext> with group 2 and 3."""
    g = np.load(os.path.join(golden_dir, "grouped64_ref.npz"))
    names = sorted(k[:-5] for k in g.files if k.endswith("_dims"))
    assert len(names) == 2
    for name in names:
        seed, N, Cin, M, H, W, k, s, p, grp = [int(v) for v in g[name + "_dims"]]
        assert Cin // grp == CG and (k, p) == (3, 1)
        X, Wt, b, _ = mg.conv_ref_inputs(seed, N, Cin, M, H, W, k, s, p, grp)
        Y = K.grouped_conv3x3_forward(dev(X), dev(Wt), dev(b), group=grp, stride=s).cpu().numpy()
        close(Y.ravel()[g[name + "_Y_idx"]], g[name + "_Y"], CONV_RTOL, CONV_FLOOR, name + " Y")


# ---- 3. isolation ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", [(2, 64, 2, 9, 17, 2), (3, 64, 1, 7, 9, 1)], ids=lambda g: "N%d_cg%d_G%d_%dx%d_s%d" % g)
def test_guarded_grouped64(K, monkeypatch, geom):
    """Guard bands intact, x / w / bias unchanged, y AND the pack written completely (no padding at this width: no
    nan_ok), bit-equal to the run on ordinary allocations (test_gpu_isolation.isolated)."""
    from test_gpu_isolation import isolated
    N, cg, G, H, W, s = geom
    X, Wt, b = case(N, G, H, W, 7900 + sum(geom), cg)
    oh, ow = (H - 1) // s + 1, (W - 1) // s + 1
    floats = K.lib().ssad_grouped_conv3x3_filter_floats(cg * G, G)
    assert floats == cg * G * 64 * 9

    def fn(al):
        packed = K.grouped_conv3x3_pack_filter(al.inp("w", Wt), G, out=al.out("packed", floats))
        y = K.grouped_conv3x3_forward(al.inp("x", X), None, al.inp("bias", b), group=G, stride=s, relu=True,
                                      out=al.out("y", (N, cg * G, oh, ow)), packed=packed)
        return dict(y=y, packed=packed)

    got = isolated(K, monkeypatch, fn)
    close(got["y"], np.maximum(_grouped_oracle(X, Wt, b, G, s), 0), CONV_RTOL, CONV_FLOOR, "relu(Y)")
    # the pack is a permutation of the filter: every word of it, nothing else
    assert np.array_equal(np.sort(got["packed"].ravel()), np.sort(Wt.ravel()))


# ---- 4. non-finite locality ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [1, 2])
def test_grouped64_nan_stays_in_its_group_image_and_window(K, s):
    N, G, H, W = 2, 2, 9, 13
    X, Wt, _ = case(N, G, H, W, 6464 + s)
    clean = K.grouped_conv3x3_forward(dev(X), dev(Wt), None, group=G, stride=s).cpu().numpy()
    assert np.all(np.isfinite(clean))
    Xn = X.copy()
    Xn[1, 70, 4, 6] = np.nan                                  # channel 70: group 1
    got = K.grouped_conv3x3_forward(dev(Xn), dev(Wt), None, group=G, stride=s).cpu().numpy()
    oh, ow = (H - 1) // s + 1, (W - 1) // s + 1
    want = np.zeros((N, G * CG, oh, ow), bool)
    for oy in range(oh):
        for ox in range(ow):
            if abs(oy * s - 4) <= 1 and abs(ox * s - 6) <= 1:         # the 3x3 window (pad 1) covers (4, 6)
                want[1, CG:2 * CG, oy, ox] = True
    assert want.sum() == CG * (9 if s == 1 else 1)            # stride 2: only output (2, 3) reads rows 3..5, columns 5..7
    assert np.array_equal(np.isnan(got), want)
    assert np.array_equal(got[~want].view(np.uint32), clean[~want].view(np.uint32))


# ---- 5. deterministic ----------------------------------------------------------------------------------------------

def test_grouped64_is_deterministic(K):
    N, G, H, W, s = 2, 2, 11, 21, 2
    X, Wt, b = case(N, G, H, W, 77)
    tx, tw, tb = dev(X), dev(Wt), dev(b)
    a = K.grouped_conv3x3_forward(tx, tw, tb, group=G, stride=s)
    c = K.grouped_conv3x3_forward(tx, tw, tb, group=G, stride=s)
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))


# ---- 6. the narrower widths are untouched ----------------------------------------------------------------------------

def narrow_case(geom):
    """Inputs of one pinned case: (X, Wt, b), seeded by the geometry as in test_grouped_conv3x3_vs_oracle."""
    N, cg, G, H, W, s = geom
    return case(N, G, H, W, sum(geom), cg)


def narrow_key(geom):
    return "N%d_cg%d_G%d_%dx%d_s%d" % tuple(geom)


def sha_words(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("geom", NARROW_GEOMS, ids=narrow_key)
def test_narrower_widths_give_the_parent_commits_bits(K, golden_dir, geom):
    """tests/golden/grouped_bits.json: sha256 of the raw fp32 output words (bias, no ReLU) of the library built from
    the commit named in the file, taken on an MI355X before the 64-wide kernel was added (profiles/x101_32x8d.md)."""
    pinned = json.load(open(os.path.join(golden_dir, "grouped_bits.json")))
    X, Wt, b = narrow_case(geom)
    N, cg, G, H, W, s = geom
    y = K.grouped_conv3x3_forward(dev(X), dev(Wt), dev(b), group=G, stride=s)
    assert sha_words(y) == pinned["sha256"][narrow_key(geom)]


# ---- 7. the network ------------------------------------------------------------------------------------------------

def rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


def test_native_x101_32x8d_teacher_matches_torch():
    """All five FPN levels against the float64 torch network (tests/torch_ref_x32.py) at the 64x4d teacher test's own
    bound, rel < 2e-5.  Measured on MI355X: see the values this test prints and profiles/x101_32x8d.md."""
    from ssad_amd.backbone_pipeline import NativeResNetFPN
    from ssad_amd import program as PR
    from torch_ref_x32 import RefX32ResNetFPN
    ref = RefX32ResNetFPN(seed=13)
    N, hw = 1, (128, 256)
    nat = NativeResNetFPN(ARCH, N, hw, "cuda", train=False, src=ref.state_dict())
    assert nat._layers["res5.0.c2"].group == 32 and nat._layers["res5.0.c2"].stride == 2
    assert nat._layers["res5.0.c2"].wcin == 64 and nat.params_flat.numel() == 0 and "sgd" not in nat.prog.marks
    assert sum(1 for o in nat.prog.ops if o.code == PR.GROUPED_CONV3X3) == 33
    images = torch.randn((N, 3) + hw, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    got = nat.forward(images)
    with torch.no_grad():
        want = ref(images)
    errs = [rel(g, w) for g, w in zip(got, want)]
    print("x101-32x8d rel P3..P7:", " ".join("%.3e" % e for e in errs))
    for g, w, e in zip(got, want, errs):
        assert tuple(g.shape) == tuple(w.shape)
        assert e < 2e-5, errs


# ---- 8. weights ----------------------------------------------------------------------------------------------------

SHAPES_128 = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]


def _blobs_from_capture(graph, rng):
    """tests/test_weights_file.reference_backbone_blobs for a capture that file's table does not list."""
    blobs = {}
    for prm in graph["params"]:
        name, shape = prm["name"], tuple(prm["shape"])
        if name.endswith("_bn_s"):
            v = rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape, p=[0.1, 0.9])
        elif name.endswith("_bn_b") or name.endswith("_b"):
            v = rng.standard_normal(shape) * 0.05
        else:
            v = rng.standard_normal(shape) * np.sqrt(2.0 / int(np.prod(shape[1:]))) * (0.25 if "branch2c" in name else 1.0)
        blobs[name] = v.astype(np.float32)
    return blobs


def test_weights_file_drives_the_32x8d_teacher(tmp_path, golden_dir):
    from ssad_amd import synth
    from ssad_amd.backbone_pipeline import NativeResNetFPN
    from ssad_amd.head_pipeline import DistillHeads
    from ssad_amd.modeling.retinanet_heads import HeadConfig
    from ssad_amd.utils import net
    from test_weights_file import reference_backbone_blobs
    rng = np.random.default_rng(328)
    s_blobs, _ = reference_backbone_blobs("r50", rng)
    t_graph = json.load(open(os.path.join(golden_dir, "backbone_graph_x101_32x8d_fpn.json")))
    t_blobs = _blobs_from_capture(t_graph, rng)           # a teacher's own file: the loader adds the teacher/ scope
    s_blobs.update(synth.head_params(rng))
    t_blobs.update(synth.head_params(rng))
    s_path, t_path = str(tmp_path / "R-50.pkl"), str(tmp_path / "X-101-32x8d.pkl")
    for path, blobs in ((s_path, s_blobs), (t_path, t_blobs)):
        with open(path, "wb") as f:
            pickle.dump(dict(blobs=dict(blobs), cfg=""), f, protocol=2)
    N, hw = 1, (128, 128)
    heads = DistillHeads(HeadConfig(num_gpus=1), N=N, shapes=SHAPES_128, device="cuda", lr=1e-3)
    model, loaded, missing = net.native_model_from_weights_files(
        heads, s_path, t_path, student_arch="r50", teacher_arch=ARCH, N=N, image_hw=hw, device="cuda", lr=1e-3)
    assert not missing and "teacher/res5_2_branch2b_w" in loaded and "teacher/res4_22_branch2c_bn_s" in loaded
    state, scales, _, miss = net.backbone_from_blobs(t_blobs, ARCH)
    assert not miss
    twin = NativeResNetFPN(ARCH, N, hw, "cuda", train=False, src=state, affine_scales=scales)
    images = torch.randn((N, 3) + hw, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    got = [t.clone() for t in model.teacher.forward(images)]
    want = twin.forward(images)
    for l, (g, w) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(w).all()) and float(w.abs().max()) > 0
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), "P%d" % (l + 3)


# ---- 9. the step ---------------------------------------------------------------------------------------------------

def test_distill_step_with_the_32x8d_teacher_two_streams_change_nothing():
    from ssad_amd import synth
    from ssad_amd.backbone_pipeline import NativeDistillModel
    from ssad_amd.head_pipeline import DistillHeads
    from ssad_amd.modeling.retinanet_heads import HeadConfig
    N, hw = 1, (128, 128)
    rng = np.random.default_rng(9)
    labs = [synth.distill_inputs(rng, N, 9, 80, h, w)[2] for h, w in SHAPES_128]
    tg = [synth.bbox_targets(rng, l) for l in labs]
    to = lambda a: torch.from_numpy(a).to("cuda")
    labels, targets = [to(a) for a in labs], [(to(y), to(l)) for y, l in tg]
    fg = torch.tensor([float(max(1, sum(t[0].shape[0] for t in tg)))], device="cuda")
    images = torch.randn((N, 3) + hw, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))

    def run(two_streams):
        torch.manual_seed(0)
        heads = DistillHeads(HeadConfig(num_gpus=1), N=N, shapes=SHAPES_128, device="cuda", lr=1e-3,
                             student_init=synth.head_params(np.random.default_rng(1)),
                             teacher_init=synth.head_params(np.random.default_rng(2)))
        m = NativeDistillModel(heads, "r50", ARCH, N=N, image_hw=hw, device="cuda", two_streams=two_streams)
        assert (m.side is not None) == two_streams and m.teacher.arch == ARCH and not m.teacher.train
        losses = []
        for _ in range(2):
            m.step(images, labels, targets, fg)
            losses.append(m.heads.losses.clone())
        torch.cuda.synchronize()
        return losses, m.student.params_flat.clone(), m.heads.params.flat.clone()

    a, b = run(True), run(False)
    for la, lb in zip(a[0], b[0]):
        assert bool(torch.isfinite(la).all())
        assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert bool(torch.isfinite(a[1]).all())
