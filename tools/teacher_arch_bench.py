"""The ResNeXt-101-32x8d teacher beside the other two teachers, and its 64-wide grouped 3x3 kernel beside its 32-wide
sibling and the `Conv` operator.  Report only: nobody has measured a 64-wide grouped layer on this chip, so no time is
fixed anywhere.  Writes profiles/x101_32x8d.md and prints one JSON line.

Everything is timed in ONE process, every timed shape warmed, the alternatives of a comparison taking turns:

 (a) res5's grouped layers of 32x8d (2048 channels, 32 groups of 64) at config 3's maps (N 16, 640 x 896 images:
     40 x 56 -> 20 x 28 at stride 2, 20 x 28 at stride 1 -- res5 has one stride-2 and two stride-1 layers) and at
     config 5's (512 x 768: 32 x 48 -> 16 x 24, 16 x 24), on
       * grouped_conv3x3_cg64_kernel;
       * the cg = 32 kernel on the same maps (C 2048, G 64), which executes exactly half the flops;
       * the `Conv` operator's default engine with group = 32 (workspace.RunOperatorOnce), the only route such a layer
         had before.  Device events cannot bracket the operator's own stream, so it is timed by the host clock around
         RunOperatorOnce + a device synchronise (operator construction included).
     Executed flops = 2 * 9 * cg * C * N * OH * OW over the device-event time of a block of launches.
 (b) the frozen teacher's forward pass for r101, x101-64x4d and x101-32x8d at bs 16, 640 x 896;
 (c) the config-3-shaped distillation step (ResNet-50 student) with each of the three teachers;
 (d) the FPN outputs of both ResNeXts against the float64 torch network at 1 x 128 x 256 (tests/torch_ref*.py), the
     figure tests/test_gpu_x101_32x8d.py bounds.

    python tools/teacher_arch_bench.py [--rounds 4] [--reps 10] [--steps 3] [--warmup 2] [--out profiles/x101_32x8d.md]

--precision f16: the same teacher in fp16 storage (NativeResNetFPNF16(wide_groups=True), the 64-wide mode of
grouped_f16_kernel).  Writes profiles/x101_32x8d_f16.md:

 (a) the three 64-wide res5 layers at N 16, 640 x 896 (res5.0 at stride 1 on res4's 40 x 56 map followed by the pass
     that keeps the even positions, as the network runs it; res5.1 / res5.2 on 20 x 28), the fp16 kernel taking turns
     with its 32-wide sibling on the same maps (half the flops) and with the fp32 64-wide kernel on the same layer;
 (b) the fp16 teacher's forward pass for x101-64x4d and x101-32x8d at N 16, 640 x 896;
 (c) the config-5-shaped step (ResNet-101 student, 512 x 768, fp16 storage everywhere) under each of the two teachers;
 (d) the FPN outputs of the fp16 32x8d teacher against float64 torch at 1 x 128 x 128, the figure
     tests/test_gpu_x101_32x8d_f16.py bounds."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEACHERS = ("r101", "x101-64x4d", "x101-32x8d")
N, IMAGE_HW = 16, (640, 896)
C5 = 2048
PEAK_F32_MFMA = 157.3e12          # MI355X, dense fp32 MFMA
KERNEL_SRC = os.path.join(ROOT, "semi-supervised-adaptive-distillation_amd", "csrc", "kernels", "grouped_conv3x3.hip")
KERNEL_SRC_F16 = os.path.join(os.path.dirname(KERNEL_SRC), "grouped_f16.hip")
F16_CG64_KERNEL = "grouped_f16_kernelILb1ELi1ELb1EE"      # grouped_f16_kernel<WIDE, NG = 1, CG64> in the remarks
PEAK_F16_MFMA, PEAK_HBM = 2.5e15, 8.0e12
FP32_PROFILE = dict(layer_ms=(0.30, 0.27), teacher_forward_ms=40.4)      # profiles/x101_32x8d.md
# (label, res4 map H x W, stride)
LAYERS = [("config 3, res5.0 (stride 2)", 40, 56, 2), ("config 3, res5.1 / res5.2 (stride 1)", 20, 28, 1),
          ("config 5, res5.0 (stride 2)", 32, 48, 2), ("config 5, res5.1 / res5.2 (stride 1)", 16, 24, 1)]


def resource_lines(path=None, src=KERNEL_SRC, match=("cg64",)):
    """The compiler's register / LDS / scratch remarks for the kernels of `src` whose name holds one of `match`: from
    `path`, else from hipcc here."""
    if path:
        text = open(path).read()
    else:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-I" + os.path.join(ROOT, "include"),
               "-I" + os.path.dirname(os.path.dirname(src)), "-Rpass-analysis=kernel-resource-usage", "-c", src,
               "-o", os.devnull]
        text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True).stdout
    out, keep = [], False
    for line in text.splitlines():
        m = re.search(r"remark: (.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            keep = any(m_ in body for m_ in match)
        if keep:
            out.append(body)
    return out


def summary(v):
    v = sorted(v)
    return dict(median=float(np.median(v)), min=v[0], max=v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10, help="launches per timed block of a grouped layer")
    ap.add_argument("--steps", type=int, default=3, help="forward passes / steps per timed block")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=N)
    ap.add_argument("--resource-usage", default=None, help="file with hipcc's -Rpass-analysis=kernel-resource-usage "
                    "output for grouped_conv3x3.hip, or grouped_f16.hip with --precision f16 (default: run hipcc)")
    ap.add_argument("--precision", choices=("f32", "f16"), default="f32")
    ap.add_argument("--out", default=None, help="default: profiles/x101_32x8d.md, profiles/x101_32x8d_f16.md for f16")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "x101_32x8d.md" if args.precision == "f32" else "x101_32x8d_f16.md")
    if args.precision == "f16":
        return main_f16(args)
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd import kernels as K, synth
    from ssad_amd.backbone_pipeline import NativeDistillModel, NativeResNetFPN
    from ssad_amd.caffe2_hip import caffe2_pb2, core, dyndep, workspace
    from ssad_amd.head_pipeline import DistillHeads
    from ssad_amd.modeling.retinanet_heads import HeadConfig
    if not torch.cuda.is_available():
        raise SystemExit("teacher_arch_bench needs a GPU: nothing is estimated without one")
    dev = torch.device("cuda", 0)
    n = args.batch
    gen = torch.Generator(device=dev).manual_seed(1234)
    res = {"metric": "teacher_arch_bench", "batch": n, "image_hw": list(IMAGE_HW), "rounds": args.rounds,
           "reps_per_block": args.reps, "steps_per_block": args.steps, "layers": [], "teacher_forward_ms": {},
           "step_ms": {}, "rel_vs_float64": {}}

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    # ---- (a) the grouped layers -----------------------------------------------------------------------------------
    dyndep.InitOpsLibrary()
    GPU = core.DeviceOption(caffe2_pb2.CUDA, 0)
    for label, H, W, s in LAYERS:
        oh, ow = (H - 1) // s + 1, (W - 1) // s + 1
        x = torch.randn((n, C5, H, W), device=dev, generator=gen)
        run, flops = {}, {}
        for cg in (64, 32):
            G = C5 // cg
            w = torch.randn((C5, cg, 3, 3), device=dev, generator=gen) * float((9 * cg) ** -0.5)
            b = torch.randn((C5,), device=dev, generator=gen)
            pf = K.grouped_conv3x3_pack_filter(w, G)
            y = torch.empty((n, C5, oh, ow), device=dev)
            run[cg] = (lambda G=G, b=b, pf=pf, y=y: K.grouped_conv3x3_forward(x, None, b, group=G, stride=s, relu=True,
                                                                              out=y, packed=pf))
            flops[cg] = 2.0 * 9 * cg * C5 * n * oh * ow
            if cg == 64:
                w64, b64, y64 = w, b, y
        workspace.ResetWorkspace()
        workspace.FeedBlob("X", x.cpu().numpy(), device_option=GPU)
        workspace.FeedBlob("w", w64.cpu().numpy(), device_option=GPU)
        workspace.FeedBlob("b", b64.cpu().numpy(), device_option=GPU)
        with core.DeviceScope(GPU):
            op = core.CreateOperator("Conv", ["X", "w", "b"], ["Y"], kernel=3, pad=1, stride=s, group=32, order="NCHW")

        def run_op():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            workspace.RunOperatorOnce(op)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        for _ in range(args.warmup):
            run[64](); run[32](); run_op()
        torch.cuda.synchronize()
        # the operator and the kernel compute the same layer (the operator has no ReLU)
        yo = torch.from_numpy(workspace.FetchBlob("Y")).to(dev)
        run[64]()
        agree = float((y64 - yo.clamp_min(0)).abs().max() / yo.abs().max())
        t = {64: [], 32: [], "op": []}
        for _ in range(args.rounds):
            t[64].append(timed(run[64], args.reps))
            t[32].append(timed(run[32], args.reps))
            t["op"].append(run_op())
        workspace.ResetWorkspace()
        e = dict(layer=label, N=n, C=C5, H=H, W=W, stride=s, OH=oh, OW=ow,
                 cg64_ms=summary(t[64]), cg32_ms=summary(t[32]), conv_operator_ms=summary(t["op"]),
                 max_abs_diff_vs_operator_of_scale=agree)
        e["cg64_tflops"] = flops[64] / (e["cg64_ms"]["median"] * 1e-3) / 1e12
        e["cg32_tflops"] = flops[32] / (e["cg32_ms"]["median"] * 1e-3) / 1e12
        e["cg64_share_of_fp32_mfma_peak"] = e["cg64_tflops"] * 1e12 / PEAK_F32_MFMA
        e["cg64_over_cg32_time"] = e["cg64_ms"]["median"] / e["cg32_ms"]["median"]
        e["cg32_spread"] = (e["cg32_ms"]["max"] - e["cg32_ms"]["min"]) / e["cg32_ms"]["median"]
        e["operator_over_cg64_time"] = e["conv_operator_ms"]["median"] / e["cg64_ms"]["median"]
        res["layers"].append(e)
        del x, run, yo

    # ---- (d) accuracy of both ResNeXts against float64 torch ------------------------------------------------------------
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from torch_ref import RefResNetFPN
    from torch_ref_x32 import RefX32ResNetFPN
    small = torch.randn((1, 3, 128, 256), device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    for arch, ref in (("x101-64x4d", RefResNetFPN("x101-64x4d", seed=13)), ("x101-32x8d", RefX32ResNetFPN(seed=13))):
        nat = NativeResNetFPN(arch, 1, (128, 256), dev, train=False, src=ref.state_dict())
        got = nat.forward(small)
        with torch.no_grad():
            want = ref(small)
        res["rel_vs_float64"][arch] = [float((g.double() - w_).norm() / w_.norm()) for g, w_ in zip(got, want)]
        del nat, ref, got, want

    # ---- (b), (c) the teachers' forward passes and the whole step -----------------------------------------------------------
    shapes = synth.LEVEL_SHAPES_600
    labels = []
    for h, w in shapes:                       # bench.py's synthetic labels: 5 % ignored, 2 % foreground
        u = torch.rand((n, 9, h, w), device=dev, generator=gen)
        lab = torch.zeros((n, 9, h, w), dtype=torch.int32, device=dev)
        lab[u < 0.05] = -1
        fg = (u >= 0.05) & (u < 0.07)
        lab[fg] = torch.randint(1, 81, (int(fg.sum()),), device=dev, generator=gen, dtype=torch.int32)
        labels.append(lab)
    targets, n_fg = [], 0
    for lab in labels:
        idx = torch.nonzero(lab > 0)
        Lc = torch.stack([idx[:, 0], 4 * idx[:, 1], idx[:, 2], idx[:, 3]], dim=1).float().contiguous()
        targets.append(((torch.randn((Lc.shape[0], 4), device=dev, generator=gen) * 0.5).contiguous(), Lc))
        n_fg += Lc.shape[0]
    fg_num = torch.tensor([float(max(n_fg, 1))], device=dev)
    images = torch.randn((n, 3) + IMAGE_HW, device=dev, generator=gen)
    models = {}
    for arch in TEACHERS:
        heads = DistillHeads(HeadConfig(num_gpus=1), N=n, shapes=shapes, device=dev, lr=1e-4,
                             student_init=synth.head_params(np.random.default_rng(1)),
                             teacher_init=synth.head_params(np.random.default_rng(2)))
        models[arch] = NativeDistillModel(heads, "r50", arch, N=n, image_hw=IMAGE_HW, device=dev)
    for arch in TEACHERS:
        for _ in range(args.warmup):
            models[arch].teacher.forward(images)
    torch.cuda.synchronize()
    fwd = {a: [] for a in TEACHERS}
    for _ in range(args.rounds):
        for arch in TEACHERS:
            fwd[arch].append(timed(lambda: models[arch].teacher.forward(images), args.steps))
    for arch in TEACHERS:
        for _ in range(args.warmup):
            models[arch].step(images, labels, targets, fg_num)
    torch.cuda.synchronize()
    stp = {a: [] for a in TEACHERS}
    for _ in range(args.rounds):
        for arch in TEACHERS:
            stp[arch].append(timed(lambda: models[arch].step(images, labels, targets, fg_num), args.steps))
    for arch in TEACHERS:
        assert bool(torch.isfinite(models[arch].heads.losses).all())
        res["teacher_forward_ms"][arch] = summary(fwd[arch])
        res["step_ms"][arch] = summary(stp[arch])

    res["resource_usage"] = resource_lines(args.resource_usage)
    bits = os.path.join(ROOT, "tests", "golden", "grouped_bits.json")
    res["narrow_width_bits_from_commit"] = json.load(open(bits))["commit"] if os.path.exists(bits) else None
    write_profile(res, args)
    print(json.dumps(res))


def main_f16(args):
    import ctypes
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd import kernels as K, synth
    from ssad_amd.backbone_f16 import NativeResNetFPNF16
    from ssad_amd.backbone_pipeline import NativeDistillModel
    from ssad_amd.head_pipeline import DistillHeadsF16
    from ssad_amd.modeling.retinanet_heads import HeadConfig
    if not torch.cuda.is_available():
        raise SystemExit("teacher_arch_bench needs a GPU: nothing is estimated without one")
    dev = torch.device("cuda", 0)
    n = args.batch
    L = K.lib()
    gen = torch.Generator(device=dev).manual_seed(1234)
    archs = ("x101-64x4d", "x101-32x8d")
    res = {"metric": "teacher_arch_bench_f16", "batch": n, "image_hw": list(IMAGE_HW), "rounds": args.rounds,
           "reps_per_block": args.reps, "steps_per_block": args.steps, "layers": [], "teacher_forward_ms": {},
           "step_ms": {}, "step_image_hw": [512, 768]}

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    # ---- (a) the three 64-wide layers -----------------------------------------------------------------------------
    for label, H, W, s in (("res5.0 (stride 2: stride 1 + even positions)", 40, 56, 2), ("res5.1 / res5.2", 20, 28, 1)):
        x = torch.randn((n, C5, H, W), device=dev, generator=gen)
        b = torch.randn((C5,), device=dev, generator=gen)
        xb, yb = K.f16_pack_activations(x), torch.empty((n, C5 // 8, H, W, 8), dtype=torch.float16, device=dev)
        oh, ow = (H - 1) // s + 1, (W - 1) // s + 1
        ys = torch.empty((n, C5 // 8, oh, ow, 8), dtype=torch.float16, device=dev)
        w64 = torch.randn((C5, 64, 3, 3), device=dev, generator=gen) * float((9 * 64) ** -0.5)
        w32 = torch.randn((C5, 32, 3, 3), device=dev, generator=gen) * float((9 * 32) ** -0.5)
        pf64 = K.grouped_conv3x3_f16_cg64_pack_filter(w64, 32)
        pf32 = torch.empty(L.ssad_grouped_conv3x3_f16_filter_halves(C5, 64), dtype=torch.float16, device=dev)
        K._check(L.ssad_grouped_conv3x3_f16_pack_filter(K._ptr(w32), C5, 64, K._ptr(pf32), stream()), "cg 32 pack")
        p32 = K.grouped_conv3x3_pack_filter(w64, 32)
        y32 = torch.empty((n, C5, oh, ow), device=dev)

        def run64():
            K.grouped_conv3x3_f16_cg64(xb, pf64, b, C5, 32, relu=True, out=yb)

        def run32():
            K._check(L.ssad_grouped_conv3x3_f16(K._ptr(xb), K._ptr(pf32), K._ptr(b), n, C5, H, W, 64, 1, K._ptr(yb),
                                                stream()), "cg 32")

        def sub():
            K._check(L.ssad_f16_subsample(K._ptr(yb), n, C5, H, W, s, K._ptr(ys), stream()), "even positions")

        def run_f32():
            K.grouped_conv3x3_forward(x, None, b, group=32, stride=s, relu=True, out=y32, packed=p32)
        runs = {"cg64": run64, "cg32": run32, "f32": run_f32}
        if s != 1:
            runs["sub"] = sub
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        # the fp16 kernel and the fp32 kernel compute the same layer
        run64()
        if s != 1:
            sub()
        run_f32()
        got = K.f16_unpack_activations(ys if s != 1 else yb, C5)
        agree = float((got - y32).abs().max() / y32.abs().max())
        t = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                t[k].append(timed(fn, args.reps))
        e = dict(layer=label, N=n, C=C5, H=H, W=W, stride=s, OH=oh, OW=ow, cg64_ms=summary(t["cg64"]),
                 cg32_ms=summary(t["cg32"]), fp32_cg64_ms=summary(t["f32"]),
                 even_positions_ms=summary(t["sub"]) if s != 1 else None, max_abs_diff_vs_fp32_of_scale=agree)
        layer_ms = e["cg64_ms"]["median"] + (e["even_positions_ms"]["median"] if s != 1 else 0.0)
        flops, nbytes = 2.0 * 9 * 64 * C5 * n * H * W, 2.0 * 2 * n * C5 * H * W
        e["layer_ms"] = layer_ms
        e["cg64_tflops"] = flops / (e["cg64_ms"]["median"] * 1e-3) / 1e12
        e["cg64_tbytes_per_s"] = nbytes / (e["cg64_ms"]["median"] * 1e-3) / 1e12
        e["least_ms_flops"], e["least_ms_bytes"] = flops / PEAK_F16_MFMA * 1e3, nbytes / PEAK_HBM * 1e3
        e["cg64_share_of_bound"] = max(e["least_ms_flops"], e["least_ms_bytes"]) / e["cg64_ms"]["median"]
        e["cg64_over_cg32_time"] = e["cg64_ms"]["median"] / e["cg32_ms"]["median"]
        e["fp32_over_f16_layer_time"] = e["fp32_cg64_ms"]["median"] / layer_ms
        res["layers"].append(e)
        del x, xb, yb, ys, y32, runs

    # ---- (d) accuracy against float64 torch -----------------------------------------------------------------------------
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from torch_ref_x32 import RefX32ResNetFPN
    small = torch.randn((1, 3, 128, 128), device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    ref = RefX32ResNetFPN(seed=13)
    nat = NativeResNetFPNF16("x101-32x8d", 1, (128, 128), dev, train=False, src=ref.state_dict(), wide_groups=True)
    nat.forward(small)
    with torch.no_grad():
        want = ref(small)
    res["rel_vs_float64"] = [float((g.double() - w_).norm() / w_.norm()) for g, w_ in zip(nat.fpn_f32(), want)]
    del nat, ref, want

    # ---- (b) the fp16 teachers' forward passes --------------------------------------------------------------------------
    images = torch.randn((n, 3) + IMAGE_HW, device=dev, generator=gen)
    teachers = {a: NativeResNetFPNF16(a, n, IMAGE_HW, dev, train=False, wide_groups=True) for a in archs}
    for a in archs:
        for _ in range(args.warmup):
            teachers[a].forward(images)
    torch.cuda.synchronize()
    fwd = {a: [] for a in archs}
    for _ in range(args.rounds):
        for a in archs:
            fwd[a].append(timed(lambda: teachers[a].forward(images), args.steps))
    for a in archs:
        assert all(bool(torch.isfinite(p).all()) for p in teachers[a].fpn)
        res["teacher_forward_ms"][a] = summary(fwd[a])
    del teachers, images

    # ---- (c) the config-5-shaped step under each teacher ------------------------------------------------------------------
    hw5, shapes = (512, 768), synth.LEVEL_SHAPES_500
    labels = []
    for h, w in shapes:                       # bench.py's synthetic labels: 5 % ignored, 2 % foreground
        u = torch.rand((n, 9, h, w), device=dev, generator=gen)
        lab = torch.zeros((n, 9, h, w), dtype=torch.int32, device=dev)
        lab[u < 0.05] = -1
        fg = (u >= 0.05) & (u < 0.07)
        lab[fg] = torch.randint(1, 81, (int(fg.sum()),), device=dev, generator=gen, dtype=torch.int32)
        labels.append(lab)
    targets, n_fg = [], 0
    for lab in labels:
        idx = torch.nonzero(lab > 0)
        Lc = torch.stack([idx[:, 0], 4 * idx[:, 1], idx[:, 2], idx[:, 3]], dim=1).float().contiguous()
        targets.append(((torch.randn((Lc.shape[0], 4), device=dev, generator=gen) * 0.5).contiguous(), Lc))
        n_fg += Lc.shape[0]
    fg_num = torch.tensor([float(max(n_fg, 1))], device=dev)
    images = torch.randn((n, 3) + hw5, device=dev, generator=gen)
    models = {}
    for a in archs:
        heads = DistillHeadsF16(HeadConfig(num_gpus=1), N=n, shapes=shapes, device=dev, lr=1e-4, blocked_io=True,
                                student_init=synth.head_params(np.random.default_rng(1)),
                                teacher_init=synth.head_params(np.random.default_rng(2)))
        models[a] = NativeDistillModel(heads, "r101", a, N=n, image_hw=hw5, device=dev, teacher_wide_groups=True)
    for a in archs:
        for _ in range(args.warmup):
            models[a].step(images, labels, targets, fg_num)
    torch.cuda.synchronize()
    stp = {a: [] for a in archs}
    for _ in range(args.rounds):
        for a in archs:
            stp[a].append(timed(lambda: models[a].step(images, labels, targets, fg_num), args.steps))
    for a in archs:
        assert bool(torch.isfinite(models[a].heads.losses).all())
        res["step_ms"][a] = summary(stp[a])

    res["resource_usage"] = resource_lines(args.resource_usage, KERNEL_SRC_F16, (F16_CG64_KERNEL,))
    write_profile_f16(res, args)
    print(json.dumps(res))


def write_profile_f16(res, args):
    f3 = lambda d: "%.3f (%.3f ... %.3f)" % (d["median"], d["min"], d["max"])
    archs = ("x101-64x4d", "x101-32x8d")
    L = ["# ResNeXt-101-32x8d as an fp16-storage teacher: the 64-wide mode of the fp16 grouped 3x3 kernel", "",
         "`python tools/teacher_arch_bench.py --precision f16` on one MI355X, batch %d.  One process; every timed shape "
         "warmed (%d passes); the alternatives of a comparison take turns, %d rounds; median (min ... max) over the "
         "rounds.  Figures of one run on one machine: rows of one table are comparable with each other, not with a "
         "figure taken in another run.  No speed is gated anywhere." % (res["batch"], args.warmup, args.rounds), "",
         "## The three 64-wide res5 layers (2048 channels, 32 groups of 64, %d x %d images)" % tuple(res["image_hw"]), "",
         "`fp16 cg 64`: `grouped_f16_kernel<true, 1, true>` (`ssad_grouped_conv3x3_f16_cg64`).  `fp16 cg 32`: the same "
         "kernel's 32-wide mode on the same maps (64 groups of 32: half the flops, the same bytes).  `fp32 cg 64`: "
         "`grouped_conv3x3_cg64_kernel` on the same layer, at its own stride.  res5.0 runs at stride 1 on res4's map and "
         "a pass keeps the even positions (`even positions ms`); `layer ms` is the sum, what the network spends.  "
         "Device events around blocks of %d launches, ms per launch.  The least time the hardware could take is the "
         "larger of flops over the %.1f PF/s dense fp16 MFMA peak and algorithmic bytes (input + output, fp16) over %.0f "
         "TB/s; `share` is that over the kernel's time." % (args.reps, PEAK_F16_MFMA / 1e15, PEAK_HBM / 1e12), "",
         "| layer (N %d) | map | fp16 cg 64 ms | TFLOP/s | TB/s | least ms (flops / bytes) | share | fp16 cg 32 ms | "
         "cg 64 / cg 32 | even positions ms | layer ms | fp32 cg 64 ms | fp32 / fp16 layer |" % res["batch"],
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for e in res["layers"]:
        L.append("| %s | %dx%d | %s | %.0f | %.2f | %.4f / %.4f | %.0f %% | %s | %.2f | %s | %.3f | %s | %.2f x |" % (
            e["layer"], e["H"], e["W"], f3(e["cg64_ms"]), e["cg64_tflops"], e["cg64_tbytes_per_s"], e["least_ms_flops"],
            e["least_ms_bytes"], 100 * e["cg64_share_of_bound"], f3(e["cg32_ms"]), e["cg64_over_cg32_time"],
            f3(e["even_positions_ms"]) if e["even_positions_ms"] else "-", e["layer_ms"], f3(e["fp32_cg64_ms"]),
            e["fp32_over_f16_layer_time"]))
    L += ["", "`profiles/x101_32x8d.md` (another run) has the fp32 layers at %.2f / %.2f ms.  The fp16 result was compared "
          "with the fp32 kernel's on both shapes before timing (largest difference as a fraction of the largest output, "
          "operand rounding included: %s)." % (FP32_PROFILE["layer_ms"] + (
              ", ".join("%.1e" % e["max_abs_diff_vs_fp32_of_scale"] for e in res["layers"]),)), ""]
    slower = [e["layer"] for e in res["layers"] if e["fp32_over_f16_layer_time"] <= 1.0]
    if slower:
        L += ["**Not faster than its fp32 sibling:** %s.  The fp32 kernel runs a stride-2 layer at stride 2 and computes "
              "a quarter of the positions; the fp16 kernel has no stride-2 form, computes all of them at stride 1 and "
              "pays a second pass over the full map to drop three quarters (a true stride-2 form is out of scope here)."
              % "; ".join(slower), ""]
    L += ["## What the compiler made of the kernel", "",
          "`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on `csrc/kernels/grouped_f16.hip`, "
          "the 64-wide instance:", "", "```"]
    L += res["resource_usage"] or ["(not available where this ran)"]
    L += ["```", "", "## The two fp16 teachers", "",
          "Forward pass of the frozen fp16 teacher alone (%d x %d) and the whole config-5-shaped step (ResNet-101 student, "
          "%d x %d, fp16 storage in both backbones and the subnets), ms; blocks of %d passes.  The fp32 32x8d teacher's "
          "forward pass is %.1f ms in `profiles/x101_32x8d.md` (another run)."
          % (res["image_hw"][0], res["image_hw"][1], res["step_image_hw"][0], res["step_image_hw"][1], args.steps,
             FP32_PROFILE["teacher_forward_ms"]), "", "| teacher | fp16 forward ms | config-5-shaped step ms |", "|---|---|---|"]
    for a in archs:
        L.append("| %s | %s | %s |" % (a, f3(res["teacher_forward_ms"][a]), f3(res["step_ms"][a])))
    L += ["", "## Accuracy against float64", "",
          "FPN levels P3..P7 of `NativeResNetFPNF16('x101-32x8d', wide_groups=True)` against the float64 torch network "
          "on the same weights, 1 x 128 x 128, relative L2 (`tests/test_gpu_x101_32x8d_f16.py` bounds each at 1.5e-2, the "
          "64x4d fp16 teacher test's bound):", "", "| P3 | P4 | P5 | P6 | P7 |", "|---|---|---|---|---|",
          "| %s |" % " | ".join("%.2e" % x for x in res["rel_vs_float64"])]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(L) + "\n")


def write_profile(res, args):
    f3 = lambda d: "%.3f (%.3f ... %.3f)" % (d["median"], d["min"], d["max"])
    L = ["# ResNeXt-101-32x8d as a teacher: the grouped 3x3 kernel for 64-wide groups", "",
         "`python tools/teacher_arch_bench.py` on one MI355X, fp32, batch %d.  One process; every timed shape warmed "
         "(%d passes); the alternatives of a comparison take turns, %d rounds; median (min ... max) over the rounds.  "
         "These are figures of one run on one machine: rows of one table are comparable with each other, not with a "
         "figure taken in another run." % (res["batch"], args.warmup, args.rounds), "",
         "## res5's grouped layers (2048 channels)", "",
         "`cg 64`: `grouped_conv3x3_cg64_kernel`, 32 groups of 64.  `cg 32`: the existing kernel on the same maps, 64 "
         "groups of 32 -- exactly half the flops.  `Conv operator`: the default engine of the `Conv` operator with "
         "`group=32` through `workspace.RunOperatorOnce`, the only route a 64-wide grouped layer had before (host clock "
         "around the call and a device synchronise, operator construction included).  Kernel times are device events "
         "around blocks of %d launches, ms per launch.  TFLOP/s = executed flops `2*9*cg*C*N*OH*OW` over that time; the "
         "share is of the %.1f TF/s dense fp32 MFMA peak.  The bound of this layer is compute: at cg = 64 it needs 1152 "
         "flops per input float staged, far above the chip's flop-to-byte ratio, so operations over the peak rate is the "
         "larger of the two lower bounds." % (args.reps, PEAK_F32_MFMA / 1e12), "",
         "| layer (N %d) | map | cg 64 ms | TFLOP/s | share of peak | cg 32 ms | cg 32 TFLOP/s | cg 64 / cg 32 time | "
         "cg 32 spread | Conv operator ms | operator / cg 64 |" % res["batch"], "|---|---|---|---|---|---|---|---|---|---|---|"]
    for e in res["layers"]:
        L.append("| %s | %dx%d -> %dx%d | %s | %.1f | %.1f %% | %s | %.1f | %.2f | %.1f %% | %s | %.1f x |" % (
            e["layer"], e["H"], e["W"], e["OH"], e["OW"], f3(e["cg64_ms"]), e["cg64_tflops"],
            100 * e["cg64_share_of_fp32_mfma_peak"], f3(e["cg32_ms"]), e["cg32_tflops"], e["cg64_over_cg32_time"],
            100 * e["cg32_spread"], f3(e["conv_operator_ms"]), e["operator_over_cg64_time"]))
    L += ["", "The yardstick for the new kernel is its sibling's per-flop rate: twice the flops at twice the arithmetic "
          "intensity per staged input byte should take at most twice the time, within the spread of the sibling's own "
          "repeats (`cg 32 spread` = (max - min) / median over the rounds).  The kernel's output was compared with the "
          "operator's on every shape before timing (largest difference, as a fraction of the largest output: %s)."
          % ", ".join("%.1e" % e["max_abs_diff_vs_operator_of_scale"] for e in res["layers"]), "",
          "Read from the code, not measured: maps of 20 x 28 and 16 x 24 outputs leave part of the 8 x 16 tiles empty "
          "(20 rows = 2.5 tiles, 28 columns = 1.75 tiles); row pairs below the map are skipped, columns beyond it are "
          "multiplied and masked, so the share of peak above understates what the MFMA pipe does on the tiles it is "
          "given.  The cg 32 kernel stages a workgroup's whole halo before its first MFMA; the cg 64 kernel fetches the "
          "next channel chunk into registers while it multiplies the current one, which is where its better rate per "
          "flop comes from, most of all at stride 2 (four times the staged floats per output).", "",
          "## What the compiler made of the kernel", "",
          "`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on "
          "`csrc/kernels/grouped_conv3x3.hip`, the two instances of the 64-wide kernel (stride 1, stride 2):", "", "```"]
    L += res["resource_usage"] or ["(not available where this ran)"]
    L += ["```", "", "## The three teachers", "",
          "Forward pass of the frozen teacher alone and the whole config-3-shaped distillation step (ResNet-50 student, "
          "%d x %d), ms; blocks of %d passes." % (res["image_hw"][0], res["image_hw"][1], args.steps), "",
          "| teacher | forward ms | step ms |", "|---|---|---|"]
    for a in TEACHERS:
        L.append("| %s | %s | %s |" % (a, f3(res["teacher_forward_ms"][a]), f3(res["step_ms"][a])))
    L += ["", "## Accuracy against float64", "",
          "FPN levels P3..P7 of the native network against the float64 torch network on the same weights, 1 x 128 x 256, "
          "relative L2 (`tests/test_gpu_x101_32x8d.py` bounds 32x8d at 2e-5, the 64x4d teacher test's own bound):", "",
          "| network | P3 | P4 | P5 | P6 | P7 |", "|---|---|---|---|---|---|"]
    for a, v in res["rel_vs_float64"].items():
        L.append("| %s | %s |" % (a, " | ".join("%.2e" % x for x in v)))
    L += ["", "## The narrower widths", "",
          "`tests/golden/grouped_bits.json` pins the sha256 of the raw output words of the cg = 4, 8, 16 and 32 paths at "
          "the shapes of `test_grouped_conv3x3_vs_oracle`.  They were produced on an MI355X by the kernel file of commit "
          "`%s` (the parent of the commit that added the 64-wide kernel), built on its own, in the same visit in which "
          "the library of this tree gave the same words." % res["narrow_width_bits_from_commit"]]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(L) + "\n")


if __name__ == "__main__":
    main()
