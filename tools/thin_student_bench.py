"""ms/step of the whole distillation step at config 3's size -- batch 16, 640 x 896, ResNet-101 teacher -- for a
ResNet-50 student of RESNETS.CHANNEL_RATIO 1.0, 0.5 and 0.25 (backbone_pipeline.NativeDistillModel,
student_channel_ratio).  Report only: nobody has set a target for a thin step.  Writes profiles/thin_student.md.

Timing: the three models live in ONE process and take turns (--rounds rounds of --steps steps each, in the order
1.0, 0.5, 0.25, 1.0, ...), HIP events around each block of steps on the launch stream; the figure of a ratio is the
median over its blocks.  Afterwards --profile-steps instrumented steps per model (program.Timing: events around every
launch, which keeps kernels from overlapping -- the per-class table is not a breakdown of the step time above).
Prints one JSON line.

    python tools/thin_student_bench.py [--steps 5] [--rounds 4] [--warmup 3] [--out profiles/thin_student.md]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATIOS = (1.0, 0.5, 0.25)
N, IMAGE_HW = 16, (640, 896)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=N)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thin_student.md"))
    args = ap.parse_args()
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd import program as PR, synth
    from ssad_amd.backbone_pipeline import NativeDistillModel, student_widths
    from ssad_amd.head_pipeline import DistillHeads
    from ssad_amd.modeling.retinanet_heads import HeadConfig
    if not torch.cuda.is_available():
        raise SystemExit("thin_student_bench needs a GPU: nothing is estimated without one")
    dev = torch.device("cuda", 0)
    shapes, n = synth.LEVEL_SHAPES_600, args.batch
    gen = torch.Generator(device=dev).manual_seed(1234)
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
    for r in RATIOS:
        dim = student_widths("r50", r).fpn_dim
        heads = DistillHeads(HeadConfig(num_gpus=1, fpn_dim=dim), N=n, shapes=shapes, device=dev,
                             student_init=synth.head_params(np.random.default_rng(1), dim=dim),
                             teacher_init=synth.head_params(np.random.default_rng(2)), lr=1e-4,
                             teacher_fpn_dim=256)
        models[r] = NativeDistillModel(heads, "r50", "r101", N=n, image_hw=IMAGE_HW, device=dev,
                                       student_channel_ratio=r)
    for r in RATIOS:
        for _ in range(args.warmup):
            models[r].step(images, labels, targets, fg_num)
    torch.cuda.synchronize()
    blocks = {r: [] for r in RATIOS}
    for _ in range(args.rounds):
        for r in RATIOS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                models[r].step(images, labels, targets, fg_num)
            e1.record()
            e1.synchronize()
            blocks[r].append(e0.elapsed_time(e1) / args.steps)
    classes = {}
    for r in RATIOS:
        t = PR.Timing()
        models[r].heads.timing = t
        models[r].timing = t
        for _ in range(args.profile_steps):
            models[r].step(images, labels, targets, fg_num)
        torch.cuda.synchronize()
        classes[r] = t.collect()
        models[r].heads.timing = None
        models[r].timing = None
        assert bool(torch.isfinite(models[r].heads.losses).all()) and bool(torch.isfinite(models[r].student.params_flat).all())

    res = {"metric": "thin_student_ms_per_step", "batch": n, "image_hw": list(IMAGE_HW), "teacher": "r101",
           "student": "r50", "steps_per_block": args.steps, "rounds": args.rounds, "ratios": {}}
    for r in RATIOS:
        b = sorted(blocks[r])
        st = models[r].student
        res["ratios"][str(r)] = dict(ms_per_step=round(float(np.median(b)), 3), min=round(b[0], 3), max=round(b[-1], 3),
                                     fpn_dim=st.D, student_parameters=int(st.params_flat.numel() + st.frozen_flat.numel()
                                                                          + models[r].heads.params.flat.numel()))
    lines = ["# The distillation step with a thin student", "",
             "`python tools/thin_student_bench.py` on one MI355X: batch %d, %d x %d, ResNet-101 teacher at full width, "
             "ResNet-50 student of `student_channel_ratio` 1.0 / 0.5 / 0.25 (FPN dimension 256 / 128 / 64), fp32, one GPU, "
             "synthetic images and labels.  The three models live in one process and take turns: %d rounds of %d "
             "steps each, HIP events around every block, %d warm-up steps per model; median (min ... max) over a "
             "ratio's blocks." % (n, IMAGE_HW[0], IMAGE_HW[1], args.rounds, args.steps, args.warmup), "",
             "| student ratio | FPN dim | student parameters | ms / step | min ... max |", "|---|---|---|---|---|"]
    for r in RATIOS:
        e = res["ratios"][str(r)]
        lines.append("| %.2f | %d | %.2f M | %.2f | %.2f ... %.2f |" % (r, e["fpn_dim"], e["student_parameters"] / 1e6,
                                                                     e["ms_per_step"], e["min"], e["max"]))
    lines += ["", "The teacher's forward pass (ResNet-101, full width, on its own stream) is the same work in all three "
              "rows; only the student's share of the step shrinks.  The engine thresholds were measured at ratio 1.0 "
              "and were not retuned for the thin layers (DESIGN 3.13).", "",
              "These are figures of one run on one machine.  Machines of the same model differ by several per cent in "
              "step time (clocks, power state, what else runs on the host), so the rows are comparable with each other "
              "-- same process, interleaved -- but not with a figure taken on another machine or in another run, such "
              "as bench.py's headline.  No bar was set for these numbers; nothing was tuned against them.", "",
              "## Per kernel class", "",
              "From %d instrumented steps per model after the timed blocks (`program.Timing`: events around every "
              "launch, so kernels that overlap in the timed step run one after the other here and the columns do not "
              "add up to the step times above).  ms per step, both backbones and the subnets; classes below 0.05 ms in "
              "every column are left out." % args.profile_steps, "",
              "| class | kernel family | ratio 1.0 | ratio 0.5 | ratio 0.25 |", "|---|---|---|---|---|"]
    keys = sorted(set(k for r in RATIOS for k in classes[r]))
    table = {}
    for k in keys:
        row = [classes[r].get(k, dict(ms=0.0))["ms"] / args.profile_steps for r in RATIOS]
        if max(row) < 0.05:
            continue
        name = PR.KLASS.get(k, dict(name="class %d" % k))["name"]
        table[k] = [round(v, 3) for v in row]
        lines.append("| %d | %s | %.2f | %.2f | %.2f |" % (k, name, row[0], row[1], row[2]))
    tot = [sum(c["ms"] for c in classes[r].values()) / args.profile_steps for r in RATIOS]
    lines.append("| | sum of all classes | %.2f | %.2f | %.2f |" % tuple(tot))
    res["classes_ms_per_step"] = table
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
