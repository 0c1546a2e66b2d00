"""ms/step of the RetinaNet subnets with RETINANET.SHARE_CLS_BBOX_TOWER / RETINANET.CLASS_SPECIFIC_BBOX
(HeadConfig.share_cls_bbox_tower / class_specific_bbox) against the separate-tower, class-agnostic heads:

  * the subnet step (head_pipeline.DistillHeads.step on fixed FPN tensors) at config 2's size (student only, batch 2,
    600 px) and at config 3's (distillation, batch 16, 600 px): default, shared tower, class-specific, both;
  * the whole config-3 step (backbone_pipeline.NativeDistillModel, ResNet-50 student under a ResNet-101 teacher,
    batch 16, 640 x 896) with and without the shared tower.

Every group holds the DEFAULT heads twice ("default", "default again"): two objects of the same code that take turns
with the others, so the difference between them is the run-to-run spread this tool shows for identical work; a
difference inside it is reported as "no difference".  All variants of a group live in ONE process and take turns
(--rounds rounds of --steps steps, HIP events around each block); the figure is the median over a variant's blocks.
Afterwards --profile-steps instrumented steps per subnet variant (program.Timing: events around every launch, which
keeps launches from overlapping -- the per-class table is not a breakdown of the step times).
Report only: no bar was set.  Writes profiles/head_options.md and prints one JSON line.

    python tools/head_options_bench.py [--steps 5] [--rounds 5] [--warmup 3] [--skip-full] [--out profiles/head_options.md]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMAGE_HW = (640, 896)
VARIANTS = (("default", {}), ("default again", {}), ("shared tower", dict(share_cls_bbox_tower=True)),
            ("shared tower, two-pass", dict(share_cls_bbox_tower=True, shared_accumulate=False)),
            ("class-specific", dict(class_specific_bbox=True)),
            ("both", dict(share_cls_bbox_tower=True, class_specific_bbox=True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=2)
    ap.add_argument("--skip-full", action="store_true", help="leave out the whole config-3 step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_options.md"))
    args = ap.parse_args()
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd import program as PR, synth
    from ssad_amd.backbone_pipeline import NativeDistillModel
    from ssad_amd.head_pipeline import DistillHeads
    from ssad_amd.modeling.retinanet_heads import HeadConfig
    if not torch.cuda.is_available():
        raise SystemExit("head_options_bench needs a GPU: nothing is estimated without one")
    dev = torch.device("cuda", 0)
    shapes = synth.LEVEL_SHAPES_600
    gen = torch.Generator(device=dev).manual_seed(1234)

    def inputs(n):
        labels = []
        for h, w in shapes:                       # bench.py's synthetic labels: 5 % ignored, 2 % foreground
            u = torch.rand((n, 9, h, w), device=dev, generator=gen)
            lab = torch.zeros((n, 9, h, w), dtype=torch.int32, device=dev)
            lab[u < 0.05] = -1
            fg = (u >= 0.05) & (u < 0.07)
            lab[fg] = torch.randint(1, 81, (int(fg.sum()),), device=dev, generator=gen, dtype=torch.int32)
            labels.append(lab)
        targets = {False: [], True: []}
        n_fg = 0
        for lab in labels:
            idx = torch.nonzero(lab > 0)
            cls = lab[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]].long()
            Y = (torch.randn((idx.shape[0], 4), device=dev, generator=gen) * 0.5).contiguous()
            for specific in (False, True):        # column 1 as the labeller writes it for either head
                ch = 4 * (cls - 1) + 320 * idx[:, 1] if specific else 4 * idx[:, 1]
                targets[specific].append((Y, torch.stack([idx[:, 0], ch, idx[:, 2], idx[:, 3]], dim=1).float().contiguous()))
            n_fg += idx.shape[0]
        fpn = [torch.randn((n, 256, h, w), device=dev, generator=gen) for h, w in shapes]
        tfpn = [torch.randn((n, 256, h, w), device=dev, generator=gen) for h, w in shapes]
        return labels, targets, torch.tensor([float(max(n_fg, 1))], device=dev), fpn, tfpn

    def params(cfg, seed):
        from ssad_amd.head_pipeline import head_param_specs
        rng = np.random.default_rng(seed)
        return {name: (np.zeros(shape, np.float32) if is_bias else (rng.standard_normal(shape) * 0.01).astype(np.float32))
                for name, shape, is_bias, _ in head_param_specs(cfg)}

    def build_heads(kw, n, distill):
        kw = dict(kw)
        accumulate = kw.pop("shared_accumulate", None)
        cfg = HeadConfig(num_gpus=1, **kw)
        return DistillHeads(cfg, N=n, shapes=shapes, device=dev, student_init=params(cfg, 1),
                            teacher_init=params(cfg, 2) if distill else None, lr=1e-4, distill=distill,
                            shared_accumulate=accumulate)

    def take_turns(steppers):
        """steppers: {name: callable running one step} -> {name: [ms/step per block]}"""
        for f in steppers.values():
            for _ in range(args.warmup):
                f()
        torch.cuda.synchronize()
        blocks = {k: [] for k in steppers}
        for _ in range(args.rounds):
            for k, f in steppers.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    f()
                e1.record()
                e1.synchronize()
                blocks[k].append(e0.elapsed_time(e1) / args.steps)
        return blocks

    def stats(b):
        b = sorted(b)
        return dict(ms_per_step=round(float(np.median(b)), 3), min=round(b[0], 3), max=round(b[-1], 3))

    res = {"metric": "head_options_ms_per_step", "steps_per_block": args.steps, "rounds": args.rounds, "groups": {}}
    lines = ["# RetinaNet head options: shared tower and class-specific box regression", "",
             "`python tools/head_options_bench.py` on one MI355X, fp32, one GPU, synthetic inputs, 81 classes, 9 anchors, "
             "the five 600 px level shapes (80 x 112 ... 5 x 7).  The variants of a group live in one process and take "
             "turns: %d rounds of %d steps each, HIP events around every block, %d warm-up steps per variant; median "
             "(min ... max) over a variant's blocks.  \"default\" and \"default again\" are two objects of the same "
             "separate-tower, class-agnostic heads: the difference between their medians is the spread this tool shows "
             "for identical work, and a variant whose median differs from \"default\" by no more than that is marked "
             "*no difference*." % (args.rounds, args.steps, args.warmup), ""]

    def table(title, blocks, note=""):
        st = {k: stats(b) for k, b in blocks.items()}
        spread = abs(st["default"]["ms_per_step"] - st["default again"]["ms_per_step"])
        lines.extend(["## " + title, "", note, "", "| heads | ms / step | min ... max | against default |", "|---|---|---|---|"])
        for k, e in st.items():
            d = e["ms_per_step"] - st["default"]["ms_per_step"]
            verdict = "" if k == "default" else ("no difference (%+.2f ms, spread %.2f ms)" % (d, spread) if abs(d) <= spread
                                                   else "%+.2f ms (%+.1f %%)" % (d, 100.0 * d / st["default"]["ms_per_step"]))
            lines.append("| %s | %.2f | %.2f ... %.2f | %s |" % (k, e["ms_per_step"], e["min"], e["max"], verdict))
        if "shared tower, two-pass" in st:
            d = st["shared tower"]["ms_per_step"] - st["shared tower, two-pass"]["ms_per_step"]
            st["accumulate_minus_two_pass_ms"] = round(d, 3)
            lines.extend(["", "Accumulate epilogue (\"shared tower\", the default) against the two-pass form: " +
                          ("no difference (%+.3f ms, spread %.3f ms)." % (d, spread) if abs(d) <= spread
                           else "%+.3f ms (spread %.3f ms)." % (d, spread))])
        lines.append("")
        st["spread_ms"] = round(spread, 3)
        return st

    classes = {}
    for gname, n, distill in (("subnet step, config 2 (student only, batch 2)", 2, False),
                              ("subnet step, config 3 (distillation, batch 16)", 16, True)):
        labels, targets, fg_num, fpn, tfpn = inputs(n)
        heads = {k: build_heads(kw, n, distill) for k, kw in VARIANTS}
        steppers = {k: (lambda h=h: h.step(fpn, tfpn if distill else None, labels,
                                           bbox_targets=targets[h.cfg.class_specific_bbox], fg_num=fg_num))
                    for k, h in heads.items()}
        res["groups"][gname] = table(gname, take_turns(steppers),
                                     "DistillHeads.step on fixed FPN tensors: filter packs, forward, losses, backward, SGD.")
        for k, h in heads.items():
            if k == "default again":
                continue
            t = PR.Timing()
            h.timing = t
            for _ in range(args.profile_steps):
                steppers[k]()
            torch.cuda.synchronize()
            classes[gname, k] = t.collect()
            h.timing = None
            assert bool(torch.isfinite(h.focal_losses).all()) and bool(torch.isfinite(h.params.flat).all()), k
            name = "retnet_bbox_pred_fpn3"
            res["groups"][gname].setdefault("bbox_pred_engines", {})[k] = dict(
                fwd=h.fwd_engine["student", name].name, dgrad=h.dgrad_engine[name].name)
        del heads, steppers
        torch.cuda.empty_cache()

    if not args.skip_full:
        n = 16
        labels, targets, fg_num, _, _ = inputs(n)
        images = torch.randn((n, 3) + IMAGE_HW, device=dev, generator=gen)
        models = {}
        for k, kw in VARIANTS[:4]:
            models[k] = NativeDistillModel(build_heads(kw, n, True), "r50", "r101", N=n, image_hw=IMAGE_HW, device=dev)
        steppers = {k: (lambda m=m: m.step(images, labels, targets[False], fg_num)) for k, m in models.items()}
        res["groups"]["whole step, config 3"] = table(
            "whole step, config 3 (ResNet-50 student, ResNet-101 teacher, batch 16, 640 x 896)", take_turns(steppers),
            "NativeDistillModel.step: both backbones and the subnets.")
        for k, m in models.items():
            assert bool(torch.isfinite(m.heads.losses).all()) and bool(torch.isfinite(m.student.params_flat).all()), k

    lines += ["## Per kernel class of the subnet step", "",
              "From %d instrumented steps per variant after the timed blocks (`program.Timing`: events around every "
              "launch, so launches that overlap in the timed step -- the filter gradients on their auxiliary stream -- "
              "run one after the other here and the columns do not add up to the step times above).  ms per step; "
              "classes below 0.02 ms in every column are left out." % args.profile_steps, ""]
    res["classes_ms_per_step"] = {}
    for gname in [g for g in res["groups"] if g.startswith("subnet")]:
        cols = [k for k, _ in VARIANTS if k != "default again"]
        lines += ["### " + gname, "", "| class | kernel family | " + " | ".join(cols) + " |", "|---|---|" + "---|" * len(cols)]
        keys = sorted(set(k for c in cols for k in classes[gname, c]))
        out = res["classes_ms_per_step"][gname] = {}
        for k in keys:
            row = [classes[gname, c].get(k, dict(ms=0.0))["ms"] / args.profile_steps for c in cols]
            if max(row) < 0.02:
                continue
            out[k] = [round(v, 3) for v in row]
            lines.append("| %d | %s | %s |" % (k, PR.KLASS.get(k, dict(name="class %d" % k))["name"],
                                             " | ".join("%.2f" % v for v in row)))
        tot = [sum(c["ms"] for c in classes[gname, col].values()) / args.profile_steps for col in cols]
        lines.append("| | sum of all classes | %s |" % " | ".join("%.2f" % v for v in tot))
        eng = res["groups"][gname]["bbox_pred_engines"]
        lines += ["", "bbox_pred's engines (forward / data gradient): " +
                  "; ".join("%s: %s / %s" % (k, e["fwd"], e["dgrad"]) for k, e in eng.items()) + ".", ""]
    lines += ["\"shared tower\", the default, forms the shared activation's gradient in `bbox_pred`'s data-gradient epilogue "
              "(`SSAD_CONV_ACCUM_AUX`, F(2x4) engine: `y = aux > 0 ? y + acc : 0` behind `cls_pred`'s unmasked gradient); "
              "\"shared tower, two-pass\" (`shared_accumulate=False`) runs both data gradients unmasked into buffers of "
              "their own, then one `SUM_N` and one `RELU_GRAD` record per level (class 39).  The epilogue is the default "
              "because it was faster than the two-pass form by more than the spread on config 2's and on config 3's "
              "subnet step (DESIGN 3.14 has every run).  The wide class-specific "
              "`bbox_pred` is on the split-operand engine, which has no such epilogue: \"both\" is two-pass.", ""]
    lines += ["These are figures of one run on one machine; the rows of a table are comparable with each other -- same "
              "process, interleaved -- but not with a figure taken in another run, such as bench.py's headline.  No bar "
              "was set for these numbers; nothing was tuned against them."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
