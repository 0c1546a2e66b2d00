"""Times config 2's subnet step (head_pipeline.DistillHeads, distill=False: towers, prediction layers, focal loss,
SelectSmoothL1Loss, backward, SGD -- no backbone) with sigmoid heads and with softmax heads (HeadConfig.softmax: a
729-wide cls_pred and the fused SoftmaxFocalLoss record) in ONE process: both pipelines are built once, warmed up,
and then timed in alternating blocks of --steps steps, --rounds times, at every --batch.  Time: HIP events around a
block of steps on the current stream, divided by the number of steps.  Prints one JSON line.

--root DIR imports the package from another checkout (built there), so that the sigmoid step of another commit can
be measured with the same inputs and the same clock in the same job; --heads restricts what is built (a checkout
without the softmax step can only run `sigmoid`).

    python tools/softmax_step_bench.py [--batch 2 16] [--steps 20] [--warmup 5] [--rounds 3] [--heads both]"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[2, 16])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--heads", default="both", choices=["both", "sigmoid", "softmax"])
    ap.add_argument("--root", default=HERE)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd import synth
    from ssad_amd.head_pipeline import DistillHeads
    from ssad_amd.modeling.retinanet_heads import HeadConfig
    if not torch.cuda.is_available():
        raise SystemExit("softmax_step_bench needs a GPU: nothing is estimated without one")
    kinds = ["sigmoid", "softmax"] if args.heads == "both" else [args.heads]
    shapes = synth.LEVEL_SHAPES_600
    out = dict(root=os.path.abspath(args.root), device=torch.cuda.get_device_name(0), steps=args.steps,
               rounds=args.rounds, batches={})
    for N in args.batch:
        rng = np.random.default_rng(100 + N)
        to = lambda a: torch.from_numpy(a).cuda()                    # noqa: E731
        fpn = [to(a) for a in synth.fpn_features(rng, N, shapes)]
        labs = [synth.distill_inputs(rng, N, 9, 80, h, w)[2] for h, w in shapes]
        tg = [synth.bbox_targets(rng, l) for l in labs]
        fg = to(np.array([max(1, sum(t[0].shape[0] for t in tg))], np.float32))
        labels, targets = [to(a) for a in labs], [(to(y), to(l)) for y, l in tg]
        heads = {}
        for kind in kinds:
            cfg = HeadConfig(num_gpus=1, softmax=True) if kind == "softmax" else HeadConfig(num_gpus=1)
            classes = cfg.num_classes if kind == "softmax" else cfg.num_classes - 1
            heads[kind] = DistillHeads(cfg, N=N, shapes=shapes, device="cuda", distill=False, lr=1e-3,
                                       student_init=synth.head_params(np.random.default_rng(7), C=classes))

        def block(h, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                h.step(fpn, None, labels, bbox_targets=targets, fg_num=fg)
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / n

        for kind in kinds:
            block(heads[kind], args.warmup)
        rounds = []
        for _ in range(args.rounds):
            rounds.append({kind: block(heads[kind], args.steps) for kind in kinds})       # alternating
        res = dict(rounds_ms_per_step=rounds)
        for kind in kinds:
            t = [r[kind] for r in rounds]
            res[kind] = dict(median_ms=float(np.median(t)), min_ms=float(min(t)), max_ms=float(max(t)),
                             focal_losses=[float(v) for v in heads[kind].focal_losses.cpu()])
            assert np.isfinite(res[kind]["focal_losses"]).all(), kind
        if len(kinds) == 2:
            res["softmax_over_sigmoid"] = res["softmax"]["median_ms"] / res["sigmoid"]["median_ms"]
        out["batches"][str(N)] = res
        del heads
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
