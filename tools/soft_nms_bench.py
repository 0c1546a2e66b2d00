"""Times RetinanetDetector per image with greedy NMS, linear and gaussian Soft-NMS, and gaussian Soft-NMS + box voting
at the reference's 5 levels x 1000 candidates (an 640 x 896 blob, 80 classes), in one process, and writes
profiles/soft_nms.md.

Two inputs: random scores over all 80 classes (about 62 candidates a class), and the worst case for the serial walk,
every candidate in ONE class (4315 of them: the three coarse levels hold fewer than 1000 anchors of one class).
Timing: HIP events around one detector call alone (all its launches, no host read-back inside the interval), the
variants alternating, a warm-up and then the median of --iters calls each.  Prints one JSON line.

    python tools/soft_nms_bench.py [--iters 50] [--warmup 3] [--out profiles/soft_nms.md]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(80, 112), (40, 56), (20, 28), (10, 14), (5, 7)]
VARIANTS = [
    ("greedy NMS", None, None),
    ("Soft-NMS linear", dict(method="linear"), None),
    ("Soft-NMS gaussian", dict(method="gaussian", sigma=0.5), None),
    ("Soft-NMS gaussian + box voting (ID)", dict(method="gaussian", sigma=0.5), dict(vote_th=0.8)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_nms.md"))
    args = ap.parse_args()
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd.roi_data.retinanet import RetinanetDetector
    if not torch.cuda.is_available():
        raise SystemExit("soft_nms_bench needs a GPU: nothing is estimated without one")
    rng = np.random.default_rng(0)
    inputs = {}
    for name in ("80 classes", "one class"):
        probs, deltas = [], []
        for h, w in SHAPES:
            p = rng.random((1, 9, 80, h, w), dtype=np.float32)
            if name == "one class":
                p[:, :, 1:] = 0.0
            probs.append(torch.from_numpy(p.reshape(1, 720, h, w)).cuda())
            deltas.append(torch.from_numpy((rng.standard_normal((1, 36, h, w)) * 0.4).astype(np.float32)).cuda())
        inputs[name] = (probs, deltas)
    dets = [(label, RetinanetDetector(SHAPES, soft_nms=soft, bbox_vote=vote)) for label, soft, vote in VARIANTS]

    def timed(det, probs, deltas):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        det(probs, deltas, 640, 896, 1.0)
        b.record()
        return a, b

    # RetinanetDetector.__call__ reads the row count back after its launches: that wait lies behind event b
    results = {}
    for name, (probs, deltas) in inputs.items():
        for _ in range(args.warmup):
            for _, det in dets:
                det(probs, deltas, 640, 896, 1.0)
        torch.cuda.synchronize()
        events = {label: [] for label, _ in dets}
        for _ in range(args.iters):
            for label, det in dets:
                events[label].append(timed(det, probs, deltas))
        torch.cuda.synchronize()
        for label, ev in events.items():
            t = [a.elapsed_time(b) for a, b in ev]
            results["%s | %s" % (name, label)] = [float(np.median(t)), float(np.min(t)), float(np.max(t))]
    lines = [
        "# Soft-NMS and box voting in `RetinanetDetector`: time per image",
        "",
        "`python tools/soft_nms_bench.py` on one MI355X: 5 levels of a 640 x 896 blob, `pre_nms_topn` 1000, 80 classes,",
        "uniform random scores and N(0, 0.4) box deltas.  HIP events around one detector call (key build, top-k select,",
        "decode, class sort, NMS, final sort, emit), the four variants alternating in one process, %d warm-up rounds,"
        % args.warmup,
        "median of %d.  \"one class\" puts every candidate (4315) into a single class: the walk of `soft_nms_kernel` is"
        % args.iters,
        "serial in the number of picks, so this is its worst case -- one workgroup, one pick after the other.",
        "",
        "| input | variant | median ms | min ... max |",
        "|---|---|---|---|",
    ]
    for key, (med, lo, hi) in results.items():
        name, label = key.split(" | ")
        lines.append("| %s | %s | %.3f | %.3f ... %.3f |" % (name, label, med, lo, hi))
    lines += ["", "No bar was set for these numbers; nothing here was tuned against them."]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"iters": args.iters, "median_min_max_ms": results}))


if __name__ == "__main__":
    main()
