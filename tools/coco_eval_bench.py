"""Times DetectionEvaluator.evaluate() at COCO minival scale -- 5000 images, 80 categories, 100 detections and about 7
ground truths per image, synthetic -- split into matching, ordering and accumulation, and beside it the numpy statement
of tests/test_coco_eval_cpu.py on a 100-image slice, scaled to the full set.  Writes profiles/coco_eval.md.

Timing: HIP events around the three stages inside evaluate() (the read-back of the results lies behind the last
event), a warm-up and then the median of --iters evaluations.  Prints one JSON line.

    python tools/coco_eval_bench.py [--iters 10] [--warmup 2] [--out profiles/coco_eval.md]"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

I, K, DETS, SLICE = 5000, 80, 100, 100


def synth(rng):
    """Per image about 7 ground truths in a handful of categories, one jittered detection for most of them and random
    boxes up to 100 detections; scores quantised to 1/1000 so that ties occur."""
    gt, dets = [], []
    for img in range(I):
        cats = rng.choice(K, size=6, replace=False)
        n = int(rng.poisson(7))
        wh = rng.uniform(8, 200, (n, 2))
        xy = rng.uniform(0, 440, (n, 2))
        c = rng.choice(cats, n)
        for j in range(n):
            gt.append((img, c[j], xy[j, 0], xy[j, 1], wh[j, 0], wh[j, 1], rng.random() < 0.03))
        m = min(n, DETS)
        jit = rng.normal(0, 0.08, (m, 4)) * np.concatenate([wh[:m], wh[:m]], 1)
        near = np.concatenate([xy[:m], xy[:m] + wh[:m] - 1], 1) + jit
        fwh, fxy = rng.uniform(8, 200, (DETS - m, 2)), rng.uniform(0, 440, (DETS - m, 2))
        box = np.concatenate([near, np.concatenate([fxy, fxy + fwh - 1], 1)]).astype(np.float32)
        box[:, 2:] = np.maximum(box[:, 2:], box[:, :2] + 1)
        dc = np.concatenate([c[:m], rng.choice(cats, DETS - m)]).astype(np.int32)
        sc = (rng.integers(1, 1001, DETS) / 1000.0).astype(np.float32)
        dets.append((box, sc, dc))
    g = np.array(gt, np.float64)
    area = g[:, 4] * g[:, 5] * rng.uniform(0.4, 1.0, len(g))
    return g, area, dets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_eval.md"))
    args = ap.parse_args()
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd.datasets import DetectionEvaluator
    if not torch.cuda.is_available():
        raise SystemExit("coco_eval_bench needs a GPU: nothing is estimated without one")
    g, area, dets = synth(np.random.default_rng(0))
    ev = DetectionEvaluator(I, K, np.ascontiguousarray(g[:, 2:6]), area, g[:, 6].astype(np.uint8),
                            g[:, 0].astype(np.int32), g[:, 1].astype(np.int32), max_dets_per_image=DETS)
    for img, (box, sc, dc) in enumerate(dets):
        ev.add_detections(img, box, sc, dc)
    for _ in range(args.warmup):
        res = ev.evaluate()
    runs = [ev.evaluate(timing=True)["timing_ms"] for _ in range(args.iters)]
    stages = ("matching", "ordering", "accumulation")
    med = {s: float(np.median([r[s] for r in runs])) for s in stages}
    lo = {s: float(np.min([r[s] for r in runs])) for s in stages}
    hi = {s: float(np.max([r[s] for r in runs])) for s in stages}
    t0 = time.perf_counter()
    ev.evaluate()
    wall = (time.perf_counter() - t0) * 1e3

    # the numpy statement on the first SLICE images
    spec = importlib.util.spec_from_file_location("test_coco_eval_cpu", os.path.join(ROOT, "tests",
                                                                                     "test_coco_eval_cpu.py"))
    st = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(st)
    sel = g[:, 0] < SLICE
    z = {"det_boxes": np.concatenate([d[0] for d in dets[:SLICE]]),
         "det_scores": np.concatenate([d[1] for d in dets[:SLICE]]),
         "det_category": np.concatenate([d[2] for d in dets[:SLICE]]),
         "det_image": np.repeat(np.arange(SLICE), DETS)}
    t0 = time.perf_counter()
    m = st.spec_match(SLICE, K, g[sel, 2:6], area[sel], g[sel, 6].astype(np.uint8), g[sel, 0].astype(np.int32),
                      g[sel, 1].astype(np.int32), z["det_boxes"], z["det_scores"], z["det_category"], z["det_image"],
                      ev.iou_thrs, ev.area_rng, ev.max_dets[-1], False)
    t1 = time.perf_counter()
    st.spec_accumulate(K, m, z["det_scores"], ev.rec_thrs, ev.max_dets)
    t2 = time.perf_counter()
    spec_ms = {"matching": (t1 - t0) * 1e3, "accumulation (with its ordering)": (t2 - t1) * 1e3}
    # the slice's cells are the first cells of the whole set: their matches must be the statement's
    got = ev.evaluate(return_matches=True)["matches"]
    nc, nd = len(m["cell"]), int(m["offsets"][-1])
    same = bool(np.array_equal(got["cell"][:nc], m["cell"]) and np.array_equal(got["offsets"][:nc + 1], m["offsets"])
                and np.array_equal(got["dt_match"][:, :, :nd], m["dt_match"])
                and np.array_equal(got["dt_ignore"][:, :, :nd], m["dt_ignore"])
                and np.array_equal(got["npig"][:nc], m["npig"]))
    if not same:
        raise SystemExit("the device's matches on the first %d images differ from the numpy statement" % SLICE)
    scale = I / SLICE

    lines = [
        "# `DetectionEvaluator.evaluate()` at minival scale",
        "",
        "`python tools/coco_eval_bench.py` on one MI355X: %d images, %d categories, %d detections and about 7 ground"
        % (I, K, DETS),
        "truths per image (%d in all), synthetic; 10 IoU thresholds x 4 area ranges, maxDets 1 / 10 / 100, 101 recall"
        % len(g),
        "thresholds.  HIP events around the three stages inside `evaluate()`, %d warm-up evaluations, median of %d."
        % (args.warmup, args.iters),
        "",
        "| stage | what runs | median ms | min ... max |",
        "|---|---|---|---|",
        "| matching | `coco_match_kernel`, one workgroup per (image, category) cell | %.3f | %.3f ... %.3f |"
        % (med["matching"], lo["matching"], hi["matching"]),
        "| ordering | three stable `torch.sort`s and a `searchsorted` over %d slots | %.3f | %.3f ... %.3f |"
        % (I * DETS, med["ordering"], lo["ordering"], hi["ordering"]),
        "| accumulation | `coco_cells_kernel`, `coco_accumulate_kernel` | %.3f | %.3f ... %.3f |"
        % (med["accumulation"], lo["accumulation"], hi["accumulation"]),
        "| sum | | %.3f | |" % sum(med.values()),
        "",
        "One whole `evaluate()` call including the read-back of precision / recall / scores and the host-side",
        "`stats`: %.1f ms wall clock.  mAP of the synthetic set: %.4f." % (wall, res["stats"][0]),
        "",
        "The numpy statement of `tests/test_coco_eval_cpu.py` (plain Python loops, one lane after the other) on the",
        "first %d images, and that time multiplied by %d:" % (SLICE, int(scale)),
        "",
        "| stage | ms on %d images | scaled to %d |" % (SLICE, I),
        "|---|---|---|",
    ]
    for name, ms in spec_ms.items():
        lines.append("| %s | %.0f | %.0f |" % (name, ms, ms * scale))
    lines += ["", "The device's matches, ignore flags and counts for the %d cells of those images equal the statement's." % nc]
    lines += ["", "The statement is a specification, not an optimised evaluator: the comparison says what the lane-by-lane",
              "walk costs when it is not spread over lanes, nothing about pycocotools.  No bar was set for these numbers;",
              "nothing here was tuned against them."]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps({"iters": args.iters, "median_ms": med, "evaluate_wall_ms": wall,
                      "numpy_statement_ms_on_slice": spec_ms, "slice": SLICE, "images": I}))


if __name__ == "__main__":
    main()
