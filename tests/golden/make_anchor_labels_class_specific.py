#!/usr/bin/env python3
"""Fixture for anchor labelling with RETINANET.CLASS_SPECIFIC_BBOX = True, produced BY THE REFERENCE'S OWN PYTHON
(detectron/lib/roi_data/retinanet.py:97-306; the switch acts at :140-151 and :286-293): column 1 of
retnet_roi_fg_bbox_locs_fpn{l} is 4 * (label - 1) + 4 * (NUM_CLASSES - 1) * anchor.  Imported and stubbed exactly
as make_anchor_labels.py does (its install() is reused; that file stays as it is; `make -C oracle pyref` first).

The ground truth holds class 1, class NUM_CLASSES - 1 and classes in between, every one on an object large enough
to own foreground anchors, so a wrong class offset cannot cancel.

Runs ONLY in the build container.  Output: tests/golden/anchor_labels_class_specific_ref.npz (data only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_anchor_labels_class_specific.py
"""
import os
import sys
from collections import defaultdict

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_anchor_labels as mal  # noqa: E402

OUT = os.path.join(HERE, "anchor_labels_class_specific_ref.npz")
CLASSES = ((1, 80, 17, 40, 80, 1), (80, 2, 1, 79, 33, 1, 80, 56))


def main():
    mal.install()
    from core.config import cfg
    import roi_data.retinanet as rn
    cfg.FPN.FPN_ON = True
    cfg.FPN.MULTILEVEL_RPN = True
    cfg.FPN.RPN_MAX_LEVEL, cfg.FPN.RPN_MIN_LEVEL = 7, 3
    cfg.FPN.COARSEST_STRIDE = 128
    cfg.RETINANET.RETINANET_ON = True
    cfg.RETINANET.SCALES_PER_OCTAVE = 3
    cfg.RETINANET.ASPECT_RATIOS = (0.5, 1.0, 2.0)
    cfg.RETINANET.ANCHOR_SCALE = 4
    cfg.RETINANET.POSITIVE_OVERLAP, cfg.RETINANET.NEGATIVE_OVERLAP = 0.5, 0.4
    cfg.RETINANET.CLASS_SPECIFIC_BBOX = True
    cfg.MODEL.NUM_CLASSES = 81
    cfg.TRAIN.MAX_SIZE = 1000

    rng = np.random.default_rng(20261020)
    image_height, image_width = 384, 512
    roidb, scales = [], []
    for classes, (h, w) in zip(CLASSES, ((300, 400), (360, 480))):
        n_gt = len(classes)
        boxes = np.zeros((n_gt, 4), np.float32)
        for g in range(n_gt):
            bw = float(np.exp(rng.uniform(np.log(20.0), np.log(0.7 * w))))
            bh = float(np.clip(bw * np.exp(rng.uniform(-0.7, 0.7)), 14.0, 0.9 * h))
            x1, y1 = rng.uniform(0, w - bw - 1), rng.uniform(0, h - bh - 1)
            boxes[g] = [x1, y1, x1 + bw, y1 + bh]
        roidb.append(dict(height=h, width=w, boxes=boxes, gt_classes=np.array(classes, np.int32),
                          is_crowd=np.zeros(n_gt, np.int32)))
        scales.append(1.0)
    blobs = defaultdict(list)
    assert rn.add_retinanet_blobs(blobs, scales, roidb, image_width, image_height)
    out = {"image_hw": np.array([image_height, image_width], np.int32), "scales": np.array(scales, np.float64),
           "num_classes": np.array(cfg.MODEL.NUM_CLASSES, np.int32)}
    for i, e in enumerate(roidb):
        out["gt_boxes_%d" % i] = e["boxes"]
        out["gt_classes_%d" % i] = e["gt_classes"]
    seen = set()
    for k, v in blobs.items():
        out["blob_" + k] = np.asarray(v)
        if k.startswith("retnet_roi_fg_bbox_locs"):
            seen |= set(((np.asarray(v)[:, 1].astype(int) % 320) // 4 + 1).tolist())
    assert {1, 80} <= seen and len(seen - {1, 80}) >= 1, seen
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, sorted(seen), {k: v.shape for k, v in out.items() if k.startswith("blob_retnet_roi_fg")})


if __name__ == "__main__":
    main()
