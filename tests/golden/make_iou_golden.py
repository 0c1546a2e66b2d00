#!/usr/bin/env python3
"""Pin for the oracle's IoU (oracle/anchors.py:bbox_overlaps), produced BY THE REFERENCE'S OWN
IoU routine: detectron/lib/utils/cython_bbox.pyx compiled from where it lies
(oracle/_pyref/cython_bbox.so, `make -C oracle pyref`; build container only, never shipped).

The routine's output over every anchor of a 640 x 896 image is 29 MB per case, so the fixture
holds the inputs (the ground-truth boxes) and the SHA-256 of the output's bytes (float32,
C order): tests/test_anchor_labels.py recomputes the oracle's output and compares digests,
i.e. bit for bit.

Runs ONLY in the build container.  Output: tests/golden/iou_ref.npz (data only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_iou_golden.py
"""
import hashlib
import importlib.util
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "iou_ref.npz")


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import anchors as OA
    from test_anchor_labels import rand_gts
    so = os.path.join(ROOT, "oracle", "_pyref", "cython_bbox.so")
    spec = importlib.util.spec_from_file_location("cython_bbox", so)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    anchors, _ = OA.all_anchors()
    rng = np.random.default_rng(5)
    out = {}
    for case, integer in (("random", False), ("integer", True)):
        g, _ = rand_gts(rng, 37, integer=integer)
        r = np.ascontiguousarray(ref.bbox_overlaps(anchors, g))
        assert r.dtype == np.float32
        out["gts_" + case] = g
        out["shape_" + case] = np.array(r.shape, np.int64)
        out["sha256_" + case] = np.array(hashlib.sha256(r.tobytes()).hexdigest())
    np.savez(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
