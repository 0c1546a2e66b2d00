#!/usr/bin/env python3
"""Golden vectors for the COCO box evaluation from the reference's own evaluator.

Like make_soft_nms_golden.py: detectron/lib/datasets/vid_eval.py (`VIDeval`) is read where it lies under
/root/reference at generation time (nothing of it is stored in the repository), a fixed list of substitutions --
`SUBSTITUTIONS`, each asserted by its count -- makes it run under Python 3 / numpy 2, and the result is EXECUTED.
Only arrays are stored.  `VIDeval` is driven the way vid_dataset_evaluator.py:192-197 drives it for boxes
(evaluate, accumulate, summarize) through a minimal stand-in for the COCO API object (getImgIds, getCatIds, getAnnIds,
loadAnns; annotation ids are 1-based because `dtm == 0` means unmatched).

Two modes of one data set:
  relax   the file as it stands: vid_eval.py:286-288 relaxes the threshold for small boxes,
          tiou = min(iou, w*h / ((w+10)*(h+10)));
  strict  that one line replaced by `tiou=iou`.  That this variant IS the COCO toolbox's `COCOeval` is stated from
          knowledge of that code and NOT CHECKED here: pycocotools is not on this machine.  UNPINNED.

Box IoU: the file calls `maskUtils.iou`, the COCO toolbox's C module behind datasets/mask.py, which is not on this
machine either.  The object injected in its place computes, in float64 on xywh boxes with no +1,
  w = min(dx+dw, gx+gw) - max(dx, gx), h likewise, IoU = 0 unless w > 0 and h > 0, i = w*h,
  union = dw*dh + gw*gh - i, or dw*dh alone for a crowd ground truth
-- the toolbox's bbIou restated from knowledge of it.  UNPINNED, as cv2.resize is for the image blobs.

Detections are float32 xyxy rows; they become COCO results by json_dataset_evaluator.py:179's rule (xyxy_to_xywh:
w = x2 - x1 + 1 in float32) and loadRes's `area = w*h` (restated: that file is not in the reference tree).

Stored (tests/golden/coco_eval_ref.npz):
  num_images, num_categories, iou_thrs, rec_thrs, max_dets, area_rng          the reference's Params
  gt_boxes [G][4] f64 xywh, gt_area, gt_iscrowd, gt_image, gt_category        in a shuffled order
  det_boxes [N][4] f32 xyxy, det_scores f32, det_category, det_image          image-major, the order within an image
                                                                              is the order of the results
  m_cell [C]       image * K + category of every evaluated cell, ascending
  m_off [C+1]      offsets of the cells' detections (score order, cut at max_dets[-1]) in the arrays below
  m_npig [C][A]    non-ignored ground truths
  <mode>_dtm [A][T][sum D] int32   dtMatches with the ground-truth id mapped to index + 1 within the cell's order
  <mode>_dtig [A][T][sum D] bool   dtIgnore
  <mode>_precision / _recall / _scores / _stats                               accumulate's and summarize's results

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_coco_eval_golden.py     -> tests/golden/coco_eval_ref.npz
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/detectron/lib/datasets/vid_eval.py"
OUT = os.path.join(HERE, "coco_eval_ref.npz")
I, K = 12, 6
F = np.float32

RELAX_LINE = "tiou=min(iou,1.0*w*h/((w+10)*(h+10)))"
SORT_LINE = "inds = np.argsort(-dtScores, kind='mergesort')"
SUBSTITUTIONS = [                                   # (old, new, places)
    ("from . import mask as maskUtils\n", "", 1),
    ("dtype=np.float)", "dtype=float)", 2),
    ("np.round((0.95 - .5) / .05) + 1", "int(np.round((0.95 - .5) / .05)) + 1", 2),
    ("np.round((1.00 - .0) / .01) + 1", "int(np.round((1.00 - .0) / .01)) + 1", 2),
    # semantics unchanged: counts the walks that leave through :284-285's break
    ("                            break\n", "                            PROBE['break'] += 1; break\n", 1),
]


class BoxIoU(object):
    """Stands where `maskUtils` stood; keeps every matrix it returned for the margin check."""

    def __init__(self):
        self.seen = []

    def iou(self, d, g, iscrowd):
        out = np.zeros((len(d), len(g)), np.float64)
        for i, (dx, dy, dw, dh) in enumerate(d):
            for j, (gx, gy, gw, gh) in enumerate(g):
                w = min(dx + dw, gx + gw) - max(dx, gx)
                h = min(dy + dh, gy + gh) - max(dy, gy)
                if w > 0 and h > 0:
                    inter = w * h
                    da = dw * dh
                    out[i, j] = inter / (da if iscrowd[j] else da + gw * gh - inter)
        if len(d) and len(g):
            self.seen.append((out, np.array([[b[2], b[3]] for b in g], np.float64)))
        return out


def reference_eval(relax, reverse_ties=False):
    text = open(REF).read()
    subs = list(SUBSTITUTIONS)
    if not relax:
        subs.append((RELAX_LINE, "tiou=iou", 1))
    if reverse_ties:         # for the generator's own assertion only: equal scores in the opposite order
        subs.append((SORT_LINE, "inds = (len(dtScores) - 1 - np.argsort(-dtScores[::-1], kind='mergesort'))", 1))
    for old, new, places in subs:
        assert text.count(old) == places, (old, text.count(old))
        text = text.replace(old, new)
    boxiou, probe = BoxIoU(), {"break": 0}
    ns = {"maskUtils": boxiou, "PROBE": probe, "__name__": "vid_eval"}
    exec(compile(text, "<vid_eval.py>", "exec"), ns)
    return ns["VIDeval"], boxiou, probe


class Api(object):
    """The four calls VIDeval makes on a COCO API object."""

    def __init__(self, anns):
        self.anns = anns

    def getImgIds(self):
        return list(range(I))

    def getCatIds(self):
        return list(range(K))

    def getAnnIds(self, imgIds=(), catIds=()):
        im, ct = set(imgIds), set(catIds)
        return [a["id"] for a in self.anns if a["image_id"] in im and a["category_id"] in ct]

    def loadAnns(self, ids):
        return [self.anns[i - 1] for i in ids]


def data():
    rng = np.random.default_rng(20261019)
    gts, dets = [], [[] for _ in range(I)]           # (img, cat, x, y, w, h, crowd); per image (cat, x1, y1, x2, y2)

    def gt_box(lo=4, hi=150):
        w, h = rng.uniform(lo, hi, 2)
        return [rng.uniform(0, 640 - w), rng.uniform(0, 480 - h), w, h]

    def near(b, jit):
        x, y, w, h = b
        x1, x2 = x + rng.normal(0, jit * w), x + w - 1 + rng.normal(0, jit * w)
        y1, y2 = y + rng.normal(0, jit * h), y + h - 1 + rng.normal(0, jit * h)
        return [x1, y1, max(x2, x1 + 1), max(y2, y1 + 1)]

    def far():
        x, y, w, h = gt_box()
        return [x, y, x + w - 1, y + h - 1]

    def inside(b):
        x, y, w, h = b
        ww, hh = rng.uniform(0.2, 0.6) * w, rng.uniform(0.2, 0.6) * h
        x1, y1 = x + rng.uniform(0, w - ww), y + rng.uniform(0, h - hh)
        return [x1, y1, x1 + ww, y1 + hh]

    # 70 ground truths in one cell: more than a wavefront
    for n in range(70):
        b = gt_box(4, 90)
        gts.append([0, 0] + b + [0])
        if n % 4 != 3:
            dets[0].append([0] + near(b, rng.choice([0.02, 0.05, 0.1])))
    dets[0] += [[0] + far() for _ in range(9)]
    # 130 detections in one cell: more than the largest maxDets
    for n in range(5):
        b = gt_box(30, 150)
        gts.append([1, 1] + b + [0])
        dets[1] += [[1] + near(b, rng.choice([0.02, 0.06, 0.12])) for _ in range(14)]
    dets[1] += [[1] + far() for _ in range(60)]
    # images 2..10, categories 0..3: a few of each, doubles and false positives; image 11 holds nothing
    for img in range(2, 11):
        for cat in range(4):
            if (img, cat) in ((2, 2), (3, 3)):
                continue
            for _ in range(int(rng.integers(0, 5))):
                b = gt_box()
                gts.append([img, cat] + b + [0])
                for _ in range(int(rng.choice([0, 1, 1, 1, 2]))):
                    dets[img].append([cat] + near(b, rng.choice([0.01, 0.03, 0.06, 0.1, 0.15])))
            dets[img] += [[cat] + far() for _ in range(int(rng.integers(0, 4)))]
    gts += [[2, 2] + gt_box() + [0] for _ in range(3)]                 # ground truth only
    dets[3] += [[3] + far() for _ in range(4)]                         # detections only
    # crowd regions, each matched by several detections, beside regular ones
    for img, cat in ((4, 0), (5, 1), (6, 2), (6, 0)):
        b = gt_box(110, 150)
        gts.append([img, cat] + b + [1])
        dets[img] += [[cat] + inside(b) for _ in range(4)]
    # a category whose ground truths are all crowd; category 5 has nothing at all
    for img in (2, 7):
        b = gt_box(100, 150)
        gts.append([img, 4] + b + [1])
        dets[img] += [[4] + inside(b) for _ in range(3)] + [[4] + far()]
    order = rng.permutation(len(gts))
    g = np.array(gts, np.float64)[order]
    area = g[:, 4] * g[:, 5] * rng.uniform(0.4, 1.0, len(g))
    blobs = {"gt_boxes": np.ascontiguousarray(g[:, 2:6]), "gt_area": area, "gt_iscrowd": g[:, 6].astype(np.uint8),
             "gt_image": g[:, 0].astype(np.int32), "gt_category": g[:, 1].astype(np.int32)}
    rows, image = [], []
    for img in range(I):
        for k in rng.permutation(len(dets[img])):
            rows.append(dets[img][k])
            image.append(img)
    d = np.array(rows, np.float64)
    blobs["det_boxes"] = np.ascontiguousarray(d[:, 1:5]).astype(F)
    blobs["det_scores"] = (rng.integers(1, 51, len(d)).astype(F) / F(50)).astype(F)        # quantised: ties are real
    blobs["det_category"] = d[:, 0].astype(np.int32)
    blobs["det_image"] = np.array(image, np.int32)
    return blobs


def annotations(b):
    gt = [dict(id=n + 1, image_id=int(b["gt_image"][n]), category_id=int(b["gt_category"][n]),
               bbox=[float(v) for v in b["gt_boxes"][n]], area=float(b["gt_area"][n]), iscrowd=int(b["gt_iscrowd"][n]))
          for n in range(len(b["gt_area"]))]
    box = b["det_boxes"]
    w = box[:, 2] - box[:, 0] + F(1)                   # float32, then widened (json_dataset_evaluator.py:179)
    h = box[:, 3] - box[:, 1] + F(1)
    assert w.dtype == F
    dt = [dict(id=n + 1, image_id=int(b["det_image"][n]), category_id=int(b["det_category"][n]),
               bbox=[float(box[n, 0]), float(box[n, 1]), float(w[n]), float(h[n])], area=float(w[n]) * float(h[n]),
               score=float(b["det_scores"][n]), iscrowd=0) for n in range(len(w))]
    return gt, dt


def run(b, relax, reverse_ties=False):
    cls, boxiou, probe = reference_eval(relax, reverse_ties)
    gt, dt = annotations(b)
    E = cls(Api(gt), Api(dt), "bbox")
    with contextlib.redirect_stdout(io.StringIO()):
        E.evaluate()
        E.accumulate()
        E.summarize()
    return E, boxiou, probe


def generate():
    b = data()
    G, N = len(b["gt_area"]), len(b["det_scores"])
    cells_gt = {}
    for n in range(G):
        cells_gt.setdefault((int(b["gt_image"][n]), int(b["gt_category"][n])), []).append(n + 1)
    cells_dt = {}
    for n in range(N):
        cells_dt.setdefault((int(b["det_image"][n]), int(b["det_category"][n])), []).append(n + 1)
    blobs = dict(b)
    blobs["num_images"], blobs["num_categories"] = np.int32(I), np.int32(K)
    results = {}
    for mode, relax in (("strict", False), ("relax", True)):
        E, boxiou, probe = run(b, relax)
        p = E.params
        T, A = len(p.iouThrs), len(p.areaRng)
        # no decision of any walk hinges on the last bits of an IoU
        margin = np.inf
        for ious, wh in boxiou.seen:
            thr = np.minimum(p.iouThrs, 1 - 1e-10)
            margin = min(margin, np.abs(ious[:, :, None] - thr).min())
            if relax:
                margin = min(margin, np.abs(ious - wh[:, 0] * wh[:, 1] / ((wh[:, 0] + 10) * (wh[:, 1] + 10))).min())
        assert margin >= 1e-9, margin
        assert probe["break"] > 0
        cell_ids, off, npig, dtm, dtig = [], [0], [], [], []
        A0, I0 = A, I
        for img in range(I):
            for cat in range(K):
                es = [E.evalImgs[cat * A0 * I0 + a * I0 + img] for a in range(A)]
                if es[0] is None:
                    assert (img, cat) not in cells_gt and (img, cat) not in cells_dt
                    continue
                local = {gid: n + 1 for n, gid in enumerate(cells_gt.get((img, cat), []))}
                local[0] = 0
                cell_ids.append(img * K + cat)
                D = len(es[0]["dtIds"])
                off.append(off[-1] + D)
                npig.append([int(np.count_nonzero(np.asarray(e["gtIgnore"]) == 0)) for e in es])
                dtm.append(np.array([[[local[int(v)] for v in row] for row in e["dtMatches"]] for e in es],
                                    np.int32).reshape(A, T, D))
                dtig.append(np.array([e["dtIgnore"] for e in es], bool).reshape(A, T, D))
        results[mode] = E
        if mode == "strict":
            blobs["m_cell"], blobs["m_off"] = np.array(cell_ids, np.int32), np.array(off, np.int32)
            blobs["m_npig"] = np.array(npig, np.int32)
            blobs["iou_thrs"], blobs["rec_thrs"] = np.asarray(p.iouThrs, np.float64), np.asarray(p.recThrs, np.float64)
            blobs["max_dets"] = np.asarray(p.maxDets, np.int32)
            blobs["area_rng"] = np.asarray(p.areaRng, np.float64)
        else:
            assert np.array_equal(blobs["m_cell"], cell_ids) and np.array_equal(blobs["m_off"], off)
        blobs[mode + "_dtm"] = np.concatenate(dtm, axis=2)
        blobs[mode + "_dtig"] = np.concatenate(dtig, axis=2)
        assert np.any(blobs[mode + "_dtig"] & (blobs[mode + "_dtm"] == 0)), "no unmatched detection ignored by area"
        for name in ("precision", "recall", "scores"):
            blobs["%s_%s" % (mode, name)] = np.asarray(E.eval[name], np.float64)
        blobs[mode + "_stats"] = np.asarray(E.stats, np.float64)
        # equal scores in the opposite order give another curve: the fixture tells a stable sort from an unstable one
        assert not np.array_equal(run(b, relax, reverse_ties=True)[0].eval["precision"], E.eval["precision"])
    # what makes the fixture meaningful
    assert not np.array_equal(blobs["strict_precision"], blobs["relax_precision"])
    sizes_gt = {c: len(v) for c, v in cells_gt.items()}
    sizes_dt = {c: len(v) for c, v in cells_dt.items()}
    assert max(sizes_gt.values()) >= 70 and max(sizes_dt.values()) >= 130 > blobs["max_dets"][-1]
    assert set(cells_gt) - set(cells_dt) and set(cells_dt) - set(cells_gt)
    assert not np.any(b["gt_image"] == I - 1) and not np.any(b["det_image"] == I - 1)
    assert np.all(b["gt_iscrowd"][b["gt_category"] == 4] == 1) and not np.any(b["gt_category"] == 5)
    assert np.all(blobs["strict_precision"][:, :, 4:] == -1) and np.all(blobs["strict_precision"][:, :, :4, 0, 2] > -1)
    crowd = np.flatnonzero(b["gt_iscrowd"] == 1)
    for n in crowd:                                   # every crowd region is matched by several detections
        c = (int(b["gt_image"][n]), int(b["gt_category"][n]))
        ci = list(blobs["m_cell"]).index(c[0] * K + c[1])
        seg = blobs["strict_dtm"][0, 0, blobs["m_off"][ci]:blobs["m_off"][ci + 1]]
        assert np.count_nonzero(seg == cells_gt[c].index(n + 1) + 1) >= 2, c
    for a in range(4):                                # every area range ignores some ground truth
        lo, hi = blobs["area_rng"][a]
        if a:
            assert np.any((b["gt_area"] < lo) | (b["gt_area"] > hi))
    ties = 0
    for cat in range(K):
        s = b["det_scores"][b["det_category"] == cat]
        ties += int(np.count_nonzero(np.unique(s, return_counts=True)[1] > 1))
    assert ties >= 50, ties
    return blobs


def main():
    blobs = generate()
    np.savez_compressed(OUT, **blobs)
    print("wrote %s: %d ground truths, %d detections, %d evaluated cells, %d bytes" % (
        OUT, len(blobs["gt_area"]), len(blobs["det_scores"]), len(blobs["m_cell"]), os.path.getsize(OUT)))


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
