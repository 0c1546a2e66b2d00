"""COCO box evaluation: the fixture tests/golden/coco_eval_ref.npz (written by the reference's own evaluator,
tests/golden/make_coco_eval_golden.py), a lane-by-lane numpy statement of what csrc/kernels/coco_eval.hip does, and
the argument checks of datasets/detection_evaluator.py -- none of it needs a GPU.

The statement does the kernels' float64 operations one by one in the same order (Python floats: IEEE doubles, one
rounding per operation, nothing fused), so it is expected to EQUAL the fixture: matches exactly, precision exactly."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
MODES = (("strict", False), ("relax", True))


def fixture():
    return np.load(os.path.join(HERE, "golden", "coco_eval_ref.npz"))


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------

def box_iou(d, g, crowd):
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if not (w > 0 and h > 0):
        return 0.0
    i = w * h
    da = d[2] * d[3]
    return i / (da if crowd else da + g[2] * g[3] - i)


def spec_match(I, K, gt_boxes, gt_area, gt_crowd, gt_image, gt_category, det_boxes, det_scores, det_category,
               det_image, iou_thrs, area_rng, max_det, relax):
    """coco_match_kernel: per (image, category) cell the detections ranked by score (equal scores in the given order),
    cut at max_det; lane (a, t) walks them over the ground truths, non-ignored first, then -- only while it holds no
    match -- the ignored ones.  Returns cell, offsets, dt_match [A][T][sum D], dt_ignore, npig [C][A] and the ranked
    detections' global indices."""
    A, T = len(area_rng), len(iou_thrs)
    w32 = det_boxes[:, 2] - det_boxes[:, 0] + F(1)
    h32 = det_boxes[:, 3] - det_boxes[:, 1] + F(1)
    assert w32.dtype == F
    dxywh = [(float(b[0]), float(b[1]), float(w), float(h)) for b, w, h in zip(det_boxes, w32, h32)]
    score = [float(s) for s in det_scores]
    gts, dts = {}, {}
    for n in range(len(gt_area)):
        gts.setdefault((int(gt_image[n]), int(gt_category[n])), []).append(n)
    for n in range(len(score)):
        dts.setdefault((int(det_image[n]), int(det_category[n])), []).append(n)
    cells, off, npig, dtm, dtig, ranked = [], [0], [], [], [], []
    for img in range(I):
        for k in range(K):
            if (img, k) not in gts and (img, k) not in dts:
                continue
            g_idx, d_idx = gts.get((img, k), []), dts.get((img, k), [])
            d_idx = sorted(d_idx, key=lambda n: -score[n])[:max_det]            # stable
            gb = [tuple(float(v) for v in gt_boxes[n]) for n in g_idx]
            D = len(d_idx)
            m_out, i_out, n_out = np.zeros((A, T, D), np.int32), np.zeros((A, T, D), bool), []
            for a in range(A):
                lo, hi = float(area_rng[a][0]), float(area_rng[a][1])
                ign = [bool(gt_crowd[n]) or float(gt_area[n]) < lo or float(gt_area[n]) > hi for n in g_idx]
                n_out.append(ign.count(False))
                for t in range(T):
                    thr = min(float(iou_thrs[t]), 1 - 1e-10)
                    gtm = [False] * len(g_idx)
                    for d, n in enumerate(d_idx):
                        iou, m = thr, -1
                        for turn in (False, True):
                            if turn and m >= 0:
                                break
                            for g in range(len(g_idx)):
                                crowd = bool(gt_crowd[g_idx[g]])
                                if ign[g] != turn or (gtm[g] and not crowd):
                                    continue
                                tiou = iou
                                if relax:
                                    gw, gh = gb[g][2], gb[g][3]
                                    tiou = min(iou, (1.0 * gw * gh) / ((gw + 10.0) * (gh + 10.0)))
                                v = box_iou(dxywh[n], gb[g], crowd)
                                if v < tiou:
                                    continue
                                iou, m = v, g
                        if m >= 0:
                            m_out[a, t, d], i_out[a, t, d], gtm[m] = m + 1, ign[m], True
                        else:
                            da = dxywh[n][2] * dxywh[n][3]
                            i_out[a, t, d] = da < lo or da > hi
            cells.append(img * K + k)
            off.append(off[-1] + D)
            npig.append(n_out)
            dtm.append(m_out)
            dtig.append(i_out)
            ranked += d_idx
    return {"cell": np.array(cells, np.int32), "offsets": np.array(off, np.int32),
            "dt_match": np.concatenate(dtm, axis=2) if dtm else np.zeros((A, T, 0), np.int32),
            "dt_ignore": np.concatenate(dtig, axis=2) if dtig else np.zeros((A, T, 0), bool),
            "npig": np.array(npig, np.int32).reshape(-1, A), "ranked": np.array(ranked, np.int64)}


def spec_accumulate(K, m, det_scores, rec_thrs, max_dets):
    """coco_accumulate_kernel: per (category, area range, maxDets entry, threshold) the tp / fp totals in a forward
    pass, then one backward pass that takes the cumulative sums apart again, carries the right-to-left maximum of the
    precision and hands it to every recall threshold whose searchsorted(rc, thr, 'left') position it passes."""
    A, T = m["dt_match"].shape[:2]
    R, M = len(rec_thrs), len(max_dets)
    eps = float(np.spacing(1))
    rec = [float(r) for r in rec_thrs]
    precision, scores, recall = -np.ones((T, R, K, A, M)), -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for k in range(K):
        mine = [c for c in range(len(m["cell"])) if m["cell"][c] % K == k]        # ascending: image order
        if not mine:
            continue
        for mi, md in enumerate(max_dets):
            cols = np.concatenate([np.arange(m["offsets"][c], min(m["offsets"][c + 1], m["offsets"][c] + md))
                                   for c in mine]).astype(np.int64)
            sc = [float(det_scores[n]) for n in m["ranked"][cols]]
            order = sorted(range(len(sc)), key=lambda i: -sc[i])                   # stable
            cols, sc = cols[order], [sc[i] for i in order]
            nd = len(sc)
            for a in range(A):
                npig = int(sum(m["npig"][c][a] for c in mine))
                if npig == 0:
                    continue
                for t in range(T):
                    mt, ig = m["dt_match"][a, t, cols] != 0, m["dt_ignore"][a, t, cols]
                    tps, fps = (mt & ~ig).tolist(), (~mt & ~ig).tolist()
                    tp, fp = sum(tps), sum(fps)
                    rc_last = tp / npig
                    recall[t, k, a, mi] = rc_last if nd else 0.0
                    precision[t, :, k, a, mi] = scores[t, :, k, a, mi] = 0.0
                    r = R - 1
                    while r >= 0 and (nd == 0 or not rc_last >= rec[r]):
                        r -= 1
                    pm = -1.0
                    for i in range(nd - 1, -1, -1):
                        if r < 0:
                            break
                        pr = tp / (fp + tp + eps)
                        pm = max(pm, pr)
                        tp, fp = tp - tps[i], fp - fps[i]
                        rc_prev = tp / npig
                        while r >= 0 and (i == 0 or rec[r] > rc_prev):
                            precision[t, r, k, a, mi], scores[t, r, k, a, mi] = pm, sc[i]
                            r -= 1
    return precision, recall, scores


def spec_eval(z, relax):
    m = spec_match(int(z["num_images"]), int(z["num_categories"]), z["gt_boxes"], z["gt_area"], z["gt_iscrowd"],
                   z["gt_image"], z["gt_category"], z["det_boxes"], z["det_scores"], z["det_category"],
                   z["det_image"], z["iou_thrs"], z["area_rng"], int(z["max_dets"][-1]), relax)
    return m, spec_accumulate(int(z["num_categories"]), m, z["det_scores"], z["rec_thrs"], z["max_dets"].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------

def test_generator_reproduces_the_committed_fixture():
    """Every array of coco_eval_ref.npz comes out of the reference's VIDeval again, bit for bit (only where the
    reference tree is present: the fixture is what travels)."""
    if not os.path.isfile("/root/reference/detectron/lib/datasets/vid_eval.py"):
        pytest.skip("the reference tree is not on this machine")
    spec = importlib.util.spec_from_file_location("make_coco_eval_golden",
                                                  os.path.join(HERE, "golden", "make_coco_eval_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh, z = gen.generate(), fixture()
    assert sorted(fresh) == sorted(z.files)
    for name in z.files:
        a, b = np.asarray(fresh[name]), z[name]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name


def test_fixture_holds_what_it_is_for():
    z = fixture()
    K = int(z["num_categories"])
    assert z.files and os.path.getsize(os.path.join(HERE, "golden", "coco_eval_ref.npz")) < 512 * 1024
    gt_cells = np.bincount(z["gt_image"] * K + z["gt_category"])
    dt_cells = np.bincount(z["det_image"] * K + z["det_category"])
    assert gt_cells.max() >= 70 and dt_cells.max() >= 130 > z["max_dets"][-1]
    assert np.bincount(z["det_image"]).max() <= 160
    assert z["det_boxes"].dtype == F and z["det_scores"].dtype == F
    assert not np.array_equal(z["strict_precision"], z["relax_precision"])
    assert z["strict_stats"].shape == (12,) and np.all(z["strict_stats"] > 0)


@pytest.mark.parametrize("mode,relax", MODES)
def test_statement_equals_the_reference(mode, relax):
    z = fixture()
    m, (precision, recall, scores) = spec_eval(z, relax)
    assert np.array_equal(m["cell"], z["m_cell"]) and np.array_equal(m["offsets"], z["m_off"])
    assert np.array_equal(m["npig"], z["m_npig"])
    assert np.array_equal(m["dt_match"], z[mode + "_dtm"])
    assert np.array_equal(m["dt_ignore"], z[mode + "_dtig"])
    assert precision.tobytes() == z[mode + "_precision"].tobytes()
    assert recall.tobytes() == z[mode + "_recall"].tobytes()
    assert scores.tobytes() == z[mode + "_scores"].tobytes()


def test_argument_checks_come_before_the_library(monkeypatch):
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd import kernels as K
    from ssad_amd.datasets import DetectionEvaluator

    def never():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(K, "lib", never)
    z = fixture()
    gt = dict(gt_boxes_xywh=z["gt_boxes"], gt_area=z["gt_area"], gt_iscrowd=z["gt_iscrowd"], gt_image=z["gt_image"],
              gt_category=z["gt_category"])

    def build(I=12, Kc=6, **kw):
        args = dict(gt, device="cpu")
        args.update(kw)
        return DetectionEvaluator(I, Kc, **args)

    for match, kw in (("num_images", dict(I=0)), ("num_categories", dict(Kc=-1)), ("num_images", dict(I=2.5)),
                      ("max_dets_per_image", dict(max_dets_per_image=0)),
                      ("gt_boxes_xywh", dict(gt_boxes_xywh=z["gt_boxes"].astype(F))),
                      ("gt_boxes_xywh", dict(gt_boxes_xywh=z["gt_boxes"][:, :3])),
                      ("gt_area", dict(gt_area=z["gt_area"].astype(F))),
                      ("gt_iscrowd", dict(gt_iscrowd=z["gt_iscrowd"].astype(np.float64))),
                      ("gt_iscrowd", dict(gt_iscrowd=z["gt_iscrowd"] + 1)),
                      ("gt_image", dict(gt_image=z["gt_image"][:-1])),
                      ("gt_image", dict(I=10)), ("gt_category", dict(Kc=4)),
                      ("gt_category", dict(gt_category=z["gt_category"] - 1)),
                      ("finite", dict(gt_area=np.where(np.arange(len(z["gt_area"])) == 3, np.nan, z["gt_area"]))),
                      ("iou_thrs", dict(iou_thrs=np.array([0.0, 0.5]))), ("iou_thrs", dict(iou_thrs=np.array([1.5]))),
                      ("iou_thrs", dict(iou_thrs=np.array([0.5], F))), ("iou_thrs", dict(iou_thrs=np.zeros((0,)))),
                      ("rec_thrs", dict(rec_thrs=np.array([0.5, 0.2]))), ("rec_thrs", dict(rec_thrs=np.array([2.0]))),
                      ("max_dets", dict(max_dets=(10, 1, 100))), ("max_dets", dict(max_dets=(0, 10))),
                      ("max_dets", dict(max_dets=())), ("max_dets", dict(max_dets=(1, 10, 10))),
                      ("max_dets above", dict(max_dets=(1, 10, 5000))),
                      ("area_rng", dict(area_rng=[[0, 1, 2]])), ("area_rng", dict(area_rng=[[5.0, 1.0]])),
                      ("small_box_relax", dict(small_box_relax=1))):
        with pytest.raises(K.KernelError, match=match):
            build(**kw)
    ev = build(max_dets_per_image=8)
    host = torch.zeros((3, 6), dtype=torch.float32)
    for match, call in (("device rows", lambda: ev.add(0, host)),
                        ("device rows", lambda: ev.add(0, np.zeros((3, 6), F))),
                        ("image_index", lambda: ev.add_detections(12, np.zeros((1, 4), F), np.zeros(1, F), [0])),
                        ("image_index", lambda: ev.add_detections(-1, np.zeros((1, 4), F), np.zeros(1, F), [0])),
                        ("exceed", lambda: ev.add_detections(0, np.zeros((9, 4), F), np.zeros(9, F), [0] * 9)),
                        ("boxes_xyxy", lambda: ev.add_detections(0, np.zeros((2, 4)), np.zeros(2, F), [0, 0])),
                        ("boxes_xyxy", lambda: ev.add_detections(0, np.zeros((2, 5), F), np.zeros(2, F), [0, 0])),
                        ("scores", lambda: ev.add_detections(0, np.zeros((2, 4), F), np.zeros(2), [0, 0])),
                        ("categories", lambda: ev.add_detections(0, np.zeros((2, 4), F), np.zeros(2, F), [0.0, 1.0])),
                        ("categories", lambda: ev.add_detections(0, np.zeros((2, 4), F), np.zeros(2, F), [0, 6])),
                        ("categories", lambda: ev.add_detections(0, np.zeros((2, 4), F), np.zeros(2, F), [0]))):
        with pytest.raises(K.KernelError, match=match):
            call()
    assert ev._added == set()
