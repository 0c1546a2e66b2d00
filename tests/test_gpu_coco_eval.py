"""COCO box evaluation on the device (csrc/kernels/coco_eval.hip, datasets/detection_evaluator.py) against
tests/golden/coco_eval_ref.npz, which the reference's own evaluator wrote (tests/golden/make_coco_eval_golden.py)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(20, 28), (10, 14), (5, 7)]          # test_gpu_soft_nms.py's levels
MODES = (("strict", False), ("relax", True))
KEYS = ("precision", "recall", "scores", "stats", "per_category_ap")
PR_TOL = 1e-12         # precision / recall against the fixture (test_precision_recall_and_scores says why)


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(HERE, "golden", "coco_eval_ref.npz"))


def build(z, relax, order=None, cap=160):
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd.datasets import DetectionEvaluator
    I = int(z["num_images"])
    ev = DetectionEvaluator(I, int(z["num_categories"]), z["gt_boxes"], z["gt_area"], z["gt_iscrowd"], z["gt_image"],
                            z["gt_category"], iou_thrs=z["iou_thrs"], rec_thrs=z["rec_thrs"],
                            max_dets=tuple(int(m) for m in z["max_dets"]), area_rng=z["area_rng"],
                            small_box_relax=relax, max_dets_per_image=cap)
    for img in (range(I) if order is None else order):
        sel = z["det_image"] == img
        ev.add_detections(int(img), torch.from_numpy(z["det_boxes"][sel]).cuda(), z["det_scores"][sel],
                          z["det_category"][sel])
    return ev


@pytest.fixture(scope="module")
def results(z):
    """One evaluation per mode, shared; nothing changes it."""
    return {mode: build(z, relax).evaluate(return_matches=True) for mode, relax in MODES}


@pytest.mark.parametrize("mode", ["strict", "relax"])
def test_matches_and_ignore_flags_equal_the_reference(z, results, mode):
    m = results[mode]["matches"]
    assert np.array_equal(m["cell"], z["m_cell"]) and np.array_equal(m["offsets"], z["m_off"])
    assert np.array_equal(m["npig"], z["m_npig"])
    assert m["dt_match"].dtype == np.int32 and np.array_equal(m["dt_match"], z[mode + "_dtm"])
    assert m["dt_ignore"].dtype == bool and np.array_equal(m["dt_ignore"], z[mode + "_dtig"])


@pytest.mark.parametrize("mode", ["strict", "relax"])
def test_precision_recall_and_scores(z, results, mode):
    """Values in [0, 1]: 1e-12 is about 4 500 double epsilons, and six orders below 1/nd^2 ~ 1e-6, the smallest
    spacing two different PR points can have at this size.  The -1 pattern and the scores are exact."""
    r = results[mode]
    for name in ("precision", "recall"):
        got, want = r[name], z["%s_%s" % (mode, name)]
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.array_equal(got == -1, want == -1)
        err = float(np.abs(got - want).max())
        print(mode, name, "max abs error", err)
        assert err <= PR_TOL
    assert r["scores"].tobytes() == z[mode + "_scores"].tobytes()


@pytest.mark.parametrize("mode", ["strict", "relax"])
def test_stats_and_per_category_ap(z, results, mode):
    r = results[mode]
    err = float(np.abs(r["stats"] - z[mode + "_stats"]).max())
    print(mode, "stats max abs error", err)
    assert r["stats"].shape == (12,) and err <= 1e-12
    want = np.full(int(z["num_categories"]), -1.0)
    for k in range(len(want)):
        s = z[mode + "_precision"][:, :, k, 0, -1]
        if np.any(s > -1):
            want[k] = np.mean(s[s > -1])
    assert np.array_equal(r["per_category_ap"] == -1, want == -1) and np.all(want[4:] == -1)
    assert float(np.abs(r["per_category_ap"] - want).max()) <= 1e-12


def test_order_of_add_calls_and_workspace_reuse(z, results):
    """Images added last to first give the same bytes; so does a second instance that finds the shared workspace
    full of another evaluation's (the other mode's) intermediate results."""
    I = int(z["num_images"])
    back = build(z, False, order=range(I - 1, -1, -1)).evaluate(return_matches=True)
    for key in KEYS:
        assert back[key].tobytes() == results["strict"][key].tobytes(), key
    for key in ("cell", "offsets", "dt_match", "dt_ignore", "npig"):
        assert back["matches"][key].tobytes() == results["strict"]["matches"][key].tobytes(), key
    build(z, True).evaluate()
    again = build(z, False).evaluate()
    for key in KEYS:
        assert again[key].tobytes() == results["strict"][key].tobytes(), key


def test_detector_rows_through_add(z):
    """Two images of RetinanetDetector output: `add` (device rows, as they are) equals the same rows copied through
    the host into `add_detections`, byte for byte.  With the ground truth equal to each image's detections (xywh, + 1)
    every detection finds its own box at IoU 1 (greedy NMS at 0.5 leaves no second box of its class above 0.5), so
    every tp count is the position and no fp exists: pr = tp / (tp + eps) is 1.0 from the second position on (2 + eps
    rounds to 2), the running maximum carries it to the first, and the last recall is 1.0 -- AP@0.5 is exactly 1.0 for
    every category with at least two detections.  A category with ONE detection has the single point
    1 / (1 + eps) = 1 - 2^-52 in the reference's arithmetic, and that is what is asserted for it."""
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd.datasets import DetectionEvaluator
    from ssad_amd.roi_data.retinanet import RetinanetDetector
    from test_anchor_labels import _detect_inputs
    det = RetinanetDetector(SHAPES)
    rows = []
    for seed in (43, 44):
        probs, deltas = _detect_inputs(np.random.default_rng(seed), SHAPES, 19)
        rows.append(det([torch.as_tensor(p).cuda() for p in probs], [torch.as_tensor(d).cuda() for d in deltas],
                        150, 210, 1.0).clone())
    host = [r.cpu().numpy() for r in rows]
    assert all(0 < len(h) <= 100 for h in host)
    gt = np.concatenate(host)
    w = (gt[:, 2] - gt[:, 0] + np.float32(1)).astype(np.float64)
    h = (gt[:, 3] - gt[:, 1] + np.float32(1)).astype(np.float64)
    args = (2, 80, np.stack([gt[:, 0].astype(np.float64), gt[:, 1].astype(np.float64), w, h], 1), w * h,
            np.zeros(len(gt), np.uint8), np.repeat([0, 1], [len(host[0]), len(host[1])]).astype(np.int32),
            gt[:, 5].astype(np.int32) - 1)
    a, b = DetectionEvaluator(*args), DetectionEvaluator(*args)
    for img in (0, 1):
        a.add(img, rows[img])
        b.add_detections(img, host[img][:, :4].copy(), host[img][:, 4].copy(), host[img][:, 5].astype(np.int32) - 1)
    ra, rb = a.evaluate(), b.evaluate()
    for key in KEYS:
        assert ra[key].tobytes() == rb[key].tobytes(), key
    count = np.bincount(gt[:, 5].astype(np.int64) - 1, minlength=80)
    assert np.count_nonzero(count >= 2) >= 10
    p50 = ra["precision"][0, :, :, 0, -1]                                    # [R][K]
    want = np.where(count >= 2, 1.0, np.where(count == 1, 1.0 / (1.0 + np.spacing(1)), -1.0))
    assert np.array_equal(p50, np.broadcast_to(want, p50.shape)), np.flatnonzero(np.any(p50 != want, axis=0))
    assert np.all(ra["per_category_ap"][count >= 2] == 1.0)
    assert np.all(ra["recall"][0, count > 0, 0, -1] == 1.0)


def test_capacity_and_duplicates_raise(z):
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd import kernels as K
    ev = build(z, False, order=[0, 2])
    with pytest.raises(K.KernelError, match="added before"):
        ev.add(2, torch.zeros((3, 6), dtype=torch.float32, device="cuda"))
    with pytest.raises(K.KernelError, match="exceed"):
        ev.add(3, torch.zeros((161, 6), dtype=torch.float32, device="cuda"))
    with pytest.raises(K.KernelError, match="exceed"):
        ev.add_detections(3, np.zeros((161, 4), np.float32), np.zeros(161, np.float32), np.zeros(161, np.int32))
    # a class outside the categories cannot be seen without a read-back: evaluate() reports it
    rows = torch.zeros((2, 6), dtype=torch.float32, device="cuda")
    rows[:, 5] = 7.0
    ev.add(3, rows)
    with pytest.raises(K.KernelError, match="outside"):
        ev.evaluate()
