"""RetinaNet anchor labelling (row f4): oracle pinning on the CPU, HIP parity on the GPU."""
import hashlib
import os

import numpy as np
import pytest

from oracle import anchors as OA

HERE = os.path.dirname(os.path.abspath(__file__))
TARGET_TOL = dict(rtol=2e-6, atol=2e-7)          # box regression targets against the oracle (logf, float32 divisions)
DETECT_BOX_TOL = dict(rtol=2e-5, atol=2e-3)      # decoded boxes against the oracle (expf)


def rand_gts(rng, n, H=640, W=896, integer=False):
    x1 = rng.uniform(0, W - 40, n)
    y1 = rng.uniform(0, H - 40, n)
    w = rng.uniform(12, 400, n)
    h = rng.uniform(12, 400, n)
    b = np.stack([x1, y1, np.minimum(x1 + w, W - 1), np.minimum(y1 + h, H - 1)], 1)
    if integer:
        b = np.round(b)          # integer boxes produce exact IoU ties between anchors
    return b.astype(np.float32), rng.integers(1, 81, n).astype(np.int32)


def test_cell_anchors_known_answers_and_product_module():
    import ssad_amd  # noqa: F401
    from ssad_amd.modeling import generate_anchors as GA
    # outputs of the reference's generate_anchors(16, (128, 256, 512), (0.5, 1, 2)) run in
    # the build container (its docstring table, generate_anchors.py:28-50, is the 1-based
    # MATLAB original; the code subtracts 1, :77)
    want = {(128, 0.5): [-84, -40, 99, 55], (256, 0.5): [-176, -88, 191, 103],
            (512, 0.5): [-360, -184, 375, 199], (128, 1): [-56, -56, 71, 71],
            (512, 1): [-248, -248, 263, 263], (128, 2): [-36, -80, 51, 95],
            (512, 2): [-168, -344, 183, 359]}
    for (size, ar), box in want.items():
        assert np.array_equal(GA.cell_anchor(16, size, ar), np.array(box, float))
        assert np.array_equal(OA.generate_anchors(16, (size,), (ar,))[0], np.array(box, float))
    assert np.array_equal(GA.cell_anchors().astype(np.float32), OA.cell_anchors())
    assert GA.field_sizes() == [128, 64, 32, 16, 8]
    anchors, meta = OA.all_anchors()
    assert anchors.shape == (9 * (128 ** 2 + 64 ** 2 + 32 ** 2 + 16 ** 2 + 8 ** 2), 4)


def test_oracle_iou_bit_exact_vs_compiled_reference(golden_dir):
    """tests/golden/iou_ref.npz (tests/golden/make_iou_golden.py): the SHA-256 of what the reference's compiled
    IoU routine returned for every anchor against 37 random and 37 integer (tie-producing) ground-truth boxes;
    the oracle's output must have the same bytes."""
    z = np.load(os.path.join(golden_dir, "iou_ref.npz"))
    anchors, _ = OA.all_anchors()
    for case in ("random", "integer"):
        got = OA.bbox_overlaps(anchors, z["gts_" + case])
        assert got.dtype == np.float32 and got.shape == tuple(z["shape_" + case]), case
        digest = hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()
        assert digest == str(z["sha256_" + case]), case


def test_oracle_labelling_invariants():
    rng = np.random.default_rng(6)
    g = [rand_gts(rng, 7, integer=True), rand_gts(rng, 3)]
    out = OA.retinanet_blobs([x[0] for x in g], [x[1] for x in g], 640, 896)
    for lvl, (h, w) in zip(range(3, 8), ((80, 112), (40, 56), (20, 28), (10, 14), (5, 7))):
        lab = out["labels_fpn%d" % lvl]
        assert lab.shape == (2, 9, h, w) and lab.dtype == np.int32
        assert lab.min() >= -1 and lab.max() <= 80
        locs, tg = out["locs_fpn%d" % lvl], out["targets_fpn%d" % lvl]
        assert locs.shape == tg.shape and locs.shape[1] == 4
        # list order: image, anchor, y, x
        key = [tuple(r) for r in locs]
        assert key == sorted(key)
        inside = (locs[:, 2] < h) & (locs[:, 3] < w)
        for r in locs[inside]:
            assert lab[int(r[0]), int(r[1]) // 4, int(r[2]), int(r[3])] > 0
    assert out["fg_num"] > 0 and out["bg_num"] > out["fg_num"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["random", "integer_ties", "single_gt_image"])
def test_device_labelling_matches_oracle(case):
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd.roi_data.retinanet import RetinanetLabeler
    rng = np.random.default_rng({"random": 11, "integer_ties": 12, "single_gt_image": 13}[case])
    N, Gmax, H, W = 3, 24, 640, 896
    counts = [9, 24, 1]
    gts = [rand_gts(rng, c, H, W, integer=(case == "integer_ties")) for c in counts]
    boxes = np.zeros((N, Gmax, 4), np.float32)
    classes = np.zeros((N, Gmax), np.int32)
    for i, (b, c) in enumerate(gts):
        boxes[i, :len(b)] = b
        classes[i, :len(c)] = c
    lab = RetinanetLabeler(N, Gmax, H, W)
    blobs = lab(torch.as_tensor(boxes).cuda(), torch.as_tensor(classes).cuda(),
                torch.as_tensor(np.array(counts, np.int32)).cuda())
    ref = OA.retinanet_blobs([g[0] for g in gts], [g[1] for g in gts], H, W)
    assert float(blobs["retnet_fg_num"]) == float(ref["fg_num"])
    assert float(blobs["retnet_bg_num"]) == float(ref["bg_num"])
    for lvl in range(3, 8):
        got = blobs["retnet_cls_labels_fpn%d" % lvl].cpu().numpy()
        assert np.array_equal(got, ref["labels_fpn%d" % lvl]), "labels level %d" % lvl
        locs = blobs["retnet_roi_fg_bbox_locs_fpn%d" % lvl].cpu().numpy()
        assert np.array_equal(locs, ref["locs_fpn%d" % lvl]), "fg list level %d" % lvl
        tg = blobs["retnet_roi_bbox_targets_fpn%d" % lvl].cpu().numpy()
        np.testing.assert_allclose(tg, ref["targets_fpn%d" % lvl], **TARGET_TOL)


@pytest.mark.gpu
def test_device_labelling_image_without_ground_truth():
    """Documented deviation: the reference asserts; here such an image is all background."""
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd.roi_data.retinanet import RetinanetLabeler
    rng = np.random.default_rng(21)
    N, Gmax, H, W = 3, 8, 640, 896
    counts = [5, 0, 8]
    gts = [rand_gts(rng, max(c, 1), H, W) for c in counts]
    boxes = np.zeros((N, Gmax, 4), np.float32)
    classes = np.zeros((N, Gmax), np.int32)
    for i, (b, c) in enumerate(gts):
        boxes[i, :counts[i]] = b[:counts[i]]
        classes[i, :counts[i]] = c[:counts[i]]
    blobs = RetinanetLabeler(N, Gmax, H, W)(
        torch.as_tensor(boxes).cuda(), torch.as_tensor(classes).cuda(),
        torch.as_tensor(np.array(counts, np.int32)).cuda())
    ref = OA.retinanet_blobs([gts[0][0], gts[2][0]], [gts[0][1], gts[2][1]], H, W)
    T = 9 * (128 ** 2 + 64 ** 2 + 32 ** 2 + 16 ** 2 + 8 ** 2)
    assert float(blobs["retnet_fg_num"]) == float(ref["fg_num"])
    assert float(blobs["retnet_bg_num"]) == float(np.float32(float(ref["bg_num"]) + (T + 1.0) * 80))
    for lvl in range(3, 8):
        got = blobs["retnet_cls_labels_fpn%d" % lvl].cpu().numpy()
        assert np.array_equal(got[[0, 2]], ref["labels_fpn%d" % lvl])
        assert not got[1].any()
        locs = blobs["retnet_roi_fg_bbox_locs_fpn%d" % lvl].cpu().numpy().copy()
        assert not (locs[:, 0] == 1).any()
        locs[:, 0] = np.where(locs[:, 0] == 2, 1, locs[:, 0])
        assert np.array_equal(locs, ref["locs_fpn%d" % lvl])


# ---------------------------------------------------------------------------
# inference post-processing (second half of row f4)
# ---------------------------------------------------------------------------

def _detect_inputs(rng, shapes, shift):
    """Scores are exact multiples of 2^-shift, each used once per level: distinct in
    float32 (ties are unspecified in the reference).  shift 24: most of the finest level
    passes the 0.05 threshold; shift 26: only part of the finest level and (threshold 0)
    the coarsest level produce candidates."""
    probs, deltas = [], []
    for h, w in shapes:
        n = 720 * h * w
        vals = (rng.permutation(n) + 1).astype(np.float64) * 2.0 ** -shift
        probs.append(vals.astype(np.float32).reshape(1, 720, h, w))
        deltas.append((rng.standard_normal((1, 36, h, w)) * 0.4).astype(np.float32))
    return probs, deltas


def test_detect_oracle_invariants():
    from oracle import detect as OD
    rng = np.random.default_rng(3)
    shapes = [(20, 28), (10, 14), (5, 7)]
    probs, deltas = _detect_inputs(rng, shapes, 19)
    cells = np.array([[OA.generate_cell64(l, a) for a in range(9)] for l in range(3, 6)])
    d = OD.im_detect_bbox(probs, deltas, cells, (150, 210), 1.0)
    assert d.shape[1] == 6 and 0 < d.shape[0] <= 100
    assert np.all(np.diff(d[:, 4]) <= 0)                       # sorted by score
    assert d[:, 0].min() >= 0 and d[:, 2].max() <= 209 and d[:, 3].max() <= 149
    assert set(np.unique(d[:, 5])) <= set(range(1, 81))
    # NMS: no two survivors of one class overlap by >= 0.5
    for c in np.unique(d[:, 5]):
        b = d[d[:, 5] == c]
        assert len(OD.nms(b[:, :5], 0.5)) == len(b)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["five_levels", "few_candidates"])
def test_device_detect_matches_oracle(case):
    import torch
    import ssad_amd  # noqa: F401
    from oracle import detect as OD
    from ssad_amd.roi_data.retinanet import RetinanetDetector
    rng = np.random.default_rng(41 if case == "five_levels" else 42)
    shapes = [(80, 112), (40, 56), (20, 28), (10, 14), (5, 7)]
    probs, deltas = _detect_inputs(rng, shapes, 24 if case == "five_levels" else 26)
    cells = np.array([[OA.generate_cell64(l, a) for a in range(9)] for l in range(3, 8)])
    im_h, im_w, scale = 600, 850, 0.9375
    ref = OD.im_detect_bbox(probs, deltas, cells, (im_h, im_w), scale)
    det = RetinanetDetector(shapes)
    got = det([torch.as_tensor(p).cuda() for p in probs], [torch.as_tensor(d).cuda() for d in deltas],
              im_h, im_w, scale).cpu().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(got[:, 4], ref[:, 4])                # scores, in order
    assert np.array_equal(got[:, 5], ref[:, 5])                # classes
    np.testing.assert_allclose(got[:, :4], ref[:, :4], **DETECT_BOX_TOL)


@pytest.mark.gpu
def test_device_detect_selection_ties_small_levels_and_topn_cut():
    """Round 6: the top-k per level is this repo's radix select + rank sort (no hipCUB).  Its corner cases: equal scores
    (the documented tie order: lower element index first into the top-k, equal final scores by class), a level with
    fewer elements than pre_nms_topn, and a topn that cuts INSIDE a run of equal scores."""
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd.roi_data.retinanet import RetinanetDetector
    shapes = [(2, 3)]                                     # one level (= k_max: threshold 0), 720 * 6 = 4320 elements
    prob = np.zeros((1, 720, 2, 3), np.float32)
    delta = np.zeros((1, 36, 2, 3), np.float32)
    # anchor 0, classes 7 / 3 / 11 at three different cells: equal scores; class 5 higher
    prob[0, 7, 0, 0] = prob[0, 3, 1, 2] = prob[0, 11, 0, 1] = 0.5
    prob[0, 5, 1, 1] = 0.75
    det = RetinanetDetector(shapes, pre_nms_topn=1000)
    got = det([torch.as_tensor(prob).cuda()], [torch.as_tensor(delta).cuda()], 64, 64, 1.0).cpu().numpy()
    assert got.shape[0] == 4 and got[0, 4] == 0.75 and got[0, 5] == 6
    assert list(got[1:, 4]) == [0.5, 0.5, 0.5] and list(got[1:, 5]) == [4, 8, 12]        # equal scores: by class
    # topn = 2 cuts inside the run of three equal scores: the two with the LOWER element index stay
    # (element index = (class * H + y) * W + x for anchor 0: class 3 -> 23, class 7 -> 42, class 11 -> 67)
    det2 = RetinanetDetector(shapes, pre_nms_topn=3, dets_per_im=3)
    got2 = det2([torch.as_tensor(prob).cuda()], [torch.as_tensor(delta).cuda()], 64, 64, 1.0).cpu().numpy()
    assert list(got2[:, 5]) == [6, 4, 8]
    # nothing above zero at all: no detections, and the call is repeatable on the same workspace
    none = det([torch.zeros_like(torch.as_tensor(prob)).cuda()], [torch.as_tensor(delta).cuda()], 64, 64, 1.0)
    assert none.shape[0] == 0
    again = det([torch.as_tensor(prob).cuda()], [torch.as_tensor(delta).cuda()], 64, 64, 1.0).cpu().numpy()
    assert np.array_equal(again, got)


def test_product_library_links_no_sort_library():
    """The product .so depends on the HIP runtime only: no rocPRIM / hipCUB symbol is left (rounds 1-5: detect.hip sorted
    with hipcub::DeviceRadixSort)."""
    import subprocess
    import ssad_amd  # noqa: F401
    from ssad_amd import kernels as K
    out = subprocess.run(["nm", "-D", "-C", K.LIB_PATH], capture_output=True, text=True).stdout
    assert "rocprim" not in out and "hipcub" not in out
    src = open(os.path.join(os.path.dirname(K.LIB_PATH), "csrc", "kernels", "detect.hip")).read()
    assert "#include <hipcub" not in src and "rocprim" not in src.replace("rocPRIM", "")


# ---------------------------------------------------------------------------
# pinned by the reference's own Python: tests/golden/anchor_labels_ref.npz was written by
# detectron/lib/roi_data/retinanet.py:97-306 (+ data_utils.py, generate_anchors.py, the compiled
# cython_bbox.pyx) and utils/boxes.py run in the build container (tests/golden/make_anchor_labels.py)
# ---------------------------------------------------------------------------

def _ref_fixture():
    return np.load(os.path.join(HERE, "golden", "anchor_labels_ref.npz"))


def test_oracle_labelling_reproduces_the_reference_blobs_exactly():
    z = _ref_fixture()
    H, W = [int(v) for v in z["image_hw"]]
    boxes, classes = [], []
    for i, s in enumerate(z["scales"]):
        boxes.append(z["gt_boxes_%d" % i] * float(s))           # retinanet.py:122: float32 boxes x python float
        classes.append(z["gt_classes_%d" % i])
        assert boxes[-1].dtype == np.float32
    out = OA.retinanet_blobs(boxes, classes, H, W)
    assert np.array_equal(np.float32(out["fg_num"]), z["blob_retnet_fg_num"][0])
    assert np.array_equal(np.float32(out["bg_num"]), z["blob_retnet_bg_num"][0])
    n_fg = 0
    for lvl in range(3, 8):
        lab = z["blob_retnet_cls_labels_fpn%d" % lvl]
        assert lab.dtype == np.int32 and np.array_equal(out["labels_fpn%d" % lvl], lab), lvl
        locs = z["blob_retnet_roi_fg_bbox_locs_fpn%d" % lvl]
        assert np.array_equal(out["locs_fpn%d" % lvl], locs), lvl
        tg = z["blob_retnet_roi_bbox_targets_fpn%d" % lvl]
        assert tg.dtype == np.float32 and np.array_equal(out["targets_fpn%d" % lvl], tg), lvl
        n_fg += locs.shape[0]
        assert locs.shape[0] > 0                                   # every level carries foreground anchors
    # the anchors themselves: first anchor of each (level, octave, aspect) field, and the field sizes
    cells = OA.cell_anchors()
    assert np.array_equal(cells.reshape(-1, 4), z["cell_anchors"])
    assert [OA.field_size(2.0 ** (3 + k // 9)) for k in range(45)] == [int(v) for v in z["field_sizes"]]


def test_oracle_nms_reproduces_the_reference_nms():
    """Greedy NMS pinned by the reference's own text: tests/golden/nms_ref.npz holds the survivors that
    detectron/lib/utils/cython_nms.pyx:37-92 -- executed as Python after its C type declarations were stripped
    (tests/golden/make_nms_golden.py; the .pyx does not build under Cython 3 / numpy 2) -- leaves of seeded detections:
    1 ... 400 boxes at three thresholds, duplicates, a box swallowed by a larger one.  Same survivors, same order."""
    from oracle import detect as OD
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nms_ref.npz"))
    n = int(z["n_cases"])
    assert n == 18
    sizes = set()
    for k in range(n):
        dets, thresh, keep = z["dets_%d" % k], float(z["thresh_%d" % k]), z["keep_%d" % k]
        got = OD.nms(dets, thresh)
        assert np.array_equal(np.asarray(got, np.int64), keep), (k, thresh)
        sizes.add((dets.shape[0], keep.size))
    assert any(a > b for a, b in sizes) and any(a == 400 for a, _ in sizes)       # something was suppressed, at size


def test_oracle_box_decoding_reproduces_the_reference():
    """bbox_transform (with the BBOX_XFORM_CLIP clamp) and clip_tiled_boxes of utils/boxes.py:193-260."""
    from oracle import detect as OD
    z = _ref_fixture()
    got = OD.bbox_transform(z["decode_anchors"], z["decode_deltas"])
    # The fixture was computed under numpy 2, whose promotion rules differ from the numpy 1.x the
    # reference was written for: `np.minimum(dw, cfg.BBOX_XFORM_CLIP)` (boxes.py:176-177) meets a
    # float64 SCALAR (np.log's result) and the width / height expressions run in float64 there before
    # they are stored into the float32 result; under the old value-based casting they stay float32,
    # which is what the oracle (and detect.hip) follow.  Hence 1-ulp differences: compared at 1e-6
    # relative, not bit for bit.
    assert str(z["decode_boxes_dtype_was"]) == "float32"
    assert np.allclose(got, z["decode_boxes"], rtol=1e-6, atol=1e-4)
    clipped = OD.clip_tiled_boxes(got.copy(), (600, 899))
    assert np.allclose(clipped, z["decode_clipped"], rtol=1e-6, atol=1e-4)
    assert clipped.min() >= 0 and clipped[:, 0::2].max() <= 898 and clipped[:, 1::2].max() <= 599
    big = z["decode_deltas"][:, 2] >= 6.0                         # the BBOX_XFORM_CLIP clamp was exercised
    assert big.any() and np.allclose((got[big, 2] - got[big, 0] + 1) /
                                     (z["decode_anchors"][big, 2] - z["decode_anchors"][big, 0] + 1), 62.5, rtol=1e-5)
