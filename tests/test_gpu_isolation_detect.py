"""Kernel isolation of the data, labelling, detection and evaluation kernels (anchor_labels.hip, detect.hip,
soft_nms.hip, coco_eval.hip, image_blobs.hip) and of the small fp32 entry points the first two isolation files left out.

Part A -- every device operand, output and workspace of a call is a view of ONE sentinel-filled arena
(tests/guarded.py), the workspace exactly *_workspace_bytes long and that length passed.  Where a class owns its
buffers (RetinanetLabeler, RetinanetDetector, DetectionEvaluator, ImageBlobBuilder) the C entry is called through
K.lib() with arena views, as test_gpu_soft_nms.raw_soft_nms does.  After the launch: guards intact, inputs
bit-identical, outputs written -- or left untouched -- exactly as include/ssad_kernels.h says (rows past a count are
excused in check() and then asserted through Arena.untouched() to hold the sentinel word for word), the existing
reference reproduced at the existing test's bar, and bit equality with the same call on ordinary allocations, whose
workspace is filled with another byte: no scratch word is read before it is written.
Every comparison introduced here is an equality; the tolerances are the named ones of test_anchor_labels.py,
test_gpu_soft_nms.py, test_gpu_coco_eval.py, test_gpu_image_blobs.py and test_gpu_kernels.py.

Part B -- what a bad value may reach: a NaN inside one image's ground truth, NaN / +Inf scores and box deltas, a NaN
box in one Soft-NMS segment, a NaN score in one evaluation cell.  Every planted value is data the kernels are
documented to accept.  NOT asserted: a NaN delta of a candidate (fminf and np.minimum differ on it, and the reference
leaves it unspecified: DESIGN.md, "Kernel isolation").
"""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import anchors as OA  # noqa: E402
from oracle import detect as OD  # noqa: E402
from oracle import oracle  # noqa: E402
from guarded import SENTINEL  # noqa: E402
from test_gpu_isolation import Plain, Guarded, isolated, bits, randn  # noqa: E402,F401
from test_gpu_kernels import CONV_FLOOR, CONV_RTOL, DX_FLOOR, DX_RTOL, LOSS_RTOL, close  # noqa: E402
from test_anchor_labels import DETECT_BOX_TOL, TARGET_TOL, _detect_inputs, rand_gts  # noqa: E402
from test_gpu_soft_nms import GAUSS_TOL, METHODS, SCORING, VOTE_TOL  # noqa: E402
from test_gpu_coco_eval import PR_TOL  # noqa: E402
from test_gpu_image_blobs import NORMS, assert_within_bound, restate  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ssad_amd import kernels
    kernels.lib()  # raises if the HIP extension is missing: no fallback
    return kernels


def p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def arena_run(K, monkeypatch, fn, modified=(), nan_ok=None):
    """test_gpu_isolation.isolated, returning the arena as well (for Arena.untouched)"""
    seen = {}

    def both(al):
        if isinstance(al, Guarded):
            seen["arena"] = al.arena
        return fn(al)

    got = isolated(K, monkeypatch, both, modified=modified, nan_ok=nan_ok)
    return got, seen["arena"]


def past(count, rows, width=4):
    """nan_ok mask of a [rows][width] list whose contract is: rows from `count` on are not written"""
    m = np.zeros((rows, width), bool)
    m[count:] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------
# Part A: anchor labelling
# ---------------------------------------------------------------------------------------------------------------------

N_IM, GMAX, BLOB_H, BLOB_W, LEVELS, NA = 3, 6, 96, 128, 5, 9
COUNTS = [4, 0, 6]
CAP_GENEROUS, CAP_SMALL = 256, 3


def gt_arrays(gts, counts):
    boxes, classes = np.zeros((N_IM, GMAX, 4), np.float32), np.zeros((N_IM, GMAX), np.int32)
    for i, (b, c) in enumerate(gts):
        boxes[i, :counts[i]], classes[i, :counts[i]] = b[:counts[i]], c[:counts[i]]
    return boxes, classes


@pytest.fixture(scope="module")
def lab():
    """ground truth, geometry and the oracle's blobs, computed once; nothing changes them"""
    import ssad_amd  # noqa: F401
    from ssad_amd.modeling.generate_anchors import AnchorConfig as cfg, cell_anchors, field_sizes
    rng = np.random.default_rng(9100)
    gts = [rand_gts(rng, max(c, 1), BLOB_H, BLOB_W) for c in COUNTS]
    boxes, classes = gt_arrays(gts, COUNTS)
    live = [i for i, c in enumerate(COUNTS) if c]
    ref = OA.retinanet_blobs([gts[i][0] for i in live], [gts[i][1] for i in live], BLOB_H, BLOB_W)
    fs = field_sizes(cfg)
    T = NA * sum(f * f for f in fs)
    # bg_num: float64 sum over the images, rounded once (anchor_labels.hip's finalize).  One image's term is below
    # 2^24, so the oracle's float32 holds it exactly; an image without ground truth is all background.
    singles = [OA.retinanet_blobs([gts[i][0]], [gts[i][1]], BLOB_H, BLOB_W) for i in live]
    assert all(float(s["bg_num"]) < 2.0 ** 24 for s in singles) and (T + 1.0) * 80 < 2.0 ** 24
    bg = np.float32(sum(float(s["bg_num"]) for s in singles) + (T + 1.0) * 80 * COUNTS.count(0))
    m = [ref["locs_fpn%d" % (3 + l)].shape[0] for l in range(LEVELS)]
    assert max(m) < CAP_GENEROUS and max(m) > CAP_SMALL and 0 < min(x for x in m if x) <= CAP_SMALL and 0 in m, m
    return dict(boxes=boxes, classes=classes, counts=np.array(COUNTS, np.int32), live=live, ref=ref, fs=fs, T=T,
                h=[int(BLOB_H / float(2 ** l)) for l in range(3, 8)], w=[int(BLOB_W / float(2 ** l)) for l in range(3, 8)],
                cells=np.ascontiguousarray(np.asarray(cell_anchors(cfg), np.float64)), m=m,
                fg_bg=np.array([ref["fg_num"], bg], np.float32))


def label_fn(K, lab, boxes, classes, counts, capacity):
    L = K.lib()
    L.ssad_retinanet_anchor_labels_workspace_bytes.restype = C.c_size_t
    IntArr, PtrArr = C.c_int * LEVELS, C.c_void_p * LEVELS
    fs, h, w = IntArr(*lab["fs"]), IntArr(*lab["h"]), IntArr(*lab["w"])
    nb = int(L.ssad_retinanet_anchor_labels_workspace_bytes(LEVELS, NA, 3, fs, N_IM, GMAX))
    assert nb > 0

    def fn(al):
        cells = al.inp("cells", lab["cells"])
        gb, gc, gn = al.inp("gt_boxes", boxes), al.inp("gt_classes", classes), al.inp("gt_counts", counts)
        labels = [al.out("labels%d" % l, (N_IM, NA, lab["h"][l], lab["w"][l]), I32) for l in range(LEVELS)]
        locs = [al.out("locs%d" % l, (capacity, 4)) for l in range(LEVELS)]
        targets = [al.out("targets%d" % l, (capacity, 4)) for l in range(LEVELS)]
        counts_out, fg_bg = al.out("counts_out", (LEVELS,), I32), al.out("fg_bg", (2,))
        ws = al.ws(nb, "anchor_labels")
        assert ws.numel() == nb
        rc = L.ssad_retinanet_anchor_labels(
            p(cells), LEVELS, NA, 3, fs, h, w, p(gb), p(gc), p(gn), N_IM, GMAX, 81, C.c_float(0.5), C.c_float(0.4),
            PtrArr(*[t.data_ptr() for t in labels]), PtrArr(*[t.data_ptr() for t in locs]),
            PtrArr(*[t.data_ptr() for t in targets]), capacity, p(counts_out), p(fg_bg), p(ws), C.c_size_t(nb),
            K._stream())
        assert rc == 0, rc
        m = counts_out.cpu().numpy()
        res = dict(counts=counts_out, fg_bg=fg_bg)
        for l in range(LEVELS):
            k = min(int(m[l]), capacity)
            res["labels%d" % l], res["locs%d" % l], res["targets%d" % l] = labels[l], locs[l][:k], targets[l][:k]
        return res

    return fn


def label_run(K, monkeypatch, lab, boxes, classes, capacity):
    """the launch in the arena with every check of Part A that needs no reference; returns the outputs"""
    written = [min(m, capacity) for m in lab["m"]]
    nan_ok = {}
    for l in range(LEVELS):
        nan_ok["locs%d" % l] = nan_ok["targets%d" % l] = past(written[l], capacity)
    got, arena = arena_run(K, monkeypatch, label_fn(K, lab, boxes, classes, lab["counts"], capacity), nan_ok=nan_ok)
    assert list(got["counts"]) == lab["m"], "counts_out reports the true M, whatever the capacity"
    for l in range(LEVELS):
        for name in ("locs%d" % l, "targets%d" % l):
            u = arena.untouched(name)
            assert u[written[l]:].all(), "%s: a row past min(M, capacity) was written" % name
            assert not u[:written[l]].any(), "%s: a row below the count was left unwritten" % name
    return got


_CLEAN = {}


def clean_labels(K, monkeypatch, lab):
    """run (a), shared by the three cases"""
    if "a" not in _CLEAN:
        _CLEAN["a"] = label_run(K, monkeypatch, lab, lab["boxes"], lab["classes"], CAP_GENEROUS)
    return _CLEAN["a"]


def test_guarded_anchor_labels_generous_capacity(K, monkeypatch, lab):
    """run (a): labels, fg lists, targets and fg / bg numbers against oracle.anchors.retinanet_blobs; list rows from
    counts_out[l] on are untouched.  Level 7 of a 96 x 128 blob has an empty label map (h = 0)."""
    got, ref, live = clean_labels(K, monkeypatch, lab), lab["ref"], lab["live"]
    for l in range(LEVELS):
        lv = got["labels%d" % l]
        assert lv.shape == (N_IM, NA, lab["h"][l], lab["w"][l])
        assert np.array_equal(lv[live], ref["labels_fpn%d" % (3 + l)]), "labels level %d" % l
        assert not lv[1].any(), "an image without ground truth is all background"
        locs = got["locs%d" % l].copy()
        assert not (locs[:, 0] == 1).any()
        locs[:, 0] = np.where(locs[:, 0] == 2, 1, locs[:, 0])          # the oracle saw two images
        assert np.array_equal(locs, ref["locs_fpn%d" % (3 + l)]), "fg list level %d" % l
        np.testing.assert_allclose(got["targets%d" % l], ref["targets_fpn%d" % (3 + l)], **TARGET_TOL)
    assert same(got["fg_bg"], lab["fg_bg"]), (got["fg_bg"], lab["fg_bg"])


def test_guarded_anchor_labels_capacity_overflow_is_reported_not_written(K, monkeypatch, lab):
    """run (b): capacity 3 is below two levels' counts.  counts_out still reports M, rows 0..2 are run (a)'s, and
    nothing is written behind them (the guards after the 48-byte lists are intact): al_scatter's pos >= capacity."""
    a = clean_labels(K, monkeypatch, lab)
    b = label_run(K, monkeypatch, lab, lab["boxes"], lab["classes"], CAP_SMALL)
    assert sum(m > CAP_SMALL for m in lab["m"]) >= 2
    for l in range(LEVELS):
        k = min(lab["m"][l], CAP_SMALL)
        assert b["locs%d" % l].shape == (k, 4)
        assert same(b["locs%d" % l], a["locs%d" % l][:k]) and same(b["targets%d" % l], a["targets%d" % l][:k]), l
        assert same(b["labels%d" % l], a["labels%d" % l])
    assert same(b["fg_bg"], a["fg_bg"])


@pytest.mark.parametrize("junk", ["nan", "decoy"])
def test_guarded_anchor_labels_honour_gt_counts(K, monkeypatch, lab, junk):
    """run (c): every slot at and beyond gt_counts[n] (the whole row of the image without ground truth) holds class 127
    and a NaN box -- or, second case, a box that would claim anchors of its own if it were read: a NaN IoU loses every
    comparison, so NaN slots alone would not show a loop that runs to Gmax.  Every output is bit-identical to run (a):
    gt_counts alone makes a slot live, in the IoU pass, the assignment and the target kernel's read through a_arg."""
    a = clean_labels(K, monkeypatch, lab)
    boxes, classes = lab["boxes"].copy(), lab["classes"].copy()
    decoy = np.array([[8, 8, 71, 55], [40, 20, 119, 90]], np.float32)
    for i, c in enumerate(COUNTS):
        boxes[i, c:] = np.nan if junk == "nan" else decoy[np.arange(GMAX - c) % 2]
        classes[i, c:] = 127
    if junk == "nan":
        assert np.isnan(boxes[1]).all() and np.isnan(boxes).sum() == 4 * (N_IM * GMAX - sum(COUNTS))
    else:
        # the decoys are boxes the labelling would use: as image 1's ground truth they claim foreground anchors
        claimed = OA.retinanet_blobs([decoy], [np.array([5, 6], np.int32)], BLOB_H, BLOB_W)
        assert float(claimed["fg_num"]) > 0
    c = label_run(K, monkeypatch, lab, boxes, classes, CAP_GENEROUS)
    assert sorted(c) == sorted(a)
    for k in a:
        assert same(c[k], a[k]), "%s depends on ground-truth slots behind gt_counts" % k


# ---------------------------------------------------------------------------------------------------------------------
# Part A: detection
# ---------------------------------------------------------------------------------------------------------------------

DET_SHAPES = [(5, 7), (3, 4), (2, 3)]
DET_A, DET_C, TOPN, KEEP = 9, 80, 50, 150
IM_H, IM_W, IM_SCALE = 150, 210, 0.9375
XFORM_CLIP = float(np.log(1000. / 16.))
# one shift per level (test_anchor_labels._detect_inputs: scores are k * 2^-shift, k = 1 ... 720 h w, each once):
# 25 200 scores up to 0.096 on the finest level, 12 093 of them above the 0.05 threshold: topn = 50 cuts inside;
# 8 640 scores up to 0.0502 on the middle level, 41 above the threshold: fewer than topn;
# threshold 0 on the coarsest: all 4 320 are candidates.
DET_SHIFTS = (18, 17.392, 18)


def det_inputs():
    rng = np.random.default_rng(9200)
    probs, deltas = [], []
    for shape, shift in zip(DET_SHAPES, DET_SHIFTS):
        pr, de = _detect_inputs(rng, [shape], shift)
        probs, deltas = probs + pr, deltas + de
    n = [int((pr > (0.05 if l < 2 else 0.0)).sum()) for l, pr in enumerate(probs)]
    assert n[0] > TOPN and 0 < n[1] < TOPN and n[2] == probs[2].size, n
    return probs, deltas


def det_cells():
    import ssad_amd  # noqa: F401
    from ssad_amd.modeling.generate_anchors import AnchorConfig as cfg, cell_anchors
    device = np.ascontiguousarray(np.asarray(cell_anchors(cfg), np.float64)[:len(DET_SHAPES)])
    host = np.array([[OA.generate_cell64(l, a) for a in range(DET_A)] for l in range(3, 3 + len(DET_SHAPES))])
    return device, host


def det_oracle(probs, deltas):
    return OD.im_detect_bbox(probs, deltas, det_cells()[1], (IM_H, IM_W), IM_SCALE, pre_nms_topn=TOPN, dets_per_im=KEEP)


def det_post(soft, vote):
    from ssad_amd.roi_data.retinanet import RetinanetDetector
    return RetinanetDetector._post(soft, vote)


def det_fn(K, probs, deltas, post):
    """both calls of a configuration on one workspace, refilled with the sentinel in between"""
    L = K.lib()
    L.ssad_retinanet_detect_workspace_bytes.restype = C.c_size_t
    n = len(DET_SHAPES)
    IntArr, PtrArr = C.c_int * n, C.c_void_p * n
    H, W = IntArr(*[h for h, _ in DET_SHAPES]), IntArr(*[w for _, w in DET_SHAPES])
    if post is None:
        nb = int(L.ssad_retinanet_detect_workspace_bytes(n, DET_A, DET_C, H, W, TOPN))
    else:
        nb = int(L.ssad_retinanet_detect_ex_workspace_bytes(n, DET_A, DET_C, H, W, TOPN, C.byref(post)))
    assert nb > 0 and nb % 4 == 0
    cells = det_cells()[0]

    def fn(al):
        dc = al.inp("cells", cells)
        tp = [al.inp("prob%d" % l, a) for l, a in enumerate(probs)]
        td = [al.inp("delta%d" % l, a) for l, a in enumerate(deltas)]
        ws = al.ws(nb, "detect")
        assert ws.numel() == nb
        res = {}
        for call in (1, 2):
            out, count = al.out("dets%d" % call, (KEEP, 6)), al.out("count%d" % call, (1,), I32)
            if call == 2:
                ws.view(I32).fill_(SENTINEL)
            args = (PtrArr(*[t.data_ptr() for t in tp]), PtrArr(*[t.data_ptr() for t in td]), p(dc), n, DET_A, DET_C, 3,
                    H, W, C.c_float(0.05), TOPN, C.c_float(0.5), KEEP, C.c_float(IM_SCALE), IM_H, IM_W,
                    C.c_float(XFORM_CLIP), p(out), p(count), p(ws), C.c_size_t(nb), K._stream())
            rc = L.ssad_retinanet_detect(*args) if post is None else L.ssad_retinanet_detect_ex(*args, C.byref(post))
            assert rc == 0, rc
            res["dets%d" % call], res["count%d" % call] = out, count
        return res

    return fn


def det_run(K, monkeypatch, probs, deltas, post):
    """Part A's checks that need no reference: all 150 rows written, zeros from `count` on, the second call (on a
    workspace refilled with the sentinel) bit-equal to the first.  Returns the rows."""
    got, _ = arena_run(K, monkeypatch, det_fn(K, probs, deltas, post))
    count = int(got["count1"][0])
    assert 0 < count <= KEEP
    assert not got["dets1"].view(np.int32)[count:].any(), "rows from count on are +0.0"
    assert same(got["dets2"], got["dets1"]) and same(got["count2"], got["count1"]), \
        "a second call on the same workspace gives other bytes: a scratch word is read before it is written"
    return got["dets1"][:count]


def assert_detections(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(got[:, 4], ref[:, 4])                # scores, in order
    assert np.array_equal(got[:, 5], ref[:, 5])                # classes
    np.testing.assert_allclose(got[:, :4], ref[:, :4], **DETECT_BOX_TOL)


def test_guarded_detect_greedy(K, monkeypatch):
    probs, deltas = det_inputs()
    ref = det_oracle(probs, deltas)
    assert 0 < ref.shape[0] < KEEP
    assert_detections(det_run(K, monkeypatch, probs, deltas, None), ref)


def composition(soft, vote):
    """test_gpu_soft_nms.test_detector_options_equal_the_per_class_composition's reference: utils.boxes per class on the
    detector's own candidates (ordinary allocations), sorted by final score, class, position"""
    import ssad_amd  # noqa: F401
    from ssad_amd.roi_data.retinanet import RetinanetDetector
    from ssad_amd.utils import boxes as B
    probs, deltas = det_inputs()
    det = RetinanetDetector(DET_SHAPES, pre_nms_topn=TOPN, nms_thresh=2.0, dets_per_im=KEEP)
    cands = det([dev(a) for a in probs], [dev(a) for a in deltas], IM_H, IM_W, IM_SCALE).clone()
    assert cands.shape[0] > TOPN
    rows = []
    for c in torch.unique(cands[:, 5]).cpu().numpy():
        dets_c = cands[cands[:, 5] == float(c)][:, :5].contiguous()
        opts = dict(sigma=0.5, score_thresh=0.0001, method="linear")
        opts.update(soft)
        top, keep = B.soft_nms(dets_c, overlap_thresh=0.5, **opts)
        top = B.box_voting(top.contiguous(), dets_c, vote["vote_th"], vote.get("scoring_method", "ID"), vote.get("beta", 1.0))
        top, keep = top.cpu().numpy(), keep.cpu().numpy()
        rows += [(-float(top[i, 4]), float(c), int(keep[i]), top[i]) for i in range(len(keep))]
    rows.sort(key=lambda r: r[:3])
    return np.array([list(r[3]) + [r[1]] for r in rows[:KEEP]], np.float32)


@pytest.mark.parametrize("soft,vote", [
    (dict(method="linear"), dict(vote_th=0.8, scoring_method="AVG")),
    (dict(method="gaussian", sigma=0.5), dict(vote_th=0.8, scoring_method="ID")),
], ids=["linear_AVG", "gaussian_ID"])
def test_guarded_detect_ex(K, monkeypatch, soft, vote):
    probs, deltas = det_inputs()
    want = composition(soft, vote)
    got = det_run(K, monkeypatch, probs, deltas, det_post(soft, vote))
    assert got.shape == want.shape and np.array_equal(got[:, 5], want[:, 5])
    if soft["method"] != "gaussian":
        assert got.tobytes() == want.tobytes()
    else:                                              # the existing test's bar for gaussian decays
        np.testing.assert_allclose(got[:, 4], want[:, 4], rtol=GAUSS_TOL, atol=0)
        np.testing.assert_allclose(got[:, :4], want[:, :4], rtol=GAUSS_TOL, atol=GAUSS_TOL * IM_W)


# ---------------------------------------------------------------------------------------------------------------------
# Part A: Soft-NMS and voting entries alone
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def zs():
    return np.load(os.path.join(HERE, "golden", "soft_nms_ref.npz"))


def soft_fn(K, dets, cls, classes, method, sigma, nt, thresh):
    L = K.lib()
    n = dets.shape[0]
    nb = int(L.ssad_soft_nms_workspace_bytes(n))

    def fn(al):
        boxes, scores = al.inp("boxes", dets[:, :4]), al.inp("scores", dets[:, 4])
        dcls = al.inp("cls", cls.astype(np.int32))
        keys, rank = al.out("keys", (n,), I64), al.out("rank", (n,), I32)
        ws = al.ws(nb, "soft_nms")
        assert ws.numel() == nb
        rc = L.ssad_soft_nms(p(boxes), p(scores), p(dcls), n, classes, method, sigma, nt, thresh, p(keys), p(rank), p(ws),
                             nb, K._stream())
        assert rc == 0, rc
        return dict(keys=keys, rank=rank)

    return fn


@pytest.mark.parametrize("name", ["linear", "hard"])
def test_guarded_soft_nms_segments(K, monkeypatch, zs, name):
    """the detector's layout (ms_*): six classes of which 0, 3 and 5 are empty, -1 in the last four slots; keys_out and
    pick_rank_out are written completely (0 / -1 for retired candidates and empty slots)"""
    dets, cls = zs["ms_dets"], zs["ms_cls"]
    got, _ = arena_run(K, monkeypatch, soft_fn(K, dets, cls, int(zs["ms_classes"]), K.NMS_METHODS[name], 0.5, 0.3, 0.001))
    keys, rank = got["keys"], got["rank"]
    want_rank, want_score = zs["ms_rank_" + name], zs["ms_score_" + name]
    pos = np.arange(len(cls), dtype=np.int64)
    assert np.array_equal(rank, want_rank)
    live = want_rank >= 0
    assert live.any() and (~live).any() and np.all(keys[~live] == 0)
    assert np.array_equal((keys[live] >> 32).astype(np.int32).view(np.float32), want_score[live])
    assert np.array_equal(keys[live] & 0xffffffff, ~pos[live] & 0xffffffff)


@pytest.mark.parametrize("size", [1024, 1025], ids=["lds_1024", "workspace_1025"])
def test_guarded_soft_nms_both_sides_of_the_lds_cap(K, monkeypatch, zs, size):
    """one class of SSAD_SOFT_NMS_LDS_CAP candidates (LDS) and of one more (current scores in the workspace), linear:
    the fixture's picks and scores bit for bit, as test_linear_and_hard_reproduce_the_reference_bit_for_bit"""
    assert int(zs["lds_cap"]) == 1024
    v = next(v for v in range(len(zs["soft_method"])) if METHODS[int(zs["soft_method"][v])] == "linear" and
             zs["soft_dets_%d" % int(zs["soft_data"][v])].shape[0] == size)
    dets = zs["soft_dets_%d" % int(zs["soft_data"][v])]
    got, _ = arena_run(K, monkeypatch, soft_fn(K, dets, np.zeros(size, np.int32), 1, K.NMS_METHODS["linear"],
                                               float(zs["soft_sigma"][v]), float(zs["soft_nt"][v]),
                                               float(zs["soft_thresh"][v])))
    keys, rank = got["keys"], got["rank"]
    picked = np.flatnonzero(rank >= 0)
    keep = picked[np.argsort(rank[picked])]
    assert np.array_equal(np.sort(rank[picked]), np.arange(len(picked))) and np.all(keys[rank < 0] == 0)
    assert np.array_equal(keep, zs["soft_keep_%d" % v])
    assert (keys[keep] >> 32).astype(np.int32).view(np.float32).tobytes() == zs["soft_scores_%d" % v].tobytes()
    assert np.array_equal(keys[keep] & 0xffffffff, ~keep.astype(np.int64) & 0xffffffff)


@pytest.mark.parametrize("scoring", ["AVG", "IOU_AVG"])
def test_guarded_box_voting(K, monkeypatch, zs, scoring):
    """the fixture's largest voting case (358 tops, 400 voters); every fifth top is handed over as retired
    (keys == 0) and every seventh as an empty slot (top_cls < 0): their rows of voted_boxes_out and their keys are
    not written, the others meet the fixture at test_box_voting_matches_the_reference's bar"""
    k = next(k for k in range(len(zs["vote_all"])) if int(zs["vote_all"][k]) == 2 and int(zs["vote_top"][k]) == 4 and
             SCORING[int(zs["vote_scoring"][k])] == scoring)
    alld, top, want = zs["vote_all_2"], zs["vote_top_4"], zs["vote_out_%d" % k]
    m, n = top.shape[0], alld.shape[0]
    pos = np.arange(m, dtype=np.int64)
    keys0 = ((top[:, 4].copy().view(np.int32).astype(np.int64) & 0xffffffff) << 32) | (~pos & 0xffffffff)
    top_cls = np.zeros(m, np.int32)
    keys0[::5] = 0
    top_cls[::7] = -1
    skipped = (keys0 == 0) | (top_cls < 0)
    assert skipped.sum() > m // 4 and (~skipped).sum() > m // 2
    L = K.lib()

    def fn(al):
        tb, tc = al.inp("top_boxes", top[:, :4]), al.inp("top_cls", top_cls)
        boxes, scores, cls = al.inp("boxes", alld[:, :4]), al.inp("scores", alld[:, 4]), al.inp("cls", np.zeros(n, np.int32))
        keys, voted = al.inp("keys", keys0), al.out("voted", (m, 4))
        rc = L.ssad_box_voting(p(tb), p(tc), m, p(boxes), p(scores), p(cls), n, 1, float(zs["vote_thresh"][k]),
                               K.VOTE_SCORING[scoring], float(zs["vote_beta"][k]), p(keys), p(voted), K._stream())
        assert rc == 0, rc
        return dict(keys=keys, voted=voted[dev(np.flatnonzero(~skipped))])

    got, arena = arena_run(K, monkeypatch, fn, modified=("keys",), nan_ok={"voted": np.repeat(skipped[:, None], 4, 1)})
    u = arena.untouched("voted")
    assert u[skipped].all() and not u[~skipped].any()
    assert np.array_equal(got["keys"][skipped], keys0[skipped])
    assert np.array_equal(got["keys"][~skipped] & 0xffffffff, keys0[~skipped] & 0xffffffff)
    big = float(np.abs(alld[:, :4]).max())
    w = want[~skipped]
    err = np.abs(got["voted"].astype(np.float64) - w[:, :4])
    assert np.all(err <= VOTE_TOL * np.abs(w[:, :4]) + VOTE_TOL * big), float(err.max())
    score = (got["keys"][~skipped] >> 32).astype(np.int32).view(np.float32).astype(np.float64)
    assert (np.abs(score - w[:, 4]) / np.abs(w[:, 4])).max() <= VOTE_TOL


# ---------------------------------------------------------------------------------------------------------------------
# Part A: evaluation
# ---------------------------------------------------------------------------------------------------------------------

EVAL_CAP = 160


@pytest.fixture(scope="module")
def ze():
    return np.load(os.path.join(HERE, "golden", "coco_eval_ref.npz"))


def evaluator(z, relax):
    """the product's host half (argument checks, ground truth sorted by cell); its device buffers are not used"""
    import ssad_amd  # noqa: F401
    from ssad_amd.datasets import DetectionEvaluator
    return DetectionEvaluator(int(z["num_images"]), int(z["num_categories"]), z["gt_boxes"], z["gt_area"], z["gt_iscrowd"],
                              z["gt_image"], z["gt_category"], iou_thrs=z["iou_thrs"], rec_thrs=z["rec_thrs"],
                              max_dets=tuple(int(m) for m in z["max_dets"]), area_rng=z["area_rng"],
                              small_box_relax=relax, max_dets_per_image=EVAL_CAP)


def host_ranks(cat, score, max_det):
    """det_rank as the header defines it: per (image, category) by score descending, equal scores (and NaNs, last) in
    slot order, cut at max_det; -1 for cut and empty slots"""
    rank = np.full(cat.shape, -1, np.int32)
    for i in range(cat.shape[0]):
        for k in np.unique(cat[i][cat[i] >= 0]):
            slots = np.flatnonzero(cat[i] == k)
            s = score[i, slots]
            order = slots[np.lexsort((slots, -np.where(np.isnan(s), -np.inf, s), np.isnan(s)))]
            rank[i, order[:max_det]] = np.arange(min(len(order), max_det))
    return rank


def eval_inputs(z):
    I = int(z["num_images"])
    per = []
    for img in range(I):
        sel = z["det_image"] == img
        per.append((z["det_boxes"][sel], z["det_scores"][sel], z["det_category"][sel].astype(np.int32)))
    cat, score = np.full((I, EVAL_CAP), -1, np.int32), np.zeros((I, EVAL_CAP), np.float64)
    for img, (b, s, c) in enumerate(per):
        cat[img, :len(c)], score[img, :len(s)] = c, s.astype(np.float64)
    return per, cat, score


@pytest.mark.parametrize("mode,relax", [("strict", False), ("relax", True)])
def test_guarded_coco_eval(K, monkeypatch, ze, mode, relax):
    """add (every image has n < cap, one has none) -> match -> accumulate on arena views"""
    z, ev = ze, evaluator(ze, relax)
    DK = ev._DK
    I, Kc, cap, A, T, M, R, G = ev.I, ev.K, ev.cap, ev.A, ev.T, ev.M, ev.R, ev.G
    AT = A * T
    per, cat, score = eval_inputs(z)
    n_of = np.array([len(s) for _, s, _ in per])
    assert n_of.max() < cap and n_of.min() == 0 and n_of.max() > ev.max_dets[-1]
    rank = host_ranks(cat, score, ev.max_dets[-1])
    assert (rank[cat >= 0] < 0).any(), "a cell is cut at max_det"
    empty = np.arange(cap)[None, :] >= n_of[:, None]                       # slots n ... cap-1
    nb_match, nb_acc = DK.coco_eval_match_workspace_bytes(G, A, T), DK.coco_eval_accumulate_workspace_bytes(Kc, A)
    assert G * AT <= nb_match < G * AT + 512, "the match workspace is the G.A.T matched flags (+ alignment)"
    host = lambda t: t.cpu().numpy()

    def fn(al):
        gt_xywh, gt_area = al.inp("gt_xywh", host(ev.gt_xywh)), al.inp("gt_area", host(ev.gt_area))
        gt_crowd, gt_off = al.inp("gt_crowd", host(ev.gt_crowd)), al.inp("gt_off", host(ev.gt_off))
        iou, rec, rng = al.inp("iou_thrs", host(ev.d_iou)), al.inp("rec_thrs", host(ev.d_rec)), al.inp("area_rng", host(ev.d_rng))
        max_dets, bad = al.inp("max_dets", host(ev.d_max_dets)), al.inp("bad_count", np.zeros(1, np.int32))
        det_xywh, det_score = al.out("det_xywh", (I, cap, 4), F64), al.out("det_score", (I, cap), F64)
        det_cat = al.out("det_cat", (I, cap), I32)
        for img, (b, s, c) in enumerate(per):
            n = len(s)
            tb, ts, tc = (al.inp("%s%d" % (nm, img), a) if n else None for nm, a in (("boxes", b), ("scores", s), ("cats", c)))
            DK.coco_eval_add(tb, 4, ts, 1, None, 0, tc, n, cap, Kc, img, det_xywh, det_score, det_cat, bad)
        det_rank, dt_match = al.out("det_rank", (I, cap), I32), al.out("dt_match", (I, cap, AT), I32)
        dt_ignore = al.out("dt_ignore", (I, cap, AT), U8)
        cell_npig, cell_eval = al.out("cell_npig", (I * Kc, A), I32), al.out("cell_eval", (I * Kc,), U8)
        ws = al.ws(nb_match, "coco_match")
        assert ws.numel() == nb_match
        DK.coco_eval_match(I, Kc, cap, det_xywh, det_score, det_cat, gt_xywh, gt_area, gt_crowd, gt_off, G, iou, T, rng, A,
                           ev.max_dets[-1], relax, det_rank, dt_match, dt_ignore, cell_npig, cell_eval, ws)
        # the one global ordering between the kernels, as DetectionEvaluator.evaluate builds it (torch.sort: plumbing)
        rk = det_rank.to(I64).view(-1)
        live = rk >= 0
        slot = torch.arange(I * cap, device="cuda", dtype=I64)
        first = torch.where(live, (slot // cap) * cap + rk, torch.full_like(slot, I * cap))
        perm = torch.sort(first, stable=True)[1]
        perm = perm[torch.sort(-det_score.view(-1)[perm], stable=True)[1]]
        key = torch.where(live, det_cat.view(-1).to(I64), torch.full_like(slot, Kc))[perm]
        key, idx = torch.sort(key, stable=True)
        seg = torch.searchsorted(key, torch.arange(Kc + 1, device="cuda", dtype=I64))
        perm, seg = al.inp("perm", host(perm[idx])), al.inp("seg", host(seg))
        precision, scores = al.out("precision", (T, R, Kc, A, M), F64), al.out("scores", (T, R, Kc, A, M), F64)
        recall = al.out("recall", (T, Kc, A, M), F64)
        wa = al.ws(nb_acc, "coco_accumulate")
        assert wa.numel() == nb_acc
        DK.coco_eval_accumulate(I, Kc, cap, A, T, M, R, max_dets, perm, seg, det_score, det_rank, dt_match, dt_ignore,
                                cell_npig, cell_eval, rec, precision, scores, recall, wa)
        ranked, filled = dev(np.flatnonzero(rank.reshape(-1) >= 0)), dev(np.flatnonzero(~empty.reshape(-1)))
        kept.update(det_rank=det_rank.view(-1), dt_match=dt_match, dt_ignore=dt_ignore, cell_npig=cell_npig,
                    cell_eval=cell_eval, det_cat=det_cat)
        return dict(det_cat=det_cat, det_rank=det_rank, cell_npig=cell_npig, cell_eval=cell_eval, precision=precision,
                    scores=scores, recall=recall, dt_match=dt_match.view(-1, AT)[ranked],
                    dt_ignore=dt_ignore.view(-1, AT)[ranked], det_xywh=det_xywh.view(-1, 4)[filled],
                    det_score=det_score.view(-1)[filled])

    kept = {}                      # the arena run's views, regrouped below by the product's own _matches
    unranked = rank < 0
    got, arena = arena_run(K, monkeypatch, fn, nan_ok={
        "det_xywh": np.repeat(empty[:, :, None], 4, 2), "det_score": empty,
        "dt_match": np.repeat(unranked[:, :, None], AT, 2)})
    # add: slots n ... cap-1 get category -1, their boxes and scores stay untouched
    assert np.array_equal(got["det_cat"], cat)
    assert arena.untouched("det_xywh")[empty].all() and not arena.untouched("det_xywh")[~empty].any()
    assert arena.untouched("det_score")[empty].all() and not arena.untouched("det_score")[~empty].any()
    # match: det_rank written completely; dt_match / dt_ignore exactly where det_rank >= 0
    assert np.array_equal(got["det_rank"], rank)
    u = arena.untouched("dt_match")
    assert u[unranked].all() and not u[~unranked].any()
    ub = arena.untouched("dt_ignore").reshape(I, cap, AT // 4)
    assert AT % 4 == 0 and ub[unranked].all() and not ub[~unranked].any()
    assert set(np.unique(got["dt_ignore"])) <= {0, 1} and set(np.unique(got["cell_eval"])) <= {0, 1}
    # the fixture, as test_gpu_coco_eval.py asserts it
    ev.det_cat = kept.pop("det_cat")
    m = ev._matches(kept)
    assert np.array_equal(m["cell"], z["m_cell"]) and np.array_equal(m["offsets"], z["m_off"])
    assert np.array_equal(m["npig"], z["m_npig"])
    assert np.array_equal(m["dt_match"], z[mode + "_dtm"]) and np.array_equal(m["dt_ignore"], z[mode + "_dtig"])
    for name in ("precision", "recall"):
        g, want = got[name], z["%s_%s" % (mode, name)]
        assert g.dtype == np.float64 and g.shape == want.shape and np.array_equal(g == -1, want == -1)
        assert float(np.abs(g - want).max()) <= PR_TOL
    assert got["scores"].tobytes() == z[mode + "_scores"].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# Part A: image blobs
# ---------------------------------------------------------------------------------------------------------------------

def test_guarded_image_blobs(K, monkeypatch):
    """two uint8 sources packed back to back (src_bytes exact), one flipped, scales 1.0 and 1.7, two norms: both
    blobs written completely by the kernel itself (padding +0.0 included: nothing pre-fills them), src frozen"""
    rng = np.random.default_rng(9300)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((5, 7), (9, 4))]
    flipped, scales, blob_hw = [0, 1], [1.0, 1.7], (16, 16)
    out_hw = [(int(np.rint(im.shape[0] * s)), int(np.rint(im.shape[1] * s))) for im, s in zip(images, scales)]
    assert out_hw == [(5, 7), (15, 7)]
    N, (Hb, Wb) = 2, blob_hw
    packed = np.concatenate([im.reshape(-1) for im in images])
    offsets = [0, images[0].size]
    L = K.lib()
    nb = int(L.ssad_image_blobs_workspace_bytes(N, Hb, Wb))
    assert nb > 0
    ints = lambda v: (C.c_int * N)(*[int(x) for x in v])

    def fn(al):
        src = al.inp("src", packed)
        outs = [al.out("blob%d" % k, (N, 3, Hb, Wb)) for k in range(len(NORMS))]
        tab = (K.ImageNorm * len(NORMS))()
        for k, ((div, mean, std), o) in enumerate(zip(NORMS, outs)):
            tab[k] = K.ImageNorm(div, (C.c_float * 3)(*mean), (C.c_float * 3)(*std), o.data_ptr())
        ws = al.ws(nb, "image_blobs")
        assert ws.numel() == nb
        rc = L.ssad_image_blobs(src.data_ptr(), packed.size, (C.c_longlong * N)(*offsets),
                                ints(im.shape[0] for im in images), ints(im.shape[1] for im in images),
                                ints(o[0] for o in out_hw), ints(o[1] for o in out_hw), (C.c_double * N)(*scales),
                                ints(flipped), N, Hb, Wb, tab, len(NORMS), ws.data_ptr(), nb, K._stream())
        assert rc == 0, rc
        return {"blob%d" % k: o for k, o in enumerate(outs)}

    got, _ = arena_run(K, monkeypatch, fn)
    for k, norm in enumerate(NORMS):
        want, inside = restate(images, flipped, scales, out_hw, blob_hw, norm)
        assert (~inside).any() and inside.any()
        assert_within_bound(torch.from_numpy(got["blob%d" % k]), want, inside, norm, "norm %d" % k)


# ---------------------------------------------------------------------------------------------------------------------
# Part A: small fp32 entries
# ---------------------------------------------------------------------------------------------------------------------

def test_guarded_conv1x1_bias_act2(K, monkeypatch):
    """a bottleneck's last layer and its projection shortcut as one product: 64 + 64 -> 128, P = 12"""
    N, C1, C2, M, H, W = 2, 64, 64, 128, 3, 4
    rng = np.random.default_rng(9400)
    X1, X2 = randn(rng, N, C1, H, W), randn(rng, N, C2, H, W)
    Wt, b, R = randn(rng, M, C1 + C2, scale=(C1 + C2) ** -0.5), randn(rng, M), randn(rng, N, M, H, W)
    L = K.lib()

    def fn(al):
        x1, x2, w, bias, r = al.inp("x1", X1), al.inp("x2", X2), al.inp("w", Wt), al.inp("bias", b), al.inp("residual", R)
        y, yr = al.out("y", (N, M, H, W)), al.out("y_residual_linear", (N, M, H, W))
        K._check(L.ssad_conv1x1_bias_act2(p(x1), C1, p(x2), C2, p(w), p(bias), p(None), p(y), N, H * W, M, 1, K._stream()),
                 "conv1x1_bias_act2")
        K._check(L.ssad_conv1x1_bias_act2(p(x1), C1, p(x2), C2, p(w), p(None), p(r), p(yr), N, H * W, M, 0, K._stream()),
                 "conv1x1_bias_act2")
        return dict(y=y, yr=yr)

    got, _ = arena_run(K, monkeypatch, fn)
    X = np.concatenate([X1, X2], 1)
    W4 = Wt.reshape(M, C1 + C2, 1, 1)
    close(got["y"], oracle.relu(oracle.conv_forward(X, W4, b, kernel=1, stride=1, pad=0)), CONV_RTOL, CONV_FLOOR, "relu(Y)")
    close(got["yr"], oracle.conv_forward(X, W4, None, kernel=1, stride=1, pad=0).astype(np.float64) + R, CONV_RTOL,
          CONV_FLOOR, "Y + R")


def test_guarded_select_smooth_l1_single_level(K, monkeypatch):
    """ssad_select_smooth_l1_forward / _backward (the operator's single-level pair)"""
    rng = np.random.default_rng(9500)
    N, A, H, W, M = 2, 2, 5, 7, 9
    pred = randn(rng, N, 4 * A, H, W)
    flat = rng.choice(N * A * H * W, size=M, replace=False)
    n_, a_, y_, x_ = np.unravel_index(flat, (N, A, H, W))
    Lc = np.stack([n_, 4 * a_, y_, x_], 1).astype(np.float32)
    Y, S, dl = randn(rng, M, 4, scale=0.5), np.array([41.0], np.float32), np.array([0.75], np.float32)
    L = K.lib()
    nb = int(L.ssad_select_smooth_l1_workspace_bytes(1))

    def fn(al):
        yh, y, lc, s, dloss = al.inp("Y_hat", pred), al.inp("Y", Y), al.inp("L", Lc), al.inp("S", S), al.inp("dloss", dl)
        loss, ws = al.out("loss", (1,)), al.ws(nb, "smoothl1")
        assert ws.numel() == max(nb, 1)
        K._check(L.ssad_select_smooth_l1_forward(p(yh), p(y), p(lc), p(s), N, 4 * A, H, W, M, 0.11, 0.5, p(loss), p(ws), nb,
                                                 K._stream()), "select_smooth_l1_forward")
        dy = K.select_smooth_l1_backward(yh, y, lc, s, dloss, beta=0.11, scale=0.5, out=al.out("dY_hat", pred.shape))
        return dict(loss=loss, dy=dy)

    got, _ = arena_run(K, monkeypatch, fn)
    _, l64 = oracle.select_smooth_l1_forward(pred, Y, Lc, S, beta=0.11, scale=0.5)
    close(float(got["loss"][0]), l64, LOSS_RTOL, 1e-9, "loss")
    want = oracle.select_smooth_l1_backward(pred, Y, Lc, S, 0.75, beta=0.11, scale=0.5)
    close(got["dy"], want, DX_RTOL, DX_FLOOR, "dY_hat")
    assert np.array_equal(got["dy"] == 0, np.asarray(want) == 0)


@pytest.mark.parametrize("n,skew", [(1, 0), (5, 0), (1023, 0), (1023, 4)])
def test_guarded_fill(K, monkeypatch, n, skew):
    value = -0.0 if skew else 3.25
    L = K.lib()

    def fn(al):
        y = al.out("y", (n,), skew=skew)
        K._check(L.ssad_fill(p(y), value, n, K._stream()), "fill")
        return dict(y=y)

    got, _ = arena_run(K, monkeypatch, fn)
    assert same(got["y"], np.full(n, value, np.float32))


@pytest.mark.parametrize("n,skew", [(5, 0), (1023, 4)])
def test_guarded_check_finite(K, monkeypatch, n, skew):
    """flag |= 1 for an Inf or a NaN among x[0..n); the flag is not cleared.  The guard band right behind x is full
    of the sentinel NaN: reading one element too many sets the flag of the finite case."""
    rng = np.random.default_rng(9600 + n)
    fin = randn(rng, n)
    fin[-1] = np.float32(3.0e38)                          # large and finite
    inf, nan = fin.copy(), fin.copy()
    inf[n // 2], nan[-1] = np.inf, np.nan
    L = K.lib()

    def fn(al):
        res = {}
        for name, x, start in (("finite", fin, 0), ("kept", fin, 4), ("inf", inf, 0), ("nan_or", nan, 4)):
            xv, flag = al.inp("x_" + name, x, skew=skew), al.inp("flag_" + name, np.array([start], np.int32))
            K._check(L.ssad_check_finite(p(xv), n, p(flag), K._stream()), "check_finite")
            res[name] = flag
        return res

    got, _ = arena_run(K, monkeypatch, fn, modified=("flag_inf", "flag_nan_or"))
    assert [int(got[k][0]) for k in ("finite", "kept", "inf", "nan_or")] == [0, 4, 1, 5]


def loss_scale_step(s, flag, good, growth, backoff, interval, lo, hi):
    """ssad_loss_scale_update restated (float32)"""
    s, good = (s * np.float32(backoff), 0) if flag else (s, good + 1)
    if not flag and good >= interval:
        s, good = s * np.float32(growth), 0
    return np.float32(min(max(s, np.float32(lo)), np.float32(hi))), good


def test_guarded_loss_scale_update(K, monkeypatch):
    """state {scale, 1 / scale} and counters {overflow flag, good steps} between guards.  Five steps: overflow ->
    backoff; a good step; growth at the interval, clamped at max_scale; overflow; overflow clamped at min_scale."""
    growth, backoff, interval, lo, hi = 2.0, 0.5, 2, 300.0, 600.0
    flags = [1, 0, 0, 1, 1]
    L = K.lib()

    def fn(al):
        state = al.inp("state", np.array([1024.0, 1.0 / 1024.0], np.float32))
        counters = al.inp("counters", np.array([0, 1], np.int32))
        trace_s, trace_c = [], []
        for f in flags:
            counters[0] = f                                        # what ssad_check_finite leaves behind
            K._check(L.ssad_loss_scale_update(p(state), p(counters), growth, backoff, interval, lo, hi, K._stream()),
                     "loss_scale_update")
            trace_s.append(state.clone())
            trace_c.append(counters.clone())
        return dict(state=torch.stack(trace_s), counters=torch.stack(trace_c))

    got, _ = arena_run(K, monkeypatch, fn, modified=("state", "counters"))
    s, good, want_s, want_c = np.float32(1024.0), 1, [], []
    for f in flags:
        s, good = loss_scale_step(s, f, good, growth, backoff, interval, lo, hi)
        want_s.append([s, np.float32(1.0) / s])
        want_c.append([0, good])
    assert [float(r[0]) for r in want_s] == [512.0, 512.0, 600.0, 300.0, 300.0]
    assert same(got["state"], np.array(want_s, np.float32)) and same(got["counters"], np.array(want_c, np.int32))


def amax_word(*tensors):
    return np.array([np.abs(t).max() for t in tensors], np.float32).view(np.int32)


def test_guarded_wgrad_split_with_handed_over_amax_words(K, monkeypatch):
    """conv3x3_wgrad / conv1x1_wgrad (split=True, x_amax=, dy_amax=): the |max| words are frozen arena inputs, and the
    result is bit for bit the one of the call that measures them itself"""
    rng = np.random.default_rng(9700)
    N, C3, M3, H3, W3 = 2, 16, 40, 9, 17
    C1, M1, H1, W1 = 72, 300, 5, 8
    X3, dY3 = randn(rng, N, C3, H3, W3), randn(rng, N, M3, H3, W3)
    X1, dY1 = randn(rng, N, C1, H1, W1), randn(rng, N, M1, H1, W1)

    def fn(al):
        x3, dy3, x1, dy1 = al.inp("x3", X3), al.inp("dy3", dY3), al.inp("x1", X1), al.inp("dy1", dY1)
        res = {}
        res["dW3"], res["db3"] = K.conv3x3_wgrad([x3], [dy3], M3, split=True, dW=al.out("dW3", (M3, C3, 3, 3)),
                                                 db=al.out("db3", (M3,)), x_amax=al.inp("x3_amax", amax_word(X3)),
                                                 dy_amax=al.inp("dy3_amax", amax_word(dY3)))
        res["own3"], res["ownb3"] = K.conv3x3_wgrad([x3], [dy3], M3, split=True, dW=al.out("dW3_own", (M3, C3, 3, 3)),
                                                    db=al.out("db3_own", (M3,)))
        res["dw1"] = K.conv1x1_wgrad(x1, dy1, out=al.out("dw1", (M1, C1)), split=True,
                                     x_amax=al.inp("x1_amax", amax_word(X1)), dy_amax=al.inp("dy1_amax", amax_word(dY1)))
        res["own1"] = K.conv1x1_wgrad(x1, dy1, out=al.out("dw1_own", (M1, C1)), split=True)
        return res

    got, _ = arena_run(K, monkeypatch, fn)
    assert same(got["dW3"], got["own3"]) and same(got["db3"], got["ownb3"]) and same(got["dw1"], got["own1"])
    rW, rb, _ = oracle.conv_backward(X3, np.zeros((M3, C3, 3, 3), np.float32), dY3)
    close(got["dW3"], rW, CONV_RTOL, CONV_FLOOR, "dW 3x3")
    close(got["db3"], rb, CONV_RTOL, CONV_FLOOR, "db 3x3")
    r1 = oracle.conv_backward(X1, np.zeros((M1, C1, 1, 1), np.float32), dY1, kernel=1, stride=1, pad=0)[0]
    close(got["dw1"], r1.reshape(M1, C1), CONV_RTOL, CONV_FLOOR, "dW 1x1")


# ---------------------------------------------------------------------------------------------------------------------
# Part B: what a bad value may reach
# ---------------------------------------------------------------------------------------------------------------------

def test_nan_ground_truth_stays_in_its_image(K):
    """one NaN coordinate in a ground-truth box INSIDE image 1's count: the label planes, fg rows and targets of
    images 0 and 2 are bit-identical to the clean run (fg_bg and image 1 itself are not asserted)"""
    from ssad_amd.roi_data.retinanet import RetinanetLabeler
    rng = np.random.default_rng(9800)
    counts = [4, 3, 6]
    boxes, classes = gt_arrays([rand_gts(rng, c, BLOB_H, BLOB_W) for c in counts], counts)
    bad = boxes.copy()
    bad[1, 1, 2] = np.nan

    def run(b):
        blobs = RetinanetLabeler(N_IM, GMAX, BLOB_H, BLOB_W)(dev(b), dev(classes), dev(np.array(counts, np.int32)))
        return {k: v.cpu().numpy().copy() for k, v in blobs.items()}

    clean, dirty = run(boxes), run(bad)
    rows = 0
    for lvl in range(3, 8):
        lc, ld = clean["retnet_cls_labels_fpn%d" % lvl], dirty["retnet_cls_labels_fpn%d" % lvl]
        assert same(lc[[0, 2]], ld[[0, 2]]), "labels level %d" % lvl
        kc = clean["retnet_roi_fg_bbox_locs_fpn%d" % lvl][:, 0] != 1
        kd = dirty["retnet_roi_fg_bbox_locs_fpn%d" % lvl][:, 0] != 1
        for name in ("retnet_roi_fg_bbox_locs_fpn%d", "retnet_roi_bbox_targets_fpn%d"):
            assert same(clean[name % lvl][kc], dirty[name % lvl][kd]), name % lvl
        rows += int(kc.sum())
    assert rows > 0
    assert any(not same(clean[k], dirty[k]) for k in clean), "the planted NaN changed nothing at all"


def detect_plain(probs, deltas):
    from ssad_amd.roi_data.retinanet import RetinanetDetector
    det = RetinanetDetector(DET_SHAPES, pre_nms_topn=TOPN, dets_per_im=KEEP)
    return det([dev(a) for a in probs], [dev(a) for a in deltas], IM_H, IM_W, IM_SCALE).cpu().numpy().copy()


def cell_of(level, flat):
    """(anchor, class, y, x) of element `flat` of a level's [A*C][H][W] score map"""
    h, w = DET_SHAPES[level]
    ac, y, x = np.unravel_index(flat, (DET_A * DET_C, h, w))
    return int(ac) // DET_C, int(ac) % DET_C, int(y), int(x)


def test_nan_scores_are_never_candidates(K):
    """the best score of the finest level and of the coarsest (threshold 0) become NaN: the result is the oracle's for
    those two scores set to 0"""
    probs, deltas = det_inputs()
    zeroed = [a.copy() for a in probs]
    for l in (0, 2):
        top = int(np.argmax(probs[l]))
        probs[l].reshape(-1)[top], zeroed[l].reshape(-1)[top] = np.nan, 0.0
    ref = det_oracle(zeroed, deltas)
    assert not same(ref, det_oracle(det_inputs()[0], deltas)), "the two scores did not matter"
    assert_detections(detect_plain(probs, deltas), ref)


def test_inf_score_sorts_first(K):
    probs, deltas = det_inputs()
    probs[0].reshape(-1)[int(np.argsort(probs[0].reshape(-1))[-7])] = np.inf
    ref = det_oracle(probs, deltas)
    assert np.isposinf(ref[0, 4]) and np.isfinite(ref[:, :4]).all() and np.isfinite(ref[1:, 4]).all()
    assert_detections(detect_plain(probs, deltas), ref)


def test_inf_deltas_are_clipped_like_the_oracle(K):
    """+Inf in dw of the best candidate's anchor cell (bbox_xform_clip) and +Inf in dx of the second best's (the clip
    to the image): finite rows in numpy and here"""
    probs, deltas = det_inputs()
    order = np.argsort(probs[0].reshape(-1))[::-1]
    a1, _, y1, x1 = cell_of(0, order[0])
    a2, _, y2, x2 = next(c for c in (cell_of(0, f) for f in order[1:]) if (c[0], c[2], c[3]) != (a1, y1, x1))
    deltas[0][0, 4 * a1 + 2, y1, x1] = np.inf
    deltas[0][0, 4 * a2 + 0, y2, x2] = np.inf
    ref = det_oracle(probs, deltas)
    assert np.isfinite(ref).all(), "the oracle's rows are not finite for this input: choose another cell"
    assert not same(ref, det_oracle(*det_inputs())), "the two deltas did not matter"
    assert_detections(detect_plain(probs, deltas), ref)


def test_nan_delta_of_no_candidate_changes_nothing(K):
    """a NaN in all four deltas of a middle-level anchor cell none of whose 80 scores passes the threshold"""
    probs, deltas = det_inputs()
    h, w = DET_SHAPES[1]
    passing = (probs[1].reshape(DET_A, DET_C, h, w) > 0.05).any(axis=1)          # [A][h][w]
    a, y, x = (int(v[0]) for v in np.nonzero(~passing))
    clean = detect_plain(probs, deltas)
    deltas[1][0, 4 * a:4 * a + 4, y, x] = np.nan
    assert same(detect_plain(probs, deltas), clean)


def test_nan_box_stays_in_its_soft_nms_segment(K, zs):
    """one NaN coordinate in the candidate of class 2 of the ms_* case: keys and ranks of every other class are
    bit-identical to the clean run"""
    from test_gpu_soft_nms import raw_soft_nms
    dets, cls = zs["ms_dets"], zs["ms_cls"]
    at = np.flatnonzero(cls == 2)
    assert len(at) >= 1
    bad = dets.copy()
    bad[at[0], 1] = np.nan
    others = cls != 2
    for method in (2, 1):                                             # SSAD_NMS_SOFT_LINEAR, SSAD_NMS_SOFT_HARD
        ck, cr = raw_soft_nms(dets, cls, int(zs["ms_classes"]), method)
        dk, dr = raw_soft_nms(bad, cls, int(zs["ms_classes"]), method)
        assert same(ck[others], dk[others]) and same(cr[others], dr[others]), method


@pytest.mark.parametrize("image,category", [(0, 0), (1, 1)])
def test_nan_score_stays_in_its_evaluation_cell(K, ze, image, category):
    """one NaN score in one cell: det_rank of that cell is still a permutation of 0 ... D-1 with the NaN last, as
    score_key promises; every output of other images or categories is bit-identical to the clean run.  The fixture's
    image 0 holds category 0 only (62 detections) and image 1 category 1 only (130: the cell is cut at max_det = 100,
    so the NaN, last of 130, falls behind the cut and the 100 ranks are a permutation without it); its cell
    (image 0, category 1) holds no detection, so these two cells stand for it."""
    z, ev = ze, evaluator(ze, True)
    DK = ev._DK
    I, Kc, cap, A, T, G = ev.I, ev.K, ev.cap, ev.A, ev.T, ev.G
    AT = A * T
    per, cat, score = eval_inputs(z)
    cell = np.flatnonzero(cat[image] == category)
    D = min(len(cell), ev.max_dets[-1])
    assert len(cell) >= 2
    victim = int(cell[np.argmax(score[image, cell])])                 # the cell's best detection becomes its last

    def run(poison):
        det_xywh, det_score = torch.zeros((I, cap, 4), dtype=F64, device="cuda"), torch.zeros((I, cap), dtype=F64, device="cuda")
        det_cat, bad = torch.full((I, cap), -1, dtype=I32, device="cuda"), torch.zeros(1, dtype=I32, device="cuda")
        for img, (b, s, c) in enumerate(per):
            s = s.copy()
            if poison and img == image:
                s[victim] = np.nan
            if len(s):
                DK.coco_eval_add(dev(b), 4, dev(s), 1, None, 0, dev(c), len(s), cap, Kc, img, det_xywh, det_score, det_cat, bad)
        out = dict(det_rank=torch.full((I, cap), 77, dtype=I32, device="cuda"),
                   dt_match=torch.full((I, cap, AT), 77, dtype=I32, device="cuda"),
                   dt_ignore=torch.full((I, cap, AT), 77, dtype=U8, device="cuda"),
                   cell_npig=torch.full((I * Kc, A), 77, dtype=I32, device="cuda"),
                   cell_eval=torch.full((I * Kc,), 77, dtype=U8, device="cuda"))
        ws = torch.full((DK.coco_eval_match_workspace_bytes(G, A, T),), 0x5A, dtype=U8, device="cuda")
        DK.coco_eval_match(I, Kc, cap, det_xywh, det_score, det_cat, ev.gt_xywh, ev.gt_area, ev.gt_crowd, ev.gt_off, G,
                           ev.d_iou, T, ev.d_rng, A, ev.max_dets[-1], True, out["det_rank"], out["dt_match"],
                           out["dt_ignore"], out["cell_npig"], out["cell_eval"], ws)
        return {k: v.cpu().numpy() for k, v in out.items()}

    clean, dirty = run(False), run(True)
    r = dirty["det_rank"][image, cell]
    assert sorted(r[r >= 0]) == list(range(D)) and int((r < 0).sum()) == len(cell) - D
    assert dirty["det_rank"][image, victim] == (len(cell) - 1 if len(cell) <= D else -1) and clean["det_rank"][image, victim] == 0
    assert np.array_equal(dirty["det_rank"], host_ranks(cat, np.where(
        (np.arange(I)[:, None] == image) & (np.arange(cap)[None, :] == victim), np.nan, score), ev.max_dets[-1]))
    other = np.ones((I, cap), bool)
    other[image, cell] = False
    for k in ("det_rank", "dt_match", "dt_ignore"):
        assert same(clean[k][other], dirty[k][other]), k
    cells = np.ones(I * Kc, bool)
    cells[image * Kc + category] = False
    assert same(clean["cell_npig"][cells], dirty["cell_npig"][cells]) and same(clean["cell_eval"][cells], dirty["cell_eval"][cells])
