"""BatchedRetinanetDetector / ssad_retinanet_detect_batch / ssad_detections_to_gt (detect_batch.hip) on the device.

The oracle is the existing per-image RetinanetDetector on each image's [n:n+1] slices (pinned by the reference's own
text in test_anchor_labels.py / test_gpu_isolation_detect.py): every comparison with it is bit for bit, `dets` viewed
as int32 and `counts`.  The batched path is never compared with itself, and every fast-path case asserts
`last_fallback == []`, so it cannot pass on the fallback alone.

Shapes: A*C = 720 on [(10,14),(5,7),(3,4),(2,2),(1,1)] (138 240 scores an image), N = 3; the class-specific and the
isolation cases use A*C = 27 on levels whose A*C*H*W is odd, so images 1 and 2 start off a 16-byte boundary and the
candidate pass takes its scalar head and tail.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import anchors as OA  # noqa: E402
from oracle import detect as OD  # noqa: E402
from test_gpu_isolation import isolated  # noqa: E402
from test_anchor_labels import DETECT_BOX_TOL  # noqa: E402

pytestmark = pytest.mark.gpu

I32 = torch.int32
SHAPES = [(10, 14), (5, 7), (3, 4), (2, 2), (1, 1)]
AC, N = 720, 3
IM_H, IM_W, IM_SCALE = [80, 75, 66], [112, 100, 90], [1.0, 0.9375, 1.25]
XFORM_CLIP = float(np.log(1000. / 16.))


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ssad_amd import kernels
    kernels.lib()  # raises if the HIP extension is missing: no fallback
    return kernels


def cfg4():
    from ssad_amd.modeling.generate_anchors import AnchorConfig

    class Cfg(AnchorConfig):
        num_classes = 4
    return Cfg


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sparse_maps(seed, planted, shapes=SHAPES, ac=AC, n_img=N, box_ch=36, last_zero=False):
    """Background: distinct multiples of 2^-22 per (image, level), all below 0.025 < 0.05 (on the last level, whose
    threshold is 0, they are the candidates -- or exact zeros with last_zero).  planted[n][l] scores per (image,
    level), distinct within the image: 0.0625 + j * 2^-12, at random cells."""
    rng = np.random.default_rng(seed)
    probs = [np.zeros((n_img, ac, h, w), np.float32) for h, w in shapes]
    deltas = [(rng.standard_normal((n_img, box_ch, h, w)) * 0.4).astype(np.float32) for h, w in shapes]
    for n in range(n_img):
        j = 0
        for l, (h, w) in enumerate(shapes):
            e = ac * h * w
            assert e * 2.0 ** -22 < 0.025
            flat = ((rng.permutation(e) + 1).astype(np.float64) * 2.0 ** -22).astype(np.float32)
            if last_zero and l == len(shapes) - 1:
                flat[:] = 0.0
            k = planted[n][l]
            at = rng.choice(e, size=k, replace=False)
            flat[at] = (0.0625 + (j + rng.permutation(k)) * 2.0 ** -12).astype(np.float32)
            j += k
            assert 0.0625 + j * 2.0 ** -12 < 1.0
            probs[l][n] = flat.reshape(ac, h, w)
    return probs, deltas


def per_image(probs, deltas, shapes=SHAPES, keep=100, sizes=(IM_H, IM_W, IM_SCALE), **kw):
    """the oracle: RetinanetDetector on each image's slices -> (dets [N][keep][6] zero-padded, counts [N]) as numpy"""
    from ssad_amd.roi_data.retinanet import RetinanetDetector
    det = RetinanetDetector(shapes, dets_per_im=keep, **kw)
    n_img = probs[0].shape[0]
    dets, counts = np.zeros((n_img, keep, 6), np.float32), np.zeros(n_img, np.int32)
    for n in range(n_img):
        rows = det([dev(p[n:n + 1]) for p in probs], [dev(d[n:n + 1]) for d in deltas], sizes[0][n], sizes[1][n],
                   sizes[2][n]).cpu().numpy()
        dets[n, :rows.shape[0]], counts[n] = rows, rows.shape[0]
    return dets, counts


def batched(probs, deltas, shapes=SHAPES, keep=100, sizes=(IM_H, IM_W, IM_SCALE), **kw):
    from ssad_amd.roi_data.retinanet import BatchedRetinanetDetector
    det = BatchedRetinanetDetector(probs[0].shape[0], shapes, dets_per_im=keep, **kw)
    dets, counts = det([dev(p) for p in probs], [dev(d) for d in deltas], *sizes)
    return det, dets.cpu().numpy().copy(), counts.cpu().numpy().copy()


def assert_same(got, want, what=""):
    (gd, gc), (wd, wc) = got, want
    assert gc.dtype == np.int32 and np.array_equal(gc, wc), (what, gc, wc)
    assert gd.shape == wd.shape and np.array_equal(gd.view(np.int32), wd.view(np.int32)), \
        "%s: rows differ from the per-image detector, first at %s" % (
            what, np.argwhere(gd.view(np.int32) != wd.view(np.int32))[:1].tolist())


PLANTED = [[150, 40, 12, 5, 0], [3, 130, 0, 2, 0], [101, 99, 30, 0, 0]]


def test_sparse_maps_take_the_fast_path():
    """topn = 100 cuts inside two lists (150, 130 and 101 planted) and just misses one (99); the default capacity is
    max(400, 720) = 720: the last level's 720 positive scores fit exactly, every other level counts <= 150."""
    probs, deltas = sparse_maps(9901, PLANTED)
    det, dets, counts = batched(probs, deltas, pre_nms_topn=100)
    assert det.capacity == 720 and det.last_fallback == []
    want = per_image(probs, deltas, pre_nms_topn=100)
    assert want[1].min() > 0
    assert_same((dets, counts), want, "sparse")


def test_topk_inside_the_list_with_equal_scores_across_the_cut():
    """120 candidates on level 0 of image 1: 40 distinct, then 30 equal scores on ranks 40 ... 69, then 50 distinct
    lower ones; topn = 50 keeps ten of the equal run -- those with the lowest element index, as detect.hip does.
    The last level is all zeros (its 720 cells would not fit capacity 256)."""
    planted = [[20, 5, 0, 0, 0], [120, 7, 3, 0, 0], [50, 51, 0, 0, 0]]
    probs, deltas = sparse_maps(9902, planted, last_zero=True)
    lvl = probs[0][1].reshape(-1)
    at = np.flatnonzero(lvl > 0.05)
    order = at[np.argsort(-lvl[at])]
    tie = np.float32(lvl[order[40]])
    lvl[order[40:70]] = tie
    probs[0][1] = lvl.reshape(probs[0][1].shape)
    assert (probs[0][1] > tie).sum() == 40 and (probs[0][1] == tie).sum() == 30
    det, dets, counts = batched(probs, deltas, pre_nms_topn=50, candidate_capacity=256, nms_thresh=2.0, keep=150)
    assert det.last_fallback == []
    assert_same((dets, counts), per_image(probs, deltas, pre_nms_topn=50, nms_thresh=2.0, keep=150), "ties")
    # nothing is suppressed at nms_thresh 2: image 1 emits 50 + 7 + 3 rows, ten of them with the tied score
    assert counts[1] == 60 and (dets[1, :60, 4] == tie).sum() == 10


def test_dense_and_mixed_maps_fall_back_per_image():
    rng = np.random.default_rng(9903)
    dense = [rng.random((N, AC, h, w), dtype=np.float32) for h, w in SHAPES]
    sparse, deltas = sparse_maps(9904, PLANTED)
    det, dets, counts = batched(dense, deltas, pre_nms_topn=100, candidate_capacity=1024)
    assert det.last_fallback == [0, 1, 2]
    assert_same((dets, counts), per_image(dense, deltas, pre_nms_topn=100), "dense")
    mixed = [s.copy() for s in sparse]
    for m, d in zip(mixed, dense):
        m[1] = d[1]
    det, dets, counts = batched(mixed, deltas, pre_nms_topn=100, candidate_capacity=1024)
    assert det.last_fallback == [1]
    assert_same((dets, counts), per_image(mixed, deltas, pre_nms_topn=100), "mixed")


def test_empty_image_and_nan_locality():
    planted = [PLANTED[0], [0, 0, 0, 0, 0], PLANTED[2]]
    probs, deltas = sparse_maps(9905, planted, last_zero=True)
    for p in probs:
        p[1] = np.minimum(p[1], 0.0)             # nothing above 0.05, nothing above 0 on the last level
    det, dets, counts = batched(probs, deltas, pre_nms_topn=100)
    assert det.last_fallback == [] and counts[1] == 0 and not dets[1].view(np.int32).any()
    assert counts[0] > 0 and counts[2] > 0
    assert_same((dets, counts), per_image(probs, deltas, pre_nms_topn=100), "empty")
    # NaN / +Inf scores and deltas inside image 1 only
    bad_p, bad_d = [p.copy() for p in probs], [d.copy() for d in deltas]
    bad_p[0][1, 5, 2, 3], bad_p[0][1, 700, 9, 13], bad_p[1][1, 0, 0, 0] = np.nan, np.inf, np.inf
    bad_d[0][1, :, 9, 13], bad_d[1][1, :, 0, 0] = np.inf, np.nan
    det2, dets2, counts2 = batched(bad_p, bad_d, pre_nms_topn=100)
    assert det2.last_fallback == [] and counts2[1] == 2          # the two +Inf scores; the NaN is no candidate
    for n in (0, 2):
        assert counts2[n] == counts[n] and np.array_equal(dets2[n].view(np.int32), dets[n].view(np.int32)), n


ODD_SHAPES = [(5, 7), (3, 3), (1, 1)]          # 27 * 35, 27 * 9, 27 scores: odd, so images 1 and 2 are misaligned
ODD_SIZES = ([40, 38, 33], [56, 50, 45], [1.0, 0.9375, 1.25])


def test_class_specific_bbox_on_odd_sized_levels():
    cfg = cfg4()
    planted = [[60, 9, 0], [45, 0, 0], [70, 20, 0]]
    probs, deltas = sparse_maps(9906, planted, shapes=ODD_SHAPES, ac=27, box_ch=9 * 4 * 3)
    assert all(p[0].size % 4 for p in probs)
    kw = dict(cfg=cfg, pre_nms_topn=40, class_specific_bbox=True)
    det, dets, counts = batched(probs, deltas, shapes=ODD_SHAPES, sizes=ODD_SIZES, **kw)
    assert det.last_fallback == [] and det.capacity == 160
    assert_same((dets, counts), per_image(probs, deltas, shapes=ODD_SHAPES, sizes=ODD_SIZES, **kw), "class-specific")
    # the class-agnostic detector on the same scores (first 36 delta channels) gives other boxes: the indexing matters
    plain_d = [np.ascontiguousarray(d[:, :36]) for d in deltas]
    _, pd, pc = batched(probs, plain_d, shapes=ODD_SHAPES, sizes=ODD_SIZES, cfg=cfg, pre_nms_topn=40)
    assert_same((pd, pc), per_image(probs, plain_d, shapes=ODD_SHAPES, sizes=ODD_SIZES, cfg=cfg, pre_nms_topn=40), "plain")
    assert not np.array_equal(pd[:, :, :4], dets[:, :, :4])


def test_repeatable_and_independent_of_workspace_contents():
    """same call twice, and once more on a workspace, outputs and flags refilled with 0xFF bytes (NaN words, negative
    counters): the launcher zeroes its counters itself and the arrival order in the lists does not reach the rows"""
    from ssad_amd.roi_data.retinanet import BatchedRetinanetDetector
    probs, deltas = sparse_maps(9907, PLANTED)
    dp, dd = [dev(p) for p in probs], [dev(d) for d in deltas]
    det = BatchedRetinanetDetector(N, SHAPES, pre_nms_topn=100)
    runs = []
    for junk in (False, False, True):
        if junk:
            for t in (det.ws, det.out.view(torch.uint8), det.counts.view(torch.uint8), det.overflow.view(torch.uint8)):
                t.fill_(0xFF)
        dets, counts = det(dp, dd, IM_H, IM_W, IM_SCALE)
        assert det.last_fallback == []
        runs.append((dets.cpu().numpy().copy(), counts.cpu().numpy().copy()))
    assert_same(runs[1], runs[0], "second call")
    assert_same(runs[2], runs[0], "junk workspace")
    assert_same(runs[0], per_image(probs, deltas, pre_nms_topn=100), "oracle")


# ---------------------------------------------------------------------------------------------------------------------
# isolation (tests/guarded.py): operands, outputs and the exactly-sized workspace inside one sentinel-filled arena
# ---------------------------------------------------------------------------------------------------------------------

def p(t):
    return C.c_void_p(t.data_ptr())


def test_guarded_detect_batch_and_detections_to_gt(K, monkeypatch):
    cfg = cfg4()
    from ssad_amd.modeling.generate_anchors import cell_anchors
    planted = [[80, 9, 0], [45, 0, 0], [70, 20, 0]]
    probs, deltas = sparse_maps(9908, planted, shapes=ODD_SHAPES, ac=27)
    levels, A, Cn, topn, cap, keep, gmax = len(ODD_SHAPES), 9, 3, 40, 64, 50, 8
    # capacity 64 is below two planted counts: images 0 and 2 overflow on level 0, their lists stop at 64 keys
    cells = np.ascontiguousarray(np.asarray(cell_anchors(cfg), np.float64)[:levels])
    L = K.lib()
    IntArr, PtrArr = C.c_int * levels, C.c_void_p * levels
    H, W = IntArr(*[h for h, _ in ODD_SHAPES]), IntArr(*[w for _, w in ODD_SHAPES])
    nb = int(L.ssad_retinanet_detect_batch_workspace_bytes(N, levels, A, Cn, H, W, topn, cap))
    assert nb > 0
    scales = np.array(ODD_SIZES[2], np.float32)

    def fn(al):
        dc = al.inp("cells", cells)
        tp = [al.inp("prob%d" % l, a) for l, a in enumerate(probs)]
        td = [al.inp("delta%d" % l, a) for l, a in enumerate(deltas)]
        dets, counts, over = al.out("dets", (N, keep, 6)), al.out("counts", (N,), I32), al.out("overflow", (N,), I32)
        ws = al.ws(nb, "detect_batch")
        assert ws.numel() == nb
        rc = L.ssad_retinanet_detect_batch(
            PtrArr(*[t.data_ptr() for t in tp]), PtrArr(*[t.data_ptr() for t in td]), p(dc), N, levels, A, Cn, 3, H, W,
            0.05, topn, cap, 0.5, keep, (C.c_float * N)(*ODD_SIZES[2]), (C.c_int * N)(*ODD_SIZES[0]),
            (C.c_int * N)(*ODD_SIZES[1]), XFORM_CLIP, 0, p(dets), p(counts), p(over), p(ws), nb, K._stream())
        assert rc == 0, rc
        sc = al.inp("im_scale", scales)
        gb, gc, gn = al.out("gt_boxes", (N, gmax, 4)), al.out("gt_classes", (N, gmax), I32), al.out("gt_counts", (N,), I32)
        rc = L.ssad_detections_to_gt(p(dets), p(counts), p(sc), N, keep, 0.07, gmax, p(gb), p(gc), p(gn), K._stream())
        assert rc == 0, rc
        # the rows of an overflowed image are unspecified: only image 1's are returned for the placement comparison
        return dict(dets1=dets[1], counts=counts[1:2], overflow=over, gt_boxes1=gb[1], gt_classes1=gc[1], gt_counts1=gn[1:2])

    # isolated() asserts: guards intact, inputs bit-identical, dets / counts / overflow / gt_* fully written
    got = isolated(K, monkeypatch, fn)
    assert list(got["overflow"] != 0) == [True, False, True]
    want = per_image(probs, deltas, shapes=ODD_SHAPES, keep=keep, sizes=ODD_SIZES, cfg=cfg, pre_nms_topn=topn)
    c1 = int(got["counts"][0])
    assert c1 == want[1][1] and np.array_equal(got["dets1"].view(np.int32), want[0][1].view(np.int32))
    assert not got["dets1"][c1:].view(np.int32).any()
    g = int(got["gt_counts1"][0])
    assert g == min(gmax, int((want[0][1][:c1, 4] >= np.float32(0.07)).sum())) and 0 < g
    assert not got["gt_boxes1"][g:].view(np.int32).any() and not got["gt_classes1"][g:].any()
    assert np.array_equal(got["gt_boxes1"][:g], want[0][1][:g, :4] * scales[1])


# ---------------------------------------------------------------------------------------------------------------------
# against the CPU oracle, pseudo-labels, the subnets
# ---------------------------------------------------------------------------------------------------------------------

def test_sparse_case_against_the_cpu_oracle():
    probs, deltas = sparse_maps(9909, PLANTED)
    det, dets, counts = batched(probs, deltas, pre_nms_topn=100)
    assert det.last_fallback == []
    cells = np.array([[OA.generate_cell64(l, a) for a in range(9)] for l in range(3, 3 + len(SHAPES))])
    for n in range(N):
        ref = OD.im_detect_bbox([q[n:n + 1] for q in probs], [d[n:n + 1] for d in deltas], cells, (IM_H[n], IM_W[n]),
                                IM_SCALE[n], pre_nms_topn=100)
        got = dets[n, :counts[n]]
        assert got.shape == ref.shape and ref.shape[0] > 0, (n, got.shape, ref.shape)
        assert np.array_equal(got[:, 4], ref[:, 4]) and np.array_equal(got[:, 5], ref[:, 5])
        np.testing.assert_allclose(got[:, :4], ref[:, :4], **DETECT_BOX_TOL)


def restate_pseudo_labels(dets, counts, scales, thresh, gmax):
    n_img = dets.shape[0]
    gb, gc, gn = np.zeros((n_img, gmax, 4), np.float32), np.zeros((n_img, gmax), np.int32), np.zeros(n_img, np.int32)
    for n in range(n_img):
        rows = dets[n, :counts[n]]
        rows = rows[rows[:, 4] >= np.float32(thresh)][:gmax]
        gn[n] = len(rows)
        gb[n, :len(rows)] = rows[:, :4] * np.float32(scales[n])
        gc[n, :len(rows)] = rows[:, 5].astype(np.int32)
    return gb, gc, gn


def test_pseudo_labels_and_the_labeler():
    """crafted score-sorted rows: image 0 has 14 survivors of the cut (Gmax = 8 keeps the first 8), image 1 none
    (count 0), image 2 five of its seven rows; rows behind a count hold junk that must not be read"""
    from ssad_amd.roi_data.retinanet import BatchedRetinanetDetector, RetinanetLabeler
    rng = np.random.default_rng(9910)
    keep, gmax, thresh, blob_h, blob_w = 20, 8, 0.3, 96, 128
    scales = [1.25, 1.0, 0.8]
    counts = np.array([20, 0, 7], np.int32)
    dets = np.full((N, keep, 6), np.nan, np.float32)
    for n, c in enumerate(counts):
        x1, y1 = rng.uniform(0, 60, c) / scales[n], rng.uniform(0, 40, c) / scales[n]
        bw, bh = rng.uniform(10, 60, c) / scales[n], rng.uniform(10, 50, c) / scales[n]
        score = np.sort(rng.uniform(0.05, 0.95, c))[::-1]
        if n == 0:
            score[:14], score[14:] = np.linspace(0.9, 0.31, 14), np.linspace(0.29, 0.06, 6)
        if n == 2:
            score[:5], score[5:] = [0.8, 0.7, 0.5, 0.3, 0.3], [0.2999, 0.1]
        dets[n, :c] = np.stack([x1, y1, x1 + bw, y1 + bh, score, rng.integers(1, 81, c)], 1)
    det = BatchedRetinanetDetector(N, SHAPES, dets_per_im=keep, pre_nms_topn=100)
    d_dets, d_counts = dev(dets), dev(counts)
    gb, gc, gn = det.pseudo_labels(d_dets, d_counts, scales, thresh, gmax)
    wb, wc, wn = restate_pseudo_labels(dets, counts, scales, thresh, gmax)
    assert list(wn) == [8, 0, 5]
    assert gn.dtype == I32 and np.array_equal(gn.cpu().numpy(), wn) and np.array_equal(gc.cpu().numpy(), wc)
    assert np.array_equal(gb.cpu().numpy().view(np.int32), wb.view(np.int32))
    # a device tensor of scales is taken as it is
    gb2, gc2, gn2 = det.pseudo_labels(d_dets, d_counts, dev(np.array(scales, np.float32)), thresh, gmax)
    assert torch.equal(gb2, gb) and torch.equal(gc2, gc) and torch.equal(gn2, gn)
    # the labeller on the device-made ground truth and on the same arrays uploaded from the host
    lab = RetinanetLabeler(N, gmax, blob_h, blob_w)
    a = {k: v.clone() for k, v in lab(gb, gc, gn).items()}
    b = lab(dev(wb), dev(wc), dev(wn))
    assert sorted(a) == sorted(b) and float(a["retnet_fg_num"][0]) > 0
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


def test_with_the_subnets_teacher_outputs():
    """DistillHeads leaves t_prob / t_bbox for the minibatch on the device: the batched detector on them equals the
    per-image detector on their slices.  The last of the two levels holds 720 * 35 positive scores: the default
    capacity takes the whole level, and its list is cut by the radix select."""
    from ssad_amd import synth
    from ssad_amd.head_pipeline import DistillHeads
    from ssad_amd.modeling.retinanet_heads import HeadConfig
    from ssad_amd.roi_data.retinanet import BatchedRetinanetDetector, RetinanetDetector
    rng = np.random.default_rng(9911)
    shapes = [(10, 14), (5, 7)]
    heads = DistillHeads(HeadConfig(num_gpus=1), N=2, shapes=shapes, device=torch.device("cuda", 0),
                         student_init=synth.head_params(rng), teacher_init=synth.head_params(rng))
    f = [dev(a) for a in synth.fpn_features(rng, 2, shapes)]
    heads.pack_student()
    heads.forward_all(f, f)
    t_prob, t_bbox = [t.contiguous() for t in heads.t_prob], [t.contiguous() for t in heads.t_bbox]
    sizes = ([80, 70], [112, 100], [1.0, 0.875])
    det = BatchedRetinanetDetector(2, shapes, pre_nms_topn=200)
    assert det.capacity == 720 * 35
    dets, counts = det(t_prob, t_bbox, *sizes)
    assert det.last_fallback == []
    single = RetinanetDetector(shapes, pre_nms_topn=200)
    for n in range(2):
        rows = single([t[n:n + 1] for t in t_prob], [t[n:n + 1] for t in t_bbox], sizes[0][n], sizes[1][n], sizes[2][n])
        assert rows.shape[0] == int(counts[n]) > 0
        assert torch.equal(dets[n, :rows.shape[0]].view(I32), rows.view(I32)), n
        assert not dets[n, rows.shape[0]:].view(I32).any()
