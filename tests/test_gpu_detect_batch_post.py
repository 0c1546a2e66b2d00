"""BatchedRetinanetDetector with Soft-NMS, box voting and the softmax head's logits (ssad_retinanet_detect_batch_ex).

The oracle is the per-image RetinanetDetector with the same options on each image's [n:n+1] slices (from_logits: its
group_spatial_softmax + detect.hip route); every comparison with it is bit for bit, `dets` viewed as int32 and
`counts`.  The batched path is never compared with itself and every fast-path case asserts `last_fallback == []`.

Helpers and shapes are test_gpu_detect_batch's: A*C = 720 on SHAPES, N = 3, and 4 classes on ODD_SHAPES.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_gpu_detect_batch as B  # noqa: E402
from test_gpu_isolation import isolated  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES, ODD_SHAPES, ODD_SIZES, N = B.SHAPES, B.ODD_SHAPES, B.ODD_SIZES, B.N
SIZES = (B.IM_H, B.IM_W, B.IM_SCALE)
I32 = torch.int32


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from ssad_amd import kernels
    kernels.lib()
    return kernels


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------

def clustered_maps(seed, shapes=SHAPES, n_cls=80, classes=(3, 17, 42), box_ch=36, block=(3, 4), anchors=(0, 4)):
    """sparse_maps' background (nothing planted) and, on level 0 of every image, candidates of at most three classes
    at the neighbouring cells of a block (two anchors each): same-class boxes one stride apart overlap.  Scores are
    distinct within the image, 0.0625 + j * 2^-12; the deltas are scaled down so the neighbours keep overlapping."""
    probs, deltas = B.sparse_maps(seed, [[0] * len(shapes)] * N, shapes=shapes, ac=9 * n_cls, box_ch=box_ch)
    deltas = [(d * np.float32(0.25)).astype(np.float32) for d in deltas]
    rng = np.random.default_rng(seed + 1)
    h, w = shapes[0]
    for n in range(N):
        y0, x0 = int(rng.integers(0, h - block[0] + 1)), int(rng.integers(0, w - block[1] + 1))
        cells = [(a, c, y0 + dy, x0 + dx) for a in anchors for c in classes[:1 + (n + 2) % 3 if n else 3]
                 for dy in range(block[0]) for dx in range(block[1])]
        order = rng.permutation(len(cells))
        for j, (a, c, y, x) in zip(order, cells):
            probs[0][n, a * n_cls + c, y, x] = np.float32(0.0625 + int(j) * 2.0 ** -12)
    return probs, deltas


def logit_maps(seed, planted, shapes=SHAPES, n_cls=80, box_ch=36, cap=720):
    """Logits [N][9*(n_cls+1)][H][W]: background 0, every foreground logit in (-9, -7), and planted[n][l] cells per
    (image, level) whose one class gets log(p / (1 - p)), p = 0.07 + j * 0.002 distinct within the image.  Checked here
    in float64: planted probabilities >= 0.06, every other foreground probability <= 0.04 (rounding cannot move a score
    across 0.05), and no (image, level) has more candidates than `cap` (the last level's threshold is 0)."""
    rng = np.random.default_rng(seed)
    K1 = n_cls + 1
    logits = [np.zeros((N, 9, K1, h, w), np.float32) for h, w in shapes]
    deltas = [(rng.standard_normal((N, box_ch, h, w)) * 0.4).astype(np.float32) for h, w in shapes]
    where = []
    for n in range(N):
        j = 0
        for l, (h, w) in enumerate(shapes):
            x = logits[l][n]
            x[:, 1:] = (-8.0 + rng.uniform(-1.0, 1.0, size=(9, n_cls, h, w))).astype(np.float32)
            k = planted[n][l]
            at = rng.choice(9 * h * w, size=k, replace=False)
            cls = rng.integers(1, K1, size=k)
            p = 0.07 + (j + rng.permutation(k)) * 0.002
            assert k == 0 or p.max() < 0.95
            j += k
            a, pos = at // (h * w), at % (h * w)
            x[a, cls, pos // w, pos % w] = np.log(p / (1.0 - p)).astype(np.float32)
            where.append((n, l, a, cls, pos))
    for l, (h, w) in enumerate(shapes):
        x64 = logits[l].astype(np.float64)
        e = np.exp(x64 - x64.max(axis=2, keepdims=True))
        p64 = (e / e.sum(axis=2, keepdims=True))[:, :, 1:]
        mark = np.zeros(p64.shape, bool)
        for n, ll, a, cls, pos in where:
            if ll == l:
                mark[n, a, cls - 1, pos // w, pos % w] = True
        assert not mark.any() or p64[mark].min() >= 0.06
        assert p64[~mark].max() <= 0.04
        th = 0.0 if l == len(shapes) - 1 else 0.05
        assert (p64 > th).reshape(N, -1).sum(axis=1).max() <= cap
    return [x.reshape(N, 9 * K1, x.shape[3], x.shape[4]) for x in logits], deltas


def oracle_logits(logits, deltas, shapes=SHAPES, keep=100, sizes=SIZES, **kw):
    """RetinanetDetector(softmax=True) on each image's logit slices, from_logits=True"""
    from ssad_amd.roi_data.retinanet import RetinanetDetector
    det = RetinanetDetector(shapes, dets_per_im=keep, softmax=True, **kw)
    dets, counts = np.zeros((N, keep, 6), np.float32), np.zeros(N, np.int32)
    for n in range(N):
        rows = det([B.dev(x[n:n + 1]) for x in logits], [B.dev(d[n:n + 1]) for d in deltas], sizes[0][n], sizes[1][n],
                   sizes[2][n], from_logits=True).cpu().numpy()
        dets[n, :rows.shape[0]], counts[n] = rows, rows.shape[0]
    return dets, counts


def batched_logits(logits, deltas, shapes=SHAPES, keep=100, sizes=SIZES, fused=True, **kw):
    """fused: the candidate pass reads the logits (detb_candidates_logits_kernel) and no probability buffer exists;
    otherwise the class's default route, group_spatial_softmax on the batch and the candidate pass on its output"""
    from ssad_amd.roi_data.retinanet import BatchedRetinanetDetector
    det = BatchedRetinanetDetector(N, shapes, dets_per_im=keep, softmax=True, fused_logits=fused, **kw)
    assert (det._probs is None) == fused
    dets, counts = det([B.dev(x) for x in logits], [B.dev(d) for d in deltas], *sizes, from_logits=True)
    return det, dets.cpu().numpy().copy(), counts.cpu().numpy().copy()


def differ(a, b):
    return not np.array_equal(a.view(np.int32), b.view(np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# 1-3: Soft-NMS and voting on scores
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def clustered():
    probs, deltas = clustered_maps(9921)
    _, dets, counts = B.batched(probs, deltas, pre_nms_topn=100)
    return probs, deltas, (dets, counts)


@pytest.mark.parametrize("method", ["hard", "linear", "gaussian"])
def test_soft_nms(clustered, method):
    """score_thresh 0.07 lies inside the planted scores (0.0625 ...), so `hard` acts too: it retires an overlapped
    candidate below it, which the greedy scan keeps"""
    probs, deltas, greedy = clustered
    kw = dict(pre_nms_topn=100, soft_nms=dict(method=method, sigma=0.5, score_thresh=0.07))
    det, dets, counts = B.batched(probs, deltas, **kw)
    assert det.last_fallback == []
    B.assert_same((dets, counts), B.per_image(probs, deltas, **kw), method)
    assert counts.min() > 0 and differ(dets, greedy[0])


def test_soft_nms_segments_on_both_sides_of_the_lds_cap():
    """one launch: image 0's class 7 has 1100 candidates on level 0 (plus its 9 on the last level: above
    SSAD_SOFT_NMS_LDS_CAP = 1024, the walk on the workspace's live words), image 1's has 200 (in LDS), image 2's
    candidates are spread over the classes"""
    topn, cls = 1100, 7
    probs, deltas = B.sparse_maps(9922, [[0] * 5, [0] * 5, [300, 60, 10, 0, 0]])
    deltas = [(d * np.float32(0.25)).astype(np.float32) for d in deltas]
    rng = np.random.default_rng(9923)
    h, w = SHAPES[0]
    assert 9 * h * w == 1260
    for n, k in ((0, 1100), (1, 200)):
        at = rng.choice(9 * h * w, size=k, replace=False)
        score = (0.0625 + rng.permutation(k) * 2.0 ** -12).astype(np.float32)
        assert score.max() < 1.0
        probs[0][n, (at // (h * w)) * 80 + cls, (at % (h * w)) // w, at % w] = score
        assert int((probs[0][n] > 0.05).sum()) == k
    kw = dict(pre_nms_topn=topn, keep=300, soft_nms=dict(method="linear"))
    det, dets, counts = B.batched(probs, deltas, **kw)
    assert det.last_fallback == [] and det.capacity == 4 * topn
    B.assert_same((dets, counts), B.per_image(probs, deltas, **kw), "lds cap")
    assert counts.min() > 0 and (dets[0, :counts[0], 5] == cls + 1).sum() > 50


VOTES = [(None, m) for m in ("ID", "TEMP_AVG", "AVG", "IOU_AVG", "GENERALIZED_AVG", "QUASI_SUM")] + [("linear", "IOU_AVG")]


@pytest.mark.parametrize("soft,scoring", VOTES, ids=lambda v: str(v))
def test_box_voting(clustered, soft, scoring):
    """vote_th 0.3: the neighbours one stride apart vote for each other"""
    probs, deltas, greedy = clustered
    kw = dict(pre_nms_topn=100, bbox_vote=dict(vote_th=0.3, scoring_method=scoring, beta=0.7))
    if soft:
        kw["soft_nms"] = dict(method=soft)
    det, dets, counts = B.batched(probs, deltas, **kw)
    assert det.last_fallback == []
    B.assert_same((dets, counts), B.per_image(probs, deltas, **kw), scoring)
    unvoted = greedy[0] if not soft else B.batched(probs, deltas, pre_nms_topn=100, soft_nms=kw["soft_nms"])[1]
    assert counts.min() > 0 and differ(dets[:, :, :4], unvoted[:, :, :4])


def raw_batch(K, entry, probs, deltas, shapes, n_cls, topn, cap, keep, sizes, ws, extra=()):
    from ssad_amd.modeling.generate_anchors import AnchorConfig, cell_anchors
    levels = len(shapes)
    cells = B.dev(np.ascontiguousarray(np.asarray(cell_anchors(AnchorConfig), np.float64)[:levels]))
    IntArr, PtrArr = C.c_int * levels, C.c_void_p * levels
    H, W = IntArr(*[h for h, _ in shapes]), IntArr(*[w for _, w in shapes])
    dets = torch.full((N, keep, 6), float("nan"), device="cuda")
    counts, over = torch.full((N,), -7, dtype=I32, device="cuda"), torch.full((N,), -7, dtype=I32, device="cuda")
    rc = entry(PtrArr(*[t.data_ptr() for t in probs]), PtrArr(*[t.data_ptr() for t in deltas]), B.p(cells), N, levels, 9,
               n_cls, 3, H, W, 0.05, topn, cap, 0.5, keep, (C.c_float * N)(*sizes[2]), (C.c_int * N)(*sizes[0]),
               (C.c_int * N)(*sizes[1]), B.XFORM_CLIP, 0, B.p(dets), B.p(counts), B.p(over), B.p(ws), ws.numel(),
               K._stream(), *extra)
    assert rc == 0, rc
    return dets.cpu().numpy(), counts.cpu().numpy(), over.cpu().numpy()


def test_the_old_entry_and_ex_with_a_null_post_give_the_same_words(K, clustered):
    probs, deltas, _ = clustered
    L = K.lib()
    IntArr = C.c_int * len(SHAPES)
    nb = int(L.ssad_retinanet_detect_batch_workspace_bytes(N, len(SHAPES), 9, 80, IntArr(*[h for h, _ in SHAPES]),
                                                           IntArr(*[w for _, w in SHAPES]), 100, 720))
    dp, dd = [B.dev(a) for a in probs], [B.dev(a) for a in deltas]
    runs = []
    for entry, extra in ((L.ssad_retinanet_detect_batch, ()), (L.ssad_retinanet_detect_batch_ex, (None, 0))):
        ws = torch.full((nb,), 0x5A, dtype=torch.uint8, device="cuda")
        runs.append(raw_batch(K, entry, dp, dd, SHAPES, 80, 100, 720, 100, SIZES, ws, extra))
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert not runs[0][2].any() and runs[0][1].min() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 4-9: from logits
# ---------------------------------------------------------------------------------------------------------------------

def test_from_logits_81_classes(K):
    logits, deltas = logit_maps(9931, B.PLANTED)
    det, dets, counts = batched_logits(logits, deltas, pre_nms_topn=100)
    assert det.capacity == 720 and det.last_fallback == []
    want = oracle_logits(logits, deltas, pre_nms_topn=100)
    assert want[1].min() > 0
    B.assert_same((dets, counts), want, "from logits")
    det1, dets1, counts1 = batched_logits(logits, deltas, pre_nms_topn=100, fused=False)
    assert det1.last_fallback == []
    B.assert_same((dets1, counts1), want, "from logits, softmax kernel first")
    # the same maps as probabilities, made for the whole batch by the softmax kernel
    probs = [K.group_spatial_softmax(B.dev(x), 81, drop_background=True).cpu().numpy() for x in logits]
    det2, dets2, counts2 = B.batched(probs, deltas, pre_nms_topn=100, softmax=True)
    assert det2.last_fallback == []
    B.assert_same((dets2, counts2), want, "probabilities")


def test_from_logits_equal_scores_across_the_cut(K):
    """image 1, level 0: 120 planted cells; the 30 on ranks 40 ... 69 get one identical logit vector (class 9), so
    their probabilities are bit-equal; topn = 50 keeps the ten with the lowest element index, as detect.hip does"""
    planted = [[20, 5, 0, 0, 0], [120, 7, 3, 0, 0], [50, 51, 0, 0, 0]]
    logits, deltas = logit_maps(9932, planted)
    h, w = SHAPES[0]
    x = logits[0][1].reshape(9, 81, h * w)
    top = x[:, 1:].max(axis=1)                                   # the cell's largest foreground logit
    cells = np.argsort(-top.reshape(-1), kind="stable")[:120]
    assert top.reshape(-1)[cells[119]] > -3 and top.reshape(-1)[np.argsort(-top.reshape(-1))[120]] < -6
    vec = np.full(81, -8.0, np.float32)
    vec[0], vec[9] = 0.0, x[cells[40] // (h * w), 1:, cells[40] % (h * w)].max()
    for c in cells[40:70]:
        x[c // (h * w), :, c % (h * w)] = vec
    logits[0][1] = x.reshape(9 * 81, h, w)
    kw = dict(pre_nms_topn=50, nms_thresh=2.0, keep=150)
    det, dets, counts = batched_logits(logits, deltas, **kw)
    assert det.last_fallback == [] and det.capacity == 720
    B.assert_same((dets, counts), oracle_logits(logits, deltas, **kw), "ties")
    # nothing is suppressed at nms_thresh 2: image 1 emits 50 + 7 + 3 + the last level's 50 rows
    prob = K.group_spatial_softmax(B.dev(logits[0][1:2]), 81, drop_background=True).cpu().numpy().reshape(9, 80, h * w)
    tie = prob[cells[40] // (h * w), 8, cells[40] % (h * w)]
    assert (prob == tie).sum() == 30 and (prob > tie).sum() == 40
    assert counts[1] == 110 and (dets[1, :110, 4] == tie).sum() == 10


def test_from_logits_4_classes_class_specific_soft_nms_and_voting(K):
    """CMAX 16; 35- and 9-cell planes (a partial chunk of 256); the same maps as probabilities [N][27][H][W] put
    images 1 and 2 off a 16-byte boundary"""
    cfg = B.cfg4()
    logits, deltas = logit_maps(9933, [[60, 9, 0], [45, 0, 0], [70, 20, 0]], shapes=ODD_SHAPES, n_cls=3,
                                box_ch=9 * 4 * 3, cap=160)
    kw = dict(cfg=cfg, pre_nms_topn=40, class_specific_bbox=True, soft_nms=dict(method="gaussian"),
              bbox_vote=dict(vote_th=0.3, scoring_method="AVG"))
    det, dets, counts = batched_logits(logits, deltas, shapes=ODD_SHAPES, sizes=ODD_SIZES, **kw)
    assert det.last_fallback == [] and det.capacity == 160
    want = oracle_logits(logits, deltas, shapes=ODD_SHAPES, sizes=ODD_SIZES, **kw)
    assert want[1].min() > 0
    B.assert_same((dets, counts), want, "4 classes")
    det1, dets1, counts1 = batched_logits(logits, deltas, shapes=ODD_SHAPES, sizes=ODD_SIZES, fused=False, **kw)
    assert det1.last_fallback == []
    B.assert_same((dets1, counts1), want, "4 classes, softmax kernel first")
    probs = [K.group_spatial_softmax(B.dev(x), 4, drop_background=True).cpu().numpy() for x in logits]
    assert all(p[0].size % 4 for p in probs)
    det2, dets2, counts2 = B.batched(probs, deltas, shapes=ODD_SHAPES, sizes=ODD_SIZES, softmax=True, **kw)
    assert det2.last_fallback == []
    B.assert_same((dets2, counts2), want, "4 classes, probabilities")


def dense_logits(seed, images):
    """logit_maps' sparse maps with `images` replaced by dense ones: N(0, 1) logits and +3.5 on about 6 % of the
    foreground classes of every cell, so level 0 holds well over 1024 candidates"""
    logits, deltas = logit_maps(seed, B.PLANTED)
    rng = np.random.default_rng(seed + 1)
    for x in logits:
        for n in images:
            d = rng.standard_normal(x[n].shape).astype(np.float32).reshape(9, 81, -1)
            d[:, 1:] += np.float32(3.5) * (rng.random(d[:, 1:].shape) < 0.06)
            x[n] = d.reshape(x[n].shape)
    x64 = logits[0].astype(np.float64).reshape(N, 9, 81, -1)
    e = np.exp(x64 - x64.max(axis=2, keepdims=True))
    above = ((e / e.sum(axis=2, keepdims=True))[:, :, 1:] > 0.06).reshape(N, -1).sum(axis=1)
    assert all(above[n] > 2048 for n in images), above
    return logits, deltas


def test_from_logits_dense_images_fall_back_per_image():
    logits, deltas = dense_logits(9934, [1])
    kw = dict(pre_nms_topn=100, soft_nms=dict(method="linear"))
    det, dets, counts = batched_logits(logits, deltas, candidate_capacity=1024, **kw)
    assert det.last_fallback == [1]
    B.assert_same((dets, counts), oracle_logits(logits, deltas, **kw), "mixed")
    logits, deltas = dense_logits(9935, [0, 1, 2])
    det, dets, counts = batched_logits(logits, deltas, candidate_capacity=1024, pre_nms_topn=100)
    assert det.last_fallback == [0, 1, 2]
    B.assert_same((dets, counts), oracle_logits(logits, deltas, pre_nms_topn=100), "dense")


def test_from_logits_nonfinite_values_stay_in_their_image():
    logits, deltas = logit_maps(9936, B.PLANTED)
    det, dets, counts = batched_logits(logits, deltas, pre_nms_topn=100)
    assert det.last_fallback == []
    bad = [x.copy() for x in logits]
    bad[0][1, 5 * 81 + 7, 2, 3], bad[0][1, 2 * 81, 9, 13], bad[1][1, 0 * 81 + 80, 0, 0] = np.nan, np.inf, np.inf
    det2, dets2, counts2 = batched_logits(bad, deltas, pre_nms_topn=100)
    assert det2.last_fallback == []
    for n in (0, 2):
        assert counts2[n] == counts[n] and np.array_equal(dets2[n].view(np.int32), dets[n].view(np.int32)), n
    B.assert_same((dets2, counts2), oracle_logits(bad, deltas, pre_nms_topn=100), "non-finite")
    assert np.isfinite(dets2[1, :counts2[1]]).all()


def test_from_logits_repeatable_and_independent_of_workspace_contents():
    from ssad_amd.roi_data.retinanet import BatchedRetinanetDetector
    logits, deltas = logit_maps(9937, B.PLANTED)
    dx, dd = [B.dev(x) for x in logits], [B.dev(d) for d in deltas]
    kw = dict(pre_nms_topn=100, soft_nms=dict(method="gaussian"), bbox_vote=dict(vote_th=0.3, scoring_method="IOU_AVG"))
    det = BatchedRetinanetDetector(N, SHAPES, softmax=True, fused_logits=True, **kw)
    runs = []
    for junk in (False, False, True):
        if junk:
            for t in (det.ws, det.out.view(torch.uint8), det.counts.view(torch.uint8), det.overflow.view(torch.uint8)):
                t.fill_(0xFF)
        dets, counts = det(dx, dd, *SIZES, from_logits=True)
        assert det.last_fallback == []
        runs.append((dets.cpu().numpy().copy(), counts.cpu().numpy().copy()))
    B.assert_same(runs[1], runs[0], "second call")
    B.assert_same(runs[2], runs[0], "junk workspace")
    B.assert_same(runs[0], oracle_logits(logits, deltas, **kw), "oracle")


# ---------------------------------------------------------------------------------------------------------------------
# 10: isolation
# ---------------------------------------------------------------------------------------------------------------------

def test_guarded_detect_batch_ex_from_logits_with_soft_nms_and_voting(K, monkeypatch):
    cfg = B.cfg4()
    from ssad_amd.modeling.generate_anchors import cell_anchors
    logits, deltas = logit_maps(9938, [[60, 9, 0], [45, 0, 0], [50, 20, 0]], shapes=ODD_SHAPES, n_cls=3, cap=64)
    levels, A, Cn, topn, cap, keep = len(ODD_SHAPES), 9, 3, 40, 64, 50
    cells = np.ascontiguousarray(np.asarray(cell_anchors(cfg), np.float64)[:levels])
    L = K.lib()
    IntArr, PtrArr = C.c_int * levels, C.c_void_p * levels
    H, W = IntArr(*[h for h, _ in ODD_SHAPES]), IntArr(*[w for _, w in ODD_SHAPES])
    post = K.DetectPost(nms_method=K.NMS_METHODS["linear"], sigma=0.5, score_thresh=0.0001, vote=1, vote_thresh=0.3,
                        scoring_method=K.VOTE_SCORING["AVG"], beta=1.0)
    nb = int(L.ssad_retinanet_detect_batch_ex_workspace_bytes(N, levels, A, Cn, H, W, topn, cap, C.byref(post)))
    assert nb > int(L.ssad_retinanet_detect_batch_workspace_bytes(N, levels, A, Cn, H, W, topn, cap)) > 0

    def fn(al):
        dc = al.inp("cells", cells)
        tx = [al.inp("logits%d" % l, a) for l, a in enumerate(logits)]
        td = [al.inp("delta%d" % l, a) for l, a in enumerate(deltas)]
        dets, counts, over = al.out("dets", (N, keep, 6)), al.out("counts", (N,), I32), al.out("overflow", (N,), I32)
        ws = al.ws(nb, "detect_batch_ex")
        assert ws.numel() == nb
        rc = L.ssad_retinanet_detect_batch_ex(
            PtrArr(*[t.data_ptr() for t in tx]), PtrArr(*[t.data_ptr() for t in td]), B.p(dc), N, levels, A, Cn, 3, H, W,
            0.05, topn, cap, 0.5, keep, (C.c_float * N)(*ODD_SIZES[2]), (C.c_int * N)(*ODD_SIZES[0]),
            (C.c_int * N)(*ODD_SIZES[1]), B.XFORM_CLIP, 0, B.p(dets), B.p(counts), B.p(over), B.p(ws), nb, K._stream(),
            C.byref(post), 1)
        assert rc == 0, rc
        return dict(dets=dets, counts=counts, overflow=over)

    # isolated() asserts: guards intact, inputs bit-identical, outputs fully written, equal to the ordinary-allocation run
    got = isolated(K, monkeypatch, fn)
    assert not got["overflow"].any()
    want = oracle_logits(logits, deltas, shapes=ODD_SHAPES, keep=keep, sizes=ODD_SIZES, cfg=cfg, pre_nms_topn=topn,
                         soft_nms=dict(method="linear"), bbox_vote=dict(vote_th=0.3, scoring_method="AVG"))
    B.assert_same((got["dets"], got["counts"]), want, "guarded")
    for n in range(N):
        assert got["counts"][n] > 0 and not got["dets"][n, got["counts"][n]:].view(np.int32).any()


# ---------------------------------------------------------------------------------------------------------------------
# 12: the native softmax heads
# ---------------------------------------------------------------------------------------------------------------------

def test_with_the_native_softmax_heads_and_the_labeler():
    """DistillHeads(softmax) leaves cls_logits / bbox_pred for the minibatch on the device, as
    test_gpu_softmax_step.py hands them to RetinanetDetector: the batched detector on them equals the per-image one
    on their slices, and its pseudo-labels feed the labeller"""
    from ssad_amd import synth
    from ssad_amd.head_pipeline import DistillHeads
    from ssad_amd.modeling import retinanet_heads as rh
    from ssad_amd.roi_data.retinanet import BatchedRetinanetDetector, RetinanetDetector, RetinanetLabeler
    n_img, HW = 2, (128, 128)
    shapes = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    rng = np.random.default_rng(9939)
    cfg = rh.HeadConfig(softmax=True, num_gpus=1)
    S = synth.head_params(rng, C=cfg.num_classes)
    b = np.zeros((9, 81), np.float32)
    b[:, 0], b[:, 5], b[:, 33] = 2.0, 3.0, 2.5                    # two classes that score above the detector's threshold
    S["retnet_cls_pred_fpn3_b"] = b.reshape(-1)
    labs = [synth.distill_inputs(rng, n_img, 9, 80, h, w)[2] for h, w in shapes]
    tg = [synth.bbox_targets(rng, l) for l in labs]
    fg = np.array([max(1, sum(t[0].shape[0] for t in tg))], np.float32)
    heads = DistillHeads(cfg, N=n_img, shapes=shapes, device=torch.device("cuda", 0), student_init=S, distill=False)
    heads.step([B.dev(a) for a in synth.fpn_features(rng, n_img, shapes)], None, [B.dev(a) for a in labs], update=False,
               bbox_targets=[(B.dev(y), B.dev(l)) for y, l in tg], fg_num=B.dev(fg))
    logits, deltas = [x.contiguous() for x in heads.cls_logits], [x.contiguous() for x in heads.bbox_pred]
    assert all(tuple(x.shape) == (n_img, 9 * 81, h, w) for x, (h, w) in zip(logits, shapes))
    sizes = ([128, 120], [128, 110], [1.0, 0.875])
    det = BatchedRetinanetDetector(n_img, shapes, softmax=True, candidate_capacity=1 << 14)
    fused = BatchedRetinanetDetector(n_img, shapes, softmax=True, candidate_capacity=1 << 14, fused_logits=True)
    dets, counts = det(logits, deltas, *sizes, from_logits=True)
    fd, fc = fused(logits, deltas, *sizes, from_logits=True)
    assert det.last_fallback == [] and fused.last_fallback == []
    single = RetinanetDetector(shapes, softmax=True)
    for n in range(n_img):
        rows = single([t[n:n + 1] for t in logits], [t[n:n + 1] for t in deltas], sizes[0][n], sizes[1][n], sizes[2][n],
                      from_logits=True)
        assert rows.shape[0] == int(counts[n]) > 0
        assert torch.equal(dets[n, :rows.shape[0]].view(I32), rows.view(I32)), n
        assert not dets[n, rows.shape[0]:].view(I32).any()
        assert int(fc[n]) == rows.shape[0] and torch.equal(fd[n, :rows.shape[0]].view(I32), rows.view(I32)), n
    gb, gc, gn = det.pseudo_labels(dets, counts, sizes[2], 0.1, 8)
    assert int(gn.min()) > 0
    blobs = RetinanetLabeler(n_img, 8, HW[0], HW[1])(gb, gc, gn)
    assert float(blobs["retnet_fg_num"][0]) > 0
