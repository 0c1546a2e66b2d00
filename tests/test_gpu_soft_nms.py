"""Soft-NMS and box voting on the device (csrc/kernels/soft_nms.hip, utils/boxes.py, RetinanetDetector's soft_nms /
bbox_vote options) against tests/golden/soft_nms_ref.npz, which the reference's own text wrote
(tests/golden/make_soft_nms_golden.py)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SCORING = ("ID", "TEMP_AVG", "AVG", "IOU_AVG", "GENERALIZED_AVG", "QUASI_SUM")      # the fixture's numbering
METHODS = {0: "hard", 1: "linear", 2: "gaussian"}                                   # the reference's numbering
SHAPES = [(20, 28), (10, 14), (5, 7)]
GAUSS_TOL = 1e-4       # relative: decayed gaussian scores (expf), and what the detector builds from them
VOTE_TOL = 1e-4        # voted boxes (relative + of the largest coordinate) and voted scores (relative)


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(HERE, "golden", "soft_nms_ref.npz"))


@pytest.fixture(scope="module")
def B():
    import ssad_amd  # noqa: F401
    from ssad_amd.utils import boxes
    return boxes


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def run_case(B, z, v):
    dets = z["soft_dets_%d" % int(z["soft_data"][v])]
    out, keep = B.soft_nms(dev(dets), sigma=float(z["soft_sigma"][v]), overlap_thresh=float(z["soft_nt"][v]),
                           score_thresh=float(z["soft_thresh"][v]), method=METHODS[int(z["soft_method"][v])])
    out, keep = out.cpu().numpy(), keep.cpu().numpy()
    assert out.dtype == np.float32 and np.array_equal(out[:, :4], dets[keep, :4]), v
    return dets, out, keep


def test_linear_and_hard_reproduce_the_reference_bit_for_bit(B, z):
    """1 ... LDS cap + 1 candidates, disjoint boxes below the score threshold, identical boxes, Nt 0.3 and 0.5."""
    cases = [v for v in range(len(z["soft_method"])) if z["soft_method"][v] != 2]
    assert len(cases) >= 30
    for v in cases:
        dets, out, keep = run_case(B, z, v)
        assert np.array_equal(keep, z["soft_keep_%d" % v]), (v, dets.shape[0])
        assert out[:, 4].tobytes() == z["soft_scores_%d" % v].tobytes(), (v, dets.shape[0])


def test_gaussian_same_picks_and_scores_within_parity_tolerance(B, z):
    """At most 63 decays a candidate, each a few 2^-24 off (expf, one multiply; the fixture's exp is numpy's float32
    one): below 2e-5, asserted at the project's 1e-4, a tenth of the fixture's decision margin (>= 1e-3).
    Measured on an MI355X: see DESIGN.md."""
    cases = [v for v in range(len(z["soft_method"])) if z["soft_method"][v] == 2]
    worst = 0.0
    for v in cases:
        _, out, keep = run_case(B, z, v)
        want = z["soft_scores_%d" % v]
        assert np.array_equal(keep, z["soft_keep_%d" % v]), v
        worst = max(worst, float(np.max(np.abs(out[:, 4].astype(np.float64) - want) / want)))
    print("gaussian soft-NMS: max relative score error %.3e over %d cases" % (worst, len(cases)))
    assert worst <= GAUSS_TOL, "max relative error of the decayed scores %.3e" % worst


def raw_soft_nms(dets, cls, classes, method, sigma=0.5, nt=0.3, thresh=0.001):
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd import kernels as K
    L = K.lib()
    n = dets.shape[0]
    boxes, scores, dcls = dev(dets[:, :4]), dev(dets[:, 4]), dev(cls.astype(np.int32))
    keys = torch.full((n,), 7, dtype=torch.int64, device="cuda")
    rank = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(L.ssad_soft_nms_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    rc = L.ssad_soft_nms(K._ptr(boxes), K._ptr(scores), K._ptr(dcls), n, classes, method, sigma, nt, thresh,
                         K._ptr(keys), K._ptr(rank), K._ptr(ws), ws.numel(), K._stream())
    assert rc == 0
    return keys.cpu().numpy(), rank.cpu().numpy()


def test_segmented_entry_with_empty_classes_and_trailing_slots(z):
    """The detector's layout: 6 classes of which 0, 3 and 5 are empty, -1 in the last four slots."""
    dets, cls = z["ms_dets"], z["ms_cls"]
    pos = np.arange(len(cls), dtype=np.int64)
    for name, method in (("linear", 2), ("hard", 1)):               # SSAD_NMS_SOFT_LINEAR, SSAD_NMS_SOFT_HARD
        keys, rank = raw_soft_nms(dets, cls, int(z["ms_classes"]), method)
        want_rank, want_score = z["ms_rank_" + name], z["ms_score_" + name]
        assert np.array_equal(rank, want_rank), name
        live = want_rank >= 0
        assert np.all(keys[~live] == 0)
        assert np.array_equal((keys[live] >> 32).astype(np.int32).view(np.float32), want_score[live])
        assert np.array_equal(keys[live] & 0xffffffff, ~pos[live] & 0xffffffff)


def test_c_abi_argument_checks():
    import ssad_amd  # noqa: F401
    from ssad_amd import kernels as K
    L = K.lib()
    null, one = C.c_void_p(0), C.c_void_p(256)      # never dereferenced: every call returns before a launch
    args = lambda n, m, sigma, nbytes: (one, one, one, n, 1, m, sigma, 0.3, 0.001, one, one, one, nbytes, null)
    assert L.ssad_soft_nms(*args(4, 0, 0.5, 1 << 20)) == -1         # greedy is not a method of this entry
    assert L.ssad_soft_nms(*args(4, 4, 0.5, 1 << 20)) == -1
    assert L.ssad_soft_nms(*args(4, 2, 0.0, 1 << 20)) == -1
    assert L.ssad_soft_nms(*args(-1, 2, 0.5, 1 << 20)) == -1
    assert L.ssad_soft_nms(*args(4, 2, 0.5, 8)) == -2               # SSAD_E_WORKSPACE
    assert L.ssad_soft_nms(*args(0, 2, 0.5, 0)) == 0
    vote = lambda m, scoring, beta: (one, one, m, one, one, one, 4, 1, 0.8, scoring, beta, one, one, null)
    assert L.ssad_box_voting(*vote(4, 6, 1.0)) == -1
    assert L.ssad_box_voting(*vote(4, 4, 0.0)) == -1                # GENERALIZED_AVG: beta is an exponent
    assert L.ssad_box_voting(*vote(-1, 0, 1.0)) == -1
    assert L.ssad_box_voting(*vote(0, 0, 1.0)) == 0


def test_box_voting_matches_the_reference(B, z):
    """Boxes: a float32 weighted mean of <= 400 positive-weight terms errs by at most 400 * 2^-24 = 2.4e-5 of the
    largest coordinate -> rtol 1e-4 + atol 1e-4 * max|coordinate|; scores rtol 1e-4.  The voter sets are exact: the
    generator keeps every IoU 1e-4 away from the threshold."""
    tops, alls = {}, {}
    worst_box, worst_score = 0.0, 0.0
    for k in range(len(z["vote_all"])):
        a, t = int(z["vote_all"][k]), int(z["vote_top"][k])
        if a not in alls:
            alls[a] = dev(z["vote_all_%d" % a])
        if t not in tops:
            tops[t] = dev(z["vote_top_%d" % t])
        want = z["vote_out_%d" % k]
        got = B.box_voting(tops[t], alls[a], float(z["vote_thresh"][k]), SCORING[int(z["vote_scoring"][k])],
                           float(z["vote_beta"][k])).cpu().numpy()
        assert got.shape == want.shape, k
        big = float(np.abs(z["vote_all_%d" % a][:, :4]).max())
        err = np.abs(got[:, :4].astype(np.float64) - want[:, :4])
        worst_box = max(worst_box, float((err / big).max()))
        assert np.all(err <= VOTE_TOL * np.abs(want[:, :4]) + VOTE_TOL * big), (k, float(err.max()), big)
        rel = np.abs(got[:, 4].astype(np.float64) - want[:, 4]) / np.abs(want[:, 4])
        worst_score = max(worst_score, float(rel.max()))
        assert rel.max() <= VOTE_TOL, (k, SCORING[int(z["vote_scoring"][k])], float(rel.max()))
        if SCORING[int(z["vote_scoring"][k])] == "ID":
            assert np.array_equal(got[:, 4], z["vote_top_%d" % t][:, 4])
    print("box voting: max box error %.3e of the largest coordinate, max relative score error %.3e over %d cases" % (
        worst_box, worst_score, len(z["vote_all"])))


def test_equal_scores_come_out_in_input_order(B):
    """The documented tie rule (the reference leaves it to its swap history): among equal current scores the lower
    position is picked first.  Disjoint boxes, so nothing decays."""
    g = np.arange(300)
    dets = np.stack([(g % 20) * 40.0, (g // 20) * 40.0, (g % 20) * 40.0 + 9, (g // 20) * 40.0 + 9,
                     np.where(g % 3 == 0, 0.5, 0.25)], 1).astype(np.float32)
    for method in ("linear", "gaussian", "hard"):
        out, keep = B.soft_nms(dev(dets), method=method)
        assert np.array_equal(keep.cpu().numpy(), np.concatenate([g[g % 3 == 0], g[g % 3 != 0]])), method
        assert np.array_equal(out.cpu().numpy()[:, 4], np.sort(dets[:, 4])[::-1]), method


def test_no_candidates_gives_empty_tensors(B):
    import torch
    empty = torch.zeros((0, 5), dtype=torch.float32, device="cuda")
    out, keep = B.soft_nms(empty)
    assert tuple(out.shape) == (0, 5) and tuple(keep.shape) == (0,)
    assert tuple(B.box_voting(empty, empty, 0.8).shape) == (0, 5)
    assert tuple(B.box_voting(empty, torch.ones((3, 5), device="cuda"), 0.8).shape) == (0, 5)


def detect_inputs(seed=43):
    import torch
    from test_anchor_labels import _detect_inputs
    probs, deltas = _detect_inputs(np.random.default_rng(seed), SHAPES, 19)
    return [torch.as_tensor(p).cuda() for p in probs], [torch.as_tensor(d).cuda() for d in deltas]


def test_detector_without_options_is_the_plain_entry_point():
    """RetinanetDetector(shapes) still calls ssad_retinanet_detect; ssad_retinanet_detect_ex with post == NULL and with
    a greedy / no-vote post struct write the same bytes into a buffer of their own."""
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd import kernels as K
    from ssad_amd.roi_data.retinanet import RetinanetDetector
    probs, deltas = detect_inputs()
    det = RetinanetDetector(SHAPES)
    assert det.post is None
    want = det(probs, deltas, 150, 210, 1.0).cpu().numpy()
    assert 0 < want.shape[0] <= 100
    PtrArr = C.c_void_p * 3
    plain = K.DetectPost(nms_method=0, sigma=0.0, score_thresh=0.0, vote=0, vote_thresh=0.0, scoring_method=0, beta=0.0)
    for post in (None, C.byref(plain)):
        out = torch.full((100, 6), -1.0, dtype=torch.float32, device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        ws = torch.empty_like(det.ws)
        rc = K.lib().ssad_retinanet_detect_ex(
            PtrArr(*[t.data_ptr() for t in probs]), PtrArr(*[t.data_ptr() for t in deltas]), K._ptr(det.cells), 3,
            det.A, det.C, det.cfg.k_min, det._H, det._W, C.c_float(0.05), 1000, C.c_float(0.5), 100, C.c_float(1.0),
            150, 210, C.c_float(float(np.log(1000. / 16.))), K._ptr(out), K._ptr(count), K._ptr(ws),
            C.c_size_t(ws.numel()), K._stream(), post)
        assert rc == 0
        got = out[:int(count.item())].cpu().numpy()
        assert got.tobytes() == want.tobytes()
    # an option struct the library does not know is refused before any launch
    bad = K.DetectPost(nms_method=9, sigma=0.5, score_thresh=0.0, vote=0, vote_thresh=0.0, scoring_method=0, beta=1.0)
    assert K.lib().ssad_retinanet_detect_ex_workspace_bytes(3, det.A, det.C, det._H, det._W, 1000, C.byref(bad)) == 0


@pytest.fixture(scope="module")
def all_candidates():
    """Every candidate of the test image with its class: nms_thresh 2.0 suppresses nothing, dets_per_im = levels * topn
    cuts nothing.  Rows are sorted by score; equal scores keep the order of the class-sorted candidate array."""
    import ssad_amd  # noqa: F401
    from ssad_amd.roi_data.retinanet import RetinanetDetector
    probs, deltas = detect_inputs()
    det = RetinanetDetector(SHAPES, pre_nms_topn=200, nms_thresh=2.0, dets_per_im=600)
    return probs, deltas, det(probs, deltas, 150, 210, 1.0).clone()


@pytest.mark.parametrize("soft,vote", [
    (dict(method="linear"), None),
    (dict(method="gaussian", sigma=0.5), None),
    (dict(method="hard", score_thresh=0.001), dict(vote_th=0.8)),
    (dict(method="linear"), dict(vote_th=0.5, scoring_method="IOU_AVG")),
    (dict(method="gaussian", sigma=0.3), dict(vote_th=0.8, scoring_method="GENERALIZED_AVG", beta=0.5)),
    (None, dict(vote_th=0.8, scoring_method="AVG")),
])
def test_detector_options_equal_the_per_class_composition(B, all_candidates, soft, vote):
    """test.py:779-797 spelled out with utils.boxes on the detector's own candidates, then sorted and cut as
    test_retinanet.py:191-194, against the detector that does it in one call.  Twice on one workspace."""
    import torch
    from ssad_amd.roi_data.retinanet import RetinanetDetector
    probs, deltas, cands = all_candidates
    assert cands.shape[0] > 300
    rows = []                                          # (score, class, position in the class, box)
    for c in torch.unique(cands[:, 5]).cpu().numpy():
        dets_c = cands[cands[:, 5] == float(c)][:, :5].contiguous()
        if soft is not None:
            opts = dict(sigma=0.5, score_thresh=0.0001, method="linear")
            opts.update(soft)
            top, keep = B.soft_nms(dets_c, overlap_thresh=0.5, **opts)
        else:                                          # greedy survivors: what the plain detector keeps of this class
            from oracle import detect as OD
            keep = torch.as_tensor(np.asarray(OD.nms(dets_c.cpu().numpy(), 0.5), np.int64)).cuda()
            top = dets_c[keep]
        if vote is not None:
            top = B.box_voting(top.contiguous(), dets_c, vote["vote_th"], vote.get("scoring_method", "ID"),
                               vote.get("beta", 1.0))
        top, keep = top.cpu().numpy(), keep.cpu().numpy()
        rows += [(-float(top[i, 4]), float(c), int(keep[i]), top[i]) for i in range(len(keep))]
    rows.sort(key=lambda r: r[:3])                     # final score, then class, then position: detect.hip's tie rule
    want = np.array([list(r[3]) + [r[1]] for r in rows[:100]], np.float32)
    det = RetinanetDetector(SHAPES, pre_nms_topn=200, soft_nms=soft, bbox_vote=vote)
    got = det(probs, deltas, 150, 210, 1.0).cpu().numpy()
    assert got.shape == want.shape == (100, 6)
    assert np.array_equal(got[:, 5], want[:, 5])
    exact = (soft is None or soft["method"] != "gaussian")
    if exact:
        assert got.tobytes() == want.tobytes()
    else:
        np.testing.assert_allclose(got[:, 4], want[:, 4], rtol=GAUSS_TOL, atol=0)
        np.testing.assert_allclose(got[:, :4], want[:, :4], rtol=GAUSS_TOL, atol=GAUSS_TOL * 210)
    again = det(probs, deltas, 150, 210, 1.0).cpu().numpy()
    assert again.tobytes() == got.tobytes()


def test_detector_with_options_and_no_candidates():
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd.roi_data.retinanet import RetinanetDetector
    det = RetinanetDetector([(2, 3)], pre_nms_topn=50, dets_per_im=20, soft_nms=dict(method="gaussian"),
                            bbox_vote=dict(scoring_method="AVG"))
    none = det([torch.zeros((1, 720, 2, 3), device="cuda")], [torch.zeros((1, 36, 2, 3), device="cuda")], 64, 64, 1.0)
    assert tuple(none.shape) == (0, 6)
