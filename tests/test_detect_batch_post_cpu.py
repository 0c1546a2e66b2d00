"""ssad_retinanet_detect_batch_ex / BatchedRetinanetDetector(soft_nms=, bbox_vote=, softmax=) without a device: the
new symbols exist, the workspace grows with the options and with N, inconsistent arguments are refused before a device
is touched, and the Python class checks its options before it calls the library."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

import ssad_amd  # noqa: E402,F401
from ssad_amd import kernels as K  # noqa: E402
from ssad_amd.roi_data.retinanet import BatchedRetinanetDetector  # noqa: E402

SHAPES = [(10, 14), (5, 7), (3, 4), (2, 2), (1, 1)]
LEVELS, A, CLS = 5, 9, 80
IntArr = C.c_int * LEVELS
H, W = IntArr(*[h for h, _ in SHAPES]), IntArr(*[w for _, w in SHAPES])
BADARG, WORKSPACE = -1, -2


def post(method="greedy", sigma=0.5, vote=0, scoring="ID", beta=1.0):
    return K.DetectPost(nms_method=K.NMS_METHODS.get(method, method), sigma=sigma, score_thresh=0.0001, vote=vote,
                        vote_thresh=0.8, scoring_method=K.VOTE_SCORING[scoring], beta=beta)


def plain_bytes(N=3, c=CLS, topn=100, cap=720):
    return int(K.lib().ssad_retinanet_detect_batch_workspace_bytes(N, LEVELS, A, c, H, W, topn, cap))


def ex_bytes(p, N=3, c=CLS, topn=100, cap=720):
    return int(K.lib().ssad_retinanet_detect_batch_ex_workspace_bytes(
        N, LEVELS, A, c, H, W, topn, cap, C.byref(p) if p is not None else None))


def test_abi_version_stays_and_the_new_symbols_resolve():
    L = K.lib()
    assert L.ssad_kernels_abi_version() == 3 == K.ABI_VERSION
    assert L.ssad_retinanet_detect_batch_ex_workspace_bytes and L.ssad_retinanet_detect_batch_ex


def test_workspace_bytes_follow_the_options():
    base = plain_bytes()
    assert base > 0
    assert ex_bytes(None) == base and ex_bytes(post()) == base
    soft, vote, both = ex_bytes(post("linear")), ex_bytes(post(vote=1)), ex_bytes(post("gaussian", vote=1, scoring="AVG"))
    assert soft > base and vote > base and both > base
    # plain + N x what the per-image entry adds for the same options
    one = K.lib().ssad_retinanet_detect_ex_workspace_bytes
    per_image = int(one(LEVELS, A, CLS, H, W, 100, C.byref(post("linear")))) - int(one(LEVELS, A, CLS, H, W, 100, None))
    assert per_image > 0 and soft - base == 3 * per_image
    sizes = [ex_bytes(post("linear"), N=n) for n in (1, 2, 3, 16, 64)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    for bad in (post(4), post(-1), post("linear", sigma=0.0), post("hard", sigma=-1.0), post(vote=1, scoring="QUASI_SUM", beta=0.0)):
        assert ex_bytes(bad) == 0
    bad = post(vote=1)
    bad.scoring_method = 6
    assert ex_bytes(bad) == 0
    assert ex_bytes(post("linear"), N=65) == 0 and ex_bytes(post("linear"), cap=99) == 0


def call_ex(p=None, logits=0, **over):
    """the entry with arguments that are consistent except for `over`; every pointer is a host address the call must
    not follow (there is no device here)"""
    junk = (C.c_double * 16)()
    ptr = C.cast(junk, C.c_void_p)
    ptrs = (C.c_void_p * LEVELS)(*[ptr.value] * LEVELS)
    a = dict(prob=ptrs, delta=ptrs, cells=ptr, N=3, levels=LEVELS, A=A, C=CLS, k_min=3, H=H, W=W, th=0.05, topn=100,
             cap=720, nms=0.5, keep=100, scale=(C.c_float * 3)(1.0, 0.5, 2.0), im_h=(C.c_int * 3)(80, 80, 80),
             im_w=(C.c_int * 3)(112, 112, 112), clip=4.135, cs=0, dets=ptr, counts=ptr, overflow=ptr, ws=ptr,
             ws_bytes=ex_bytes(p), stream=None)
    a.update(over)
    return K.lib().ssad_retinanet_detect_batch_ex(*[a[k] for k in (
        "prob", "delta", "cells", "N", "levels", "A", "C", "k_min", "H", "W", "th", "topn", "cap", "nms", "keep", "scale",
        "im_h", "im_w", "clip", "cs", "dets", "counts", "overflow", "ws", "ws_bytes", "stream")],
        C.byref(p) if p is not None else None, logits)


def test_detect_batch_ex_refuses_bad_arguments_without_a_device():
    big = plain_bytes() * 4
    assert call_ex(logits=2) == BADARG and call_ex(logits=-1) == BADARG
    assert call_ex(post("linear", sigma=0.0), ws_bytes=big) == BADARG
    assert call_ex(post("gaussian", sigma=-0.5), ws_bytes=big) == BADARG
    assert call_ex(post(4), ws_bytes=big) == BADARG and call_ex(post(-1), ws_bytes=big) == BADARG
    assert call_ex(post(vote=1, scoring="TEMP_AVG", beta=0.0), ws_bytes=big) == BADARG
    # logits of 129 classes a cell: past the softmax kernels' limit; 128 foreground classes as scores are fine
    assert call_ex(logits=1, C=128, ws_bytes=plain_bytes(c=128)) == BADARG
    assert call_ex(logits=0, C=128, ws_bytes=plain_bytes(c=128) - 1) == WORKSPACE
    # what the plain entry refuses is refused here
    for over in (dict(prob=None), dict(N=0), dict(N=65), dict(cap=99), dict(keep=0), dict(keep=501), dict(cs=2),
                 dict(scale=(C.c_float * 3)(1.0, 0.0, 1.0)), dict(overflow=None)):
        assert call_ex(post("linear"), **over) == BADARG, over
        assert call_ex(None, logits=1, **over) == BADARG, over


def test_detect_batch_ex_reports_a_short_workspace():
    for p in (post("linear"), post("hard"), post(vote=1), post("gaussian", vote=1, scoring="IOU_AVG")):
        assert call_ex(p, ws_bytes=plain_bytes()) == WORKSPACE            # sized for the plain call
        assert call_ex(p, ws_bytes=ex_bytes(p) - 1) == WORKSPACE
    assert call_ex(None, ws_bytes=plain_bytes() - 1) == WORKSPACE
    assert call_ex(None, logits=1, ws_bytes=plain_bytes() - 1) == WORKSPACE
    assert call_ex(post("linear"), ws=None) == WORKSPACE


# ---------------------------------------------------------------------------------------------------------------------
# the Python class: every check below fails before the library is called
# ---------------------------------------------------------------------------------------------------------------------

def host_detector(**kw):
    return BatchedRetinanetDetector(2, [(2, 3), (1, 1)], pre_nms_topn=10, dets_per_im=5, device="cpu", **kw)


def test_constructor_checks_the_options_before_the_library(monkeypatch):
    monkeypatch.setattr(K, "lib", lambda: pytest.fail("the library was reached"))
    with pytest.raises(K.KernelError, match="unknown soft_nms method"):
        host_detector(soft_nms=dict(method="softer"))
    with pytest.raises(K.KernelError, match="soft_nms options"):
        host_detector(soft_nms=dict(method="linear", Nt=0.3))
    with pytest.raises(K.KernelError, match="bbox_vote options"):
        host_detector(bbox_vote=dict(vote_thresh=0.8))
    with pytest.raises(K.KernelError, match="unknown scoring method"):
        host_detector(bbox_vote=dict(scoring_method="MEDIAN"))
    with pytest.raises(K.KernelError, match="sigma"):
        host_detector(soft_nms=dict(sigma=0.0))
    with pytest.raises(K.KernelError, match="beta"):
        host_detector(bbox_vote=dict(scoring_method="QUASI_SUM", beta=0.0))
    with pytest.raises(K.KernelError, match="booleans"):
        host_detector(softmax=1)


def test_the_options_size_the_workspace():
    plain = host_detector()
    assert plain.post is None and plain.softmax is False
    soft = host_detector(softmax=True)
    assert soft.ws.numel() == plain.ws.numel() and [tuple(t.shape) for t in soft._probs] == [(2, 720, 2, 3), (2, 720, 1, 1)]
    assert host_detector(softmax=True, fused_logits=True)._probs is None and plain._probs is None
    with pytest.raises(K.KernelError, match="boolean"):
        host_detector(softmax=True, fused_logits=1)
    soft = host_detector(soft_nms=dict(method="gaussian", sigma=0.4), bbox_vote=dict(scoring_method="AVG"))
    assert soft.post.nms_method == K.NMS_METHODS["gaussian"] and soft.post.vote == 1
    assert soft.ws.numel() > plain.ws.numel()


def test_call_checks_from_logits_before_the_library(monkeypatch):
    sig, soft = host_detector(), host_detector(softmax=True)
    monkeypatch.setattr(K, "lib", lambda: pytest.fail("the library was reached"))
    sizes = ([16, 16], [24, 24], [1.0, 1.0])
    zeros = lambda ch: [torch.zeros((2, ch, h, w)) for h, w in [(2, 3), (1, 1)]]      # noqa: E731
    with pytest.raises(K.KernelError, match="from_logits=True needs"):
        sig(zeros(729), zeros(36), *sizes, from_logits=True)
    with pytest.raises(K.KernelError, match="booleans"):
        soft(zeros(729), zeros(36), *sizes, from_logits=1)
    with pytest.raises(K.KernelError, match=r"logits must be N x A\*\(C\+1\)"):      # probabilities' channel count
        soft(zeros(720), zeros(36), *sizes, from_logits=True)
    with pytest.raises(K.KernelError, match="cls_prob must be"):                     # logits' channel count
        soft(zeros(729), zeros(36), *sizes)
    with pytest.raises(K.KernelError, match="device tensors"):                       # right shape, host tensors
        soft(zeros(729), zeros(36), *sizes, from_logits=True)
