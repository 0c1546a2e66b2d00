"""Soft-NMS and bounding-box voting on device tensors: the two functions of the reference's
detectron/lib/utils/boxes.py (`soft_nms` :321-338, `box_voting` :262-311) that its test path
(core/test.py:779-797) may apply per class, here on csrc/kernels/soft_nms.hip.

torch is plumbing only (splitting the [n][5] rows, ordering the picks by the rank the kernel wrote); arguments are
checked before the library is touched."""
import ctypes as C

import torch

from .. import kernels as K

SOFT_NMS_METHODS = ("hard", "linear", "gaussian")


def _rows(t, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 5:
        raise K.KernelError("%s must be a tensor [n][5] = x1, y1, x2, y2, score" % name)


def _dets(t, name):
    _rows(t, name)
    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        raise K.KernelError("%s must be a contiguous float32 device tensor" % name)
    return t


def _score_keys(scores):
    """(score bits << 32) | ~position: the survivor word of detect.hip / soft_nms.hip."""
    pos = torch.arange(scores.numel(), dtype=torch.int64, device=scores.device)
    return ((scores.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff) << 32) | (~pos & 0xffffffff)


def _key_scores(keys):
    return (keys >> 32).to(torch.int32).view(torch.float32)


def soft_nms(dets, sigma=0.5, overlap_thresh=0.3, score_thresh=0.001, method='linear'):
    """Returns (dets_out [m][5], keep [m]) in pick order: dets_out[:, 4] are the decayed scores, keep (int64) indexes
    `dets`.  Equal current scores are picked in input order (unspecified in the reference)."""
    if method not in SOFT_NMS_METHODS:
        raise K.KernelError("unknown soft_nms method %r (one of %s)" % (method, ", ".join(SOFT_NMS_METHODS)))
    if not sigma > 0:
        raise K.KernelError("soft_nms: sigma must be positive")
    _dets(dets, "dets")
    n = dets.shape[0]
    if n == 0:
        return dets, torch.empty(0, dtype=torch.int64, device=dets.device)
    L = K.lib()
    boxes, scores = dets[:, :4].contiguous(), dets[:, 4].contiguous()
    cls = torch.zeros(n, dtype=torch.int32, device=dets.device)
    keys = torch.empty(n, dtype=torch.int64, device=dets.device)
    rank = torch.empty(n, dtype=torch.int32, device=dets.device)
    nb = int(L.ssad_soft_nms_workspace_bytes(n))
    ws = K._workspace(nb, "soft_nms")
    K._check(L.ssad_soft_nms(K._ptr(boxes), K._ptr(scores), K._ptr(cls), n, 1, K.NMS_METHODS[method], float(sigma),
                             float(overlap_thresh), float(score_thresh), K._ptr(keys), K._ptr(rank), K._ptr(ws),
                             C.c_size_t(ws.numel()), K._stream()), "soft_nms")
    picked = torch.nonzero(rank >= 0)[:, 0]
    keep = picked[torch.argsort(rank[picked])]
    out = torch.cat([boxes[keep], _key_scores(keys[keep])[:, None]], dim=1)
    return out, keep


def box_voting(top_dets, all_dets, thresh, scoring_method='ID', beta=1.0):
    """`top_dets` [m][5] refined by the votes of `all_dets` [n][5] (IoU >= thresh, weighted by score); returns [m][5].
    A top box that overlaps nothing in `all_dets` keeps its box and score."""
    if scoring_method not in K.VOTE_SCORING:
        raise K.KernelError("unknown scoring method %r (one of %s)" % (scoring_method, ", ".join(K.VOTE_SCORING)))
    if scoring_method in ("TEMP_AVG", "GENERALIZED_AVG", "QUASI_SUM") and not beta > 0:
        raise K.KernelError("box_voting: beta must be positive for %s" % scoring_method)
    _rows(top_dets, "top_dets")
    _rows(all_dets, "all_dets")
    m, n = top_dets.shape[0], all_dets.shape[0]
    if n == 0 and m > 0:
        raise K.KernelError("box_voting: all_dets is empty but top_dets is not")
    _dets(top_dets, "top_dets")
    _dets(all_dets, "all_dets")
    if m == 0:
        return top_dets
    L = K.lib()
    dev = top_dets.device
    top_cls = torch.zeros(m, dtype=torch.int32, device=dev)
    cls = torch.zeros(n, dtype=torch.int32, device=dev)
    top_boxes = top_dets[:, :4].contiguous()
    keys = _score_keys(top_dets[:, 4])
    boxes, scores = all_dets[:, :4].contiguous(), all_dets[:, 4].contiguous()
    voted = torch.empty((m, 4), dtype=torch.float32, device=dev)
    K._check(L.ssad_box_voting(K._ptr(top_boxes), K._ptr(top_cls), m,
                               K._ptr(boxes), K._ptr(scores), K._ptr(cls),
                               n, 1, float(thresh), K.VOTE_SCORING[scoring_method], float(beta), K._ptr(keys),
                               K._ptr(voted), K._stream()), "box_voting")
    return torch.cat([voted, _key_scores(keys)[:, None]], dim=1)
