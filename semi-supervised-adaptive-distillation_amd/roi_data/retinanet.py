"""RetinaNet training blobs computed on the GPU (row f4): the device replacement of
`add_retinanet_blobs` (detectron/lib/roi_data/retinanet.py:97-196)."""
import ctypes as C

import numpy as np
import torch

from .. import kernels as K
from ..modeling.generate_anchors import AnchorConfig, cell_anchors, field_sizes


class RetinanetLabeler(object):
    """Pre-allocates everything once; `__call__` labels one minibatch.

    gt_boxes  float32 [N][Gmax][4] device (x1, y1, x2, y2 in blob pixels, already scaled)
    gt_classes int32  [N][Gmax] device, gt_counts int32 [N] device
    Returns a dict with the reference's blob names (labels / locs / targets per
    level, `retnet_fg_num`, `retnet_bg_num`); the list tensors are views of
    length M (one host sync to read the five counts).

    class_specific_bbox (None: cfg.class_specific_bbox; RETINANET.CLASS_SPECIFIC_BBOX): column 1 of
    `retnet_roi_fg_bbox_locs_fpn{l}` is 4 * (label - 1) + 4 * (num_classes - 1) * anchor instead of
    4 * anchor (retinanet.py:140-151,288-293)."""

    def __init__(self, N, Gmax, im_height, im_width, cfg=AnchorConfig, capacity=1 << 16,
                 device="cuda", class_specific_bbox=None):
        self.cfg, self.N, self.Gmax, self.capacity = cfg, N, Gmax, capacity
        if class_specific_bbox is None:
            class_specific_bbox = getattr(cfg, "class_specific_bbox", False)
        if not isinstance(class_specific_bbox, (bool, np.bool_)):
            raise K.KernelError("class_specific_bbox= is a boolean")
        self.class_specific_bbox = bool(class_specific_bbox)
        self.levels = cfg.k_max - cfg.k_min + 1
        self.A = cfg.scales_per_octave * len(cfg.aspect_ratios)
        self.fs = field_sizes(cfg)
        self.h = [int(im_height / float(2 ** l)) for l in range(cfg.k_min, cfg.k_max + 1)]
        self.w = [int(im_width / float(2 ** l)) for l in range(cfg.k_min, cfg.k_max + 1)]
        self.cells = torch.as_tensor(cell_anchors(cfg), dtype=torch.float64, device=device)
        self.labels = [torch.empty((N, self.A, h, w), dtype=torch.int32, device=device)
                       for h, w in zip(self.h, self.w)]
        self.locs = [torch.empty((capacity, 4), dtype=torch.float32, device=device)
                     for _ in range(self.levels)]
        self.targets = [torch.empty((capacity, 4), dtype=torch.float32, device=device)
                        for _ in range(self.levels)]
        self.counts = torch.zeros(self.levels, dtype=torch.int32, device=device)
        self.fg_bg = torch.zeros(2, dtype=torch.float32, device=device)
        L = K.lib()
        IntArr = C.c_int * self.levels
        self._fs, self._h, self._w = IntArr(*self.fs), IntArr(*self.h), IntArr(*self.w)
        L.ssad_retinanet_anchor_labels_workspace_bytes.restype = C.c_size_t
        nb = L.ssad_retinanet_anchor_labels_workspace_bytes(self.levels, self.A, cfg.k_min,
                                                            self._fs, N, Gmax)
        self.ws = torch.empty(max(int(nb), 1), dtype=torch.uint8, device=device)
        PtrArr = C.c_void_p * self.levels
        self._labels = PtrArr(*[t.data_ptr() for t in self.labels])
        self._locs = PtrArr(*[t.data_ptr() for t in self.locs])
        self._targets = PtrArr(*[t.data_ptr() for t in self.targets])

    def __call__(self, gt_boxes, gt_classes, gt_counts):
        cfg = self.cfg
        for t, dt in ((gt_boxes, torch.float32), (gt_classes, torch.int32), (gt_counts, torch.int32)):
            if t.dtype != dt or not t.is_contiguous() or not t.is_cuda:
                raise K.KernelError("ground truth must be contiguous device tensors (f32, i32, i32)")
        if tuple(gt_boxes.shape) != (self.N, self.Gmax, 4):
            raise K.KernelError("gt_boxes must be N x Gmax x 4")
        args = (
            C.c_void_p(self.cells.data_ptr()), self.levels, self.A, cfg.k_min, self._fs, self._h,
            self._w, C.c_void_p(gt_boxes.data_ptr()), C.c_void_p(gt_classes.data_ptr()),
            C.c_void_p(gt_counts.data_ptr()), self.N, self.Gmax, cfg.num_classes,
            C.c_float(cfg.positive_overlap), C.c_float(cfg.negative_overlap), self._labels,
            self._locs, self._targets, self.capacity, C.c_void_p(self.counts.data_ptr()),
            C.c_void_p(self.fg_bg.data_ptr()), C.c_void_p(self.ws.data_ptr()),
            C.c_size_t(self.ws.numel()), K._stream())
        if self.class_specific_bbox:
            rc = K.lib().ssad_retinanet_anchor_labels_ex(*args, 1)
        else:
            rc = K.lib().ssad_retinanet_anchor_labels(*args)
        if rc:
            raise K.KernelError("retinanet_anchor_labels failed (%d)" % rc)
        counts = self.counts.cpu().numpy()
        if int(counts.max(initial=0)) > self.capacity:
            raise K.KernelError("foreground list capacity %d exceeded (%d)" %
                                (self.capacity, int(counts.max())))
        blobs = {"retnet_fg_num": self.fg_bg[0:1], "retnet_bg_num": self.fg_bg[1:2]}
        for i, lvl in enumerate(range(cfg.k_min, cfg.k_max + 1)):
            m = int(counts[i])
            blobs["retnet_cls_labels_fpn%d" % lvl] = self.labels[i]
            blobs["retnet_roi_fg_bbox_locs_fpn%d" % lvl] = self.locs[i][:m]
            blobs["retnet_roi_bbox_targets_fpn%d" % lvl] = self.targets[i][:m]
        return blobs


class RetinanetDetector(object):
    """Device replacement of `im_detect_bbox`'s post-processing
    (detectron/lib/core/test_retinanet.py:108-206) for one image.

    `__call__(cls_probs, box_preds, im_height, im_width, im_scale)` takes the per-level
    sigmoid scores [1][A*C][H][W] and box deltas [1][A*4][H][W] (device tensors) and
    returns float32 [n <= dets_per_im][6] = x1, y1, x2, y2, score, class.

    The reference's two post-processing options (core/test.py:779-797), both None by default:
    `soft_nms` = dict(method='linear' | 'gaussian' | 'hard', sigma=0.5, score_thresh=0.0001) replaces the greedy NMS
    by Soft-NMS (TEST.SOFT_NMS; the overlap threshold stays `nms_thresh`, test.py:783); `bbox_vote` =
    dict(vote_th=0.8, scoring_method='ID', beta=1.0) refines every survivor by box voting (TEST.BBOX_VOTE).  The
    output is sorted by the final scores and cut at dets_per_im as before.

    `softmax=True` is the RETINANET.SOFTMAX head (test_retinanet.py:123-124 drops the background column before
    the top-k): `__call__` then takes either the foreground probabilities [1][A*C][H][W] as above, or, with
    `from_logits=True`, the raw cls_pred logits [1][A*(C+1)][H][W] (background first in every anchor's group),
    which it turns into the former with kernels.group_spatial_softmax(drop_background=True) in buffers
    allocated here.

    `class_specific_bbox=True` is the RETINANET.CLASS_SPECIFIC_BBOX head: box deltas are [1][A*4*C][H][W] and a
    candidate (anchor a, class c, y, x) takes its four deltas from channels a*4*C + 4*c + k, the layout the
    training loss addresses (RetinanetLabeler(class_specific_bbox=True)).  The reference's own test path cannot
    run such a head (test_retinanet.py:120-121 reshapes box_pred to (N, A, 4, H, W)); DESIGN.md lists this
    as UNPINNED."""

    def __init__(self, level_shapes, cfg=AnchorConfig, inference_th=0.05, pre_nms_topn=1000,
                 nms_thresh=0.5, dets_per_im=100, device="cuda", *, soft_nms=None, bbox_vote=None, softmax=False,
                 class_specific_bbox=False):
        self.post = self._post(soft_nms, bbox_vote)
        self.softmax = self._softmax_args(softmax, False)
        if not isinstance(class_specific_bbox, (bool, np.bool_)):
            raise K.KernelError("class_specific_bbox= is a boolean")
        self.class_specific_bbox = bool(class_specific_bbox)
        self.cfg = cfg
        self.levels = len(level_shapes)
        self.A = cfg.scales_per_octave * len(cfg.aspect_ratios)
        self.C = cfg.num_classes - 1
        self.th, self.topn, self.nms, self.keep = inference_th, pre_nms_topn, nms_thresh, dets_per_im
        self.cells = torch.as_tensor(cell_anchors(cfg)[:self.levels], dtype=torch.float64,
                                     device=device).contiguous()
        IntArr = C.c_int * self.levels
        self._H = IntArr(*[h for h, _ in level_shapes])
        self._W = IntArr(*[w for _, w in level_shapes])
        self.shapes = list(level_shapes)
        L = K.lib()
        L.ssad_retinanet_detect_workspace_bytes.restype = C.c_size_t
        if self.post is None:
            nb = L.ssad_retinanet_detect_workspace_bytes(self.levels, self.A, self.C, self._H, self._W,
                                                         self.topn)
        else:
            nb = L.ssad_retinanet_detect_ex_workspace_bytes(self.levels, self.A, self.C, self._H, self._W,
                                                            self.topn, C.byref(self.post))
        if nb == 0:
            raise K.KernelError("retinanet_detect: unsupported geometry")
        self.ws = torch.empty(int(nb), dtype=torch.uint8, device=device)
        self.out = torch.zeros((dets_per_im, 6), dtype=torch.float32, device=device)
        self.count = torch.zeros(1, dtype=torch.int32, device=device)
        self._probs = [torch.empty((1, self.A * self.C, h, w), dtype=torch.float32, device=device)
                       for h, w in level_shapes] if self.softmax else None

    @staticmethod
    def _softmax_args(softmax, from_logits):
        """Checks the softmax= / from_logits= pair before the library is touched; returns bool(softmax)."""
        if not isinstance(softmax, (bool, np.bool_)) or not isinstance(from_logits, (bool, np.bool_)):
            raise K.KernelError("softmax= and from_logits= are booleans")
        if from_logits and not softmax:
            raise K.KernelError("from_logits=True needs a detector built with softmax=True (a sigmoid head's "
                                "scores come from the cls_pred convolution's fused Sigmoid)")
        return bool(softmax)

    @staticmethod
    def _post(soft_nms, bbox_vote):
        """The ssad_detect_post of the two option dicts, or None for the plain greedy path; checked before the
        library is touched."""
        if soft_nms is None and bbox_vote is None:
            return None
        post = K.DetectPost(nms_method=K.NMS_METHODS["greedy"], sigma=0.5, score_thresh=0.0001, vote=0,
                            vote_thresh=0.8, scoring_method=K.VOTE_SCORING["ID"], beta=1.0)
        if soft_nms is not None:
            opts = dict(method="linear", sigma=0.5, score_thresh=0.0001)
            if set(soft_nms) - set(opts):
                raise K.KernelError("soft_nms options: %s" % ", ".join(sorted(opts)))
            opts.update(soft_nms)
            if opts["method"] not in ("hard", "linear", "gaussian"):
                raise K.KernelError("unknown soft_nms method %r" % (opts["method"],))
            if not opts["sigma"] > 0:
                raise K.KernelError("soft_nms: sigma must be positive")
            post.nms_method, post.sigma = K.NMS_METHODS[opts["method"]], opts["sigma"]
            post.score_thresh = opts["score_thresh"]
        if bbox_vote is not None:
            opts = dict(vote_th=0.8, scoring_method="ID", beta=1.0)
            if set(bbox_vote) - set(opts):
                raise K.KernelError("bbox_vote options: %s" % ", ".join(sorted(opts)))
            opts.update(bbox_vote)
            if opts["scoring_method"] not in K.VOTE_SCORING:
                raise K.KernelError("unknown scoring method %r" % (opts["scoring_method"],))
            if opts["scoring_method"] in ("TEMP_AVG", "GENERALIZED_AVG", "QUASI_SUM") and not opts["beta"] > 0:
                raise K.KernelError("bbox_vote: beta must be positive for %s" % opts["scoring_method"])
            post.vote, post.vote_thresh = 1, opts["vote_th"]
            post.scoring_method, post.beta = K.VOTE_SCORING[opts["scoring_method"]], opts["beta"]
        return post

    def __call__(self, cls_probs, box_preds, im_height, im_width, im_scale, *, from_logits=False):
        self._softmax_args(self.softmax, from_logits)
        if from_logits:
            for t, (h, w) in zip(cls_probs, self.shapes):
                if tuple(t.shape) != (1, self.A * (self.C + 1), h, w):
                    raise K.KernelError("cls_pred logits must be 1 x A*(C+1) x H x W")
            cls_probs = [K.group_spatial_softmax(t, self.C + 1, drop_background=True, out=o)
                         for t, o in zip(cls_probs, self._probs)]
        for t, (h, w) in zip(cls_probs, self.shapes):
            if tuple(t.shape) != (1, self.A * self.C, h, w) or t.dtype != torch.float32 or \
                    not t.is_contiguous() or not t.is_cuda:
                raise K.KernelError("cls_prob must be 1 x A*C x H x W contiguous float32 device tensors")
        box_ch = self.A * 4 * (self.C if self.class_specific_bbox else 1)
        for t, (h, w) in zip(box_preds, self.shapes):
            if tuple(t.shape) != (1, box_ch, h, w) or t.dtype != torch.float32 or \
                    not t.is_contiguous() or not t.is_cuda:
                raise K.KernelError("box_pred must be 1 x %s x H x W contiguous float32 device tensors"
                                    % ("A*4*C" if self.class_specific_bbox else "A*4"))
        PtrArr = C.c_void_p * self.levels
        args = (
            PtrArr(*[t.data_ptr() for t in cls_probs]), PtrArr(*[t.data_ptr() for t in box_preds]),
            C.c_void_p(self.cells.data_ptr()), self.levels, self.A, self.C, self.cfg.k_min, self._H,
            self._W, C.c_float(self.th), self.topn, C.c_float(self.nms), self.keep,
            C.c_float(im_scale), int(im_height), int(im_width),
            C.c_float(float(np.log(1000. / 16.))), C.c_void_p(self.out.data_ptr()),
            C.c_void_p(self.count.data_ptr()), C.c_void_p(self.ws.data_ptr()),
            C.c_size_t(self.ws.numel()), K._stream())
        if self.class_specific_bbox:
            rc = K.lib().ssad_retinanet_detect_class_specific(
                *args, C.byref(self.post) if self.post is not None else C.c_void_p(0), 1)
        elif self.post is None:
            rc = K.lib().ssad_retinanet_detect(*args)
        else:
            rc = K.lib().ssad_retinanet_detect_ex(*args, C.byref(self.post))
        if rc:
            raise K.KernelError("retinanet_detect failed (%d)" % rc)
        return self.out[:int(self.count.item())]


class BatchedRetinanetDetector(object):
    """`RetinanetDetector` for a minibatch: N images per call, one kernel sequence whose length does not depend on N
    (ssad_retinanet_detect_batch / ssad_retinanet_detect_batch_ex).

    `__call__(cls_probs, box_preds, im_heights, im_widths, im_scales)` takes the per-level sigmoid scores
    [N][A*C][H][W] and box deltas [N][A*4][H][W] ([N][A*4*C][H][W] with `class_specific_bbox=True`) as device tensors
    -- what DistillHeads leaves in t_prob / t_bbox -- and three host sequences of N.  It returns
    (dets float32 [N][dets_per_im][6], counts int32 [N]): image n's rows are dets[n, :counts[n]], bit for bit the rows
    RetinanetDetector gives on the [n:n+1] slices; rows from counts[n] on are zero.  Both tensors are this object's
    buffers: the next call overwrites them.

    `soft_nms`, `bbox_vote` and `softmax` mean what they mean to RetinanetDetector and are checked the same way:
    Soft-NMS and box voting run for all N images in one launch each.  `softmax=True` takes the foreground
    probabilities [N][A*C][H][W], or, with `__call__(..., from_logits=True)`, the softmax head's cls_pred logits
    [N][A*(C+1)][H][W] (DistillHeads' cls_logits), which one group_spatial_softmax(drop_background=True) launch per
    level turns into the former for the whole batch, in buffers allocated here.  (ssad_retinanet_detect_batch_ex can
    read the logits itself, cls_is_logits = 1; measured, that fused pass was not faster than this route --
    profiles/detect_batch.md; `fused_logits=True` selects it, and then no probability buffer is allocated.)

    Only scores above the threshold become sort keys, in lists of `candidate_capacity` keys per (image, level).  An
    image with a fuller level is reported by the kernels; `__call__` reads those N flags (the one device-to-host copy
    of a call), runs the per-image detector on each flagged image's slices and stores that result in its row:
    `last_fallback` lists them.  So the capacity decides speed, never the result.  The default (None) is
    max(4 * pre_nms_topn, min(scores of one image on the last level, 65536)): the last level's threshold is 0, so on
    sigmoid scores its list holds the whole level.

    `pseudo_labels(dets, counts, im_scales, score_thresh, Gmax)` turns detections into the labeller's ground truth:
    (gt_boxes float32 [N][Gmax][4] in blob pixels, gt_classes int32 [N][Gmax], gt_counts int32 [N]), device tensors
    for RetinanetLabeler.__call__ (ssad_detections_to_gt)."""

    DEFAULT_CAPACITY_LIMIT = 1 << 16

    def __init__(self, N, level_shapes, cfg=AnchorConfig, inference_th=0.05, pre_nms_topn=1000,
                 nms_thresh=0.5, dets_per_im=100, device="cuda", *, class_specific_bbox=False,
                 candidate_capacity=None, soft_nms=None, bbox_vote=None, softmax=False,
                 fused_logits=False):
        self.post = RetinanetDetector._post(soft_nms, bbox_vote)
        self.softmax = RetinanetDetector._softmax_args(softmax, False)
        self._options = dict(soft_nms=soft_nms, bbox_vote=bbox_vote, softmax=self.softmax)
        if not isinstance(fused_logits, (bool, np.bool_)):
            raise K.KernelError("fused_logits= is a boolean")
        self.fused_logits = bool(fused_logits)
        if not isinstance(class_specific_bbox, (bool, np.bool_)):
            raise K.KernelError("class_specific_bbox= is a boolean")
        self.class_specific_bbox = bool(class_specific_bbox)
        self.N, self.cfg, self.device = int(N), cfg, device
        self.shapes = [(int(h), int(w)) for h, w in level_shapes]
        self.levels = len(self.shapes)
        self.A = cfg.scales_per_octave * len(cfg.aspect_ratios)
        self.C = cfg.num_classes - 1
        self.th, self.topn, self.nms, self.keep = inference_th, int(pre_nms_topn), nms_thresh, int(dets_per_im)
        if self.N < 1 or self.levels < 1:
            raise K.KernelError("BatchedRetinanetDetector needs N >= 1 images and at least one level")
        if candidate_capacity is None:
            last = self.A * self.C * self.shapes[-1][0] * self.shapes[-1][1]
            candidate_capacity = max(4 * self.topn, min(last, self.DEFAULT_CAPACITY_LIMIT))
        self.capacity = int(candidate_capacity)
        if self.capacity < self.topn:
            raise K.KernelError("candidate_capacity %d is below pre_nms_topn %d" % (self.capacity, self.topn))
        IntArr = C.c_int * self.levels
        self._H = IntArr(*[h for h, _ in self.shapes])
        self._W = IntArr(*[w for _, w in self.shapes])
        if self.post is None:
            nb = K.lib().ssad_retinanet_detect_batch_workspace_bytes(self.N, self.levels, self.A, self.C, self._H,
                                                                     self._W, self.topn, self.capacity)
        else:
            nb = K.lib().ssad_retinanet_detect_batch_ex_workspace_bytes(self.N, self.levels, self.A, self.C, self._H,
                                                                        self._W, self.topn, self.capacity,
                                                                        C.byref(self.post))
        if nb == 0:
            raise K.KernelError("retinanet_detect_batch: unsupported geometry")
        self.cells = torch.as_tensor(cell_anchors(cfg)[:self.levels], dtype=torch.float64,
                                     device=device).contiguous()
        self.ws = torch.empty(int(nb), dtype=torch.uint8, device=device)
        self.out = torch.zeros((self.N, self.keep, 6), dtype=torch.float32, device=device)
        self.counts = torch.zeros(self.N, dtype=torch.int32, device=device)
        self.overflow = torch.zeros(self.N, dtype=torch.int32, device=device)
        # from_logits=True: the batch's foreground probabilities (group_spatial_softmax writes them, the candidate
        # pass reads them: the fused pass of ssad_retinanet_detect_batch_ex was not faster, profiles/detect_batch.md)
        self._probs = [torch.empty((self.N, self.A * self.C, h, w), dtype=torch.float32, device=device)
                       for h, w in self.shapes] if self.softmax and not self.fused_logits else None
        self.last_fallback = []
        self._single = None

    def _check_inputs(self, cls_probs, box_preds, im_heights, im_widths, im_scales, from_logits=False):
        if len(cls_probs) != self.levels or len(box_preds) != self.levels:
            raise K.KernelError("one cls_prob and one box_pred tensor per level (%d)" % self.levels)
        box_ch = self.A * 4 * (self.C if self.class_specific_bbox else 1)
        cls_ch = self.A * (self.C + 1 if from_logits else self.C)
        for t, (h, w) in zip(cls_probs, self.shapes):
            if tuple(t.shape) != (self.N, cls_ch, h, w) or t.dtype != torch.float32 or \
                    not t.is_contiguous() or not t.is_cuda:
                if from_logits:
                    raise K.KernelError("cls_pred logits must be N x A*(C+1) x H x W contiguous float32 device tensors")
                raise K.KernelError("cls_prob must be N x A*C x H x W contiguous float32 device tensors")
        for t, (h, w) in zip(box_preds, self.shapes):
            if tuple(t.shape) != (self.N, box_ch, h, w) or t.dtype != torch.float32 or \
                    not t.is_contiguous() or not t.is_cuda:
                raise K.KernelError("box_pred must be N x %s x H x W contiguous float32 device tensors"
                                    % ("A*4*C" if self.class_specific_bbox else "A*4"))
        if len(im_heights) != self.N or len(im_widths) != self.N or len(im_scales) != self.N:
            raise K.KernelError("im_heights, im_widths and im_scales are host sequences of N = %d" % self.N)
        if not all(float(s) > 0 for s in im_scales):
            raise K.KernelError("every im_scale must be positive")

    def __call__(self, cls_probs, box_preds, im_heights, im_widths, im_scales, *, from_logits=False):
        RetinanetDetector._softmax_args(self.softmax, from_logits)
        self._check_inputs(cls_probs, box_preds, im_heights, im_widths, im_scales, from_logits)
        PtrArr = C.c_void_p * self.levels
        scores = cls_probs
        if from_logits and not self.fused_logits:
            scores = [K.group_spatial_softmax(t, self.C + 1, drop_background=True, out=o)
                      for t, o in zip(cls_probs, self._probs)]
        args = (
            PtrArr(*[t.data_ptr() for t in scores]), PtrArr(*[t.data_ptr() for t in box_preds]),
            C.c_void_p(self.cells.data_ptr()), self.N, self.levels, self.A, self.C, self.cfg.k_min, self._H, self._W,
            self.th, self.topn, self.capacity, self.nms, self.keep,
            (C.c_float * self.N)(*[float(s) for s in im_scales]), (C.c_int * self.N)(*[int(h) for h in im_heights]),
            (C.c_int * self.N)(*[int(w) for w in im_widths]), float(np.log(1000. / 16.)),
            int(self.class_specific_bbox), C.c_void_p(self.out.data_ptr()), C.c_void_p(self.counts.data_ptr()),
            C.c_void_p(self.overflow.data_ptr()), C.c_void_p(self.ws.data_ptr()), self.ws.numel(), K._stream())
        fused = bool(from_logits and self.fused_logits)
        if self.post is None and not fused:
            rc = K.lib().ssad_retinanet_detect_batch(*args)
        else:
            rc = K.lib().ssad_retinanet_detect_batch_ex(
                *args, C.byref(self.post) if self.post is not None else None, int(fused))
        if rc:
            raise K.KernelError("retinanet_detect_batch failed (%d)" % rc)
        self.last_fallback = [int(n) for n in torch.nonzero(self.overflow).flatten().cpu().numpy()]
        for n in self.last_fallback:
            if self._single is None:
                self._single = RetinanetDetector(self.shapes, self.cfg, self.th, self.topn, self.nms, self.keep,
                                                 self.device, class_specific_bbox=self.class_specific_bbox,
                                                 **self._options)
            # slices of an [N][ch][H][W] tensor are contiguous; the detector's own buffers hold all dets_per_im rows
            self._single([t[n:n + 1] for t in cls_probs], [t[n:n + 1] for t in box_preds],
                         im_heights[n], im_widths[n], im_scales[n], from_logits=from_logits)
            self.out[n].copy_(self._single.out)
            self.counts[n:n + 1].copy_(self._single.count)
        return self.out, self.counts

    def pseudo_labels(self, dets, counts, im_scales, score_thresh, Gmax):
        if tuple(dets.shape) != (self.N, self.keep, 6) or dets.dtype != torch.float32 or not dets.is_contiguous() \
                or not dets.is_cuda:
            raise K.KernelError("dets must be the N x dets_per_im x 6 contiguous float32 device tensor of __call__")
        if tuple(counts.shape) != (self.N,) or counts.dtype != torch.int32 or not counts.is_contiguous() \
                or not counts.is_cuda:
            raise K.KernelError("counts must be the contiguous int32 device tensor [N] of __call__")
        if not torch.is_tensor(im_scales):
            if len(im_scales) != self.N:
                raise K.KernelError("im_scales has one value per image (N = %d)" % self.N)
            im_scales = torch.tensor([float(s) for s in im_scales], dtype=torch.float32, device=dets.device)
        if tuple(im_scales.shape) != (self.N,) or im_scales.dtype != torch.float32 or not im_scales.is_contiguous() \
                or not im_scales.is_cuda:
            raise K.KernelError("im_scales must be N floats (a host sequence or a float32 device tensor)")
        Gmax = int(Gmax)
        if Gmax < 1:
            raise K.KernelError("Gmax must be at least 1")
        gt_boxes = torch.empty((self.N, Gmax, 4), dtype=torch.float32, device=dets.device)
        gt_classes = torch.empty((self.N, Gmax), dtype=torch.int32, device=dets.device)
        gt_counts = torch.empty(self.N, dtype=torch.int32, device=dets.device)
        rc = K.lib().ssad_detections_to_gt(
            C.c_void_p(dets.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(im_scales.data_ptr()), self.N,
            self.keep, float(score_thresh), Gmax, C.c_void_p(gt_boxes.data_ptr()), C.c_void_p(gt_classes.data_ptr()),
            C.c_void_p(gt_counts.data_ptr()), K._stream())
        if rc:
            raise K.KernelError("detections_to_gt failed (%d)" % rc)
        return gt_boxes, gt_classes, gt_counts
