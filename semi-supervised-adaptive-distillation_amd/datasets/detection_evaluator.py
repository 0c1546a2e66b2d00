"""COCO box evaluation on the device: detections + ground truth -> matches, PR curves, mAP.

The reference's evaluator is detectron/lib/datasets/vid_eval.py (`VIDeval`): the COCO toolbox's `COCOeval` with one
changed line, :286-288, which relaxes the IoU threshold for small ground-truth boxes; vid_dataset_evaluator.py:192-197
drives it for boxes.  `DetectionEvaluator` computes what its evaluate / accumulate / summarize compute for
iouType 'bbox' with useCats = 1: matching, cumulative sums, running maximum and threshold lookup are the kernels of
csrc/kernels/coco_eval.hip; the one global stable ordering between them is torch.sort (plumbing, outside any training
step).  Masks, keypoints, JSON files and dataset catalogues are out of scope.

UNPINNED, both stated from knowledge of the COCO toolbox, neither checked against it (pycocotools and the C module
behind the reference's datasets/mask.py are not available to the fixture generator):
  - the box IoU (float64, xywh, no +1; the union of a crowd ground truth is the detection's area alone);
  - that `small_box_relax=False` (tiou = iou) is the toolbox's `COCOeval`.
`small_box_relax=True` is the reference's file as it stands and is pinned by tests/golden/coco_eval_ref.npz."""
import numpy as np
import torch

from .. import kernels as K

AREA_RNG = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))     # vid_eval.py:514


def _fail(msg):
    raise K.KernelError("DetectionEvaluator: " + msg)


def _int_array(x, name, n):
    a = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)
    if a.dtype.kind not in "iub" or a.shape != (n,):
        _fail("%s must be %d integers" % (name, n))
    return a.astype(np.int64)


def _f64_array(x, name, shape):
    a = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)
    if a.dtype != np.float64 or a.shape != shape:
        _fail("%s must be float64 of shape %r" % (name, shape))
    return np.ascontiguousarray(a)


def _al(n):
    return (int(n) + 255) & ~255


class DetectionEvaluator(object):
    """`add(image_index, dets)` takes RetinanetDetector's [n][6] device rows (x1, y1, x2, y2, score, 1-based class) as
    they are -- no host sync; `add_detections(image_index, boxes_xyxy, scores, categories)` is the general form
    (0-based categories).  Boxes become xywh with w = x2 - x1 + 1 in float32, then widened
    (json_dataset_evaluator.py:179); the detection's area is w*h in float64.  The result does not depend on the order
    of the calls (images are concatenated by index, vid_eval.py:363-375), the order of the rows within an image
    breaks ties of equal scores as in the reference.  An image may be added once, with at most `max_dets_per_image`
    rows.

    `evaluate()` returns precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M] (float64 numpy, -1 where the
    reference leaves -1), stats [12] (summarize's numbers, :463-477; None unless there are the four area ranges, three
    max_dets and .5 / .75 among the thresholds as it assumes) and per_category_ap [K] (the mean of
    precision[:, :, k, 0, -1] over entries > -1, json_dataset_evaluator.py:204-234; -1 without any).  With
    `return_matches=True` also `matches`: cell [C] (image * K + category of every evaluated cell, ascending), offsets
    [C+1], dt_match [A,T,sum D] int32 (index + 1 of the matched ground truth in the cell's given order, 0 for none),
    dt_ignore [A,T,sum D] bool, both per cell in score order cut at max_dets[-1], and npig [C,A]."""

    def __init__(self, num_images, num_categories, gt_boxes_xywh, gt_area, gt_iscrowd, gt_image, gt_category, *,
                 iou_thrs=None, rec_thrs=None, max_dets=(1, 10, 100), area_rng=AREA_RNG, small_box_relax=False,
                 max_dets_per_image=100, device="cuda"):
        # every check comes before the library is touched
        for name, v in (("num_images", num_images), ("num_categories", num_categories),
                        ("max_dets_per_image", max_dets_per_image)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v <= 0:
                _fail("%s must be a positive integer" % name)
        I, Kc, cap = int(num_images), int(num_categories), int(max_dets_per_image)
        if I * Kc >= 2 ** 31 - 1 or I * cap >= 2 ** 31:
            _fail("num_images * num_categories and num_images * max_dets_per_image must stay below 2^31")
        if not isinstance(small_box_relax, (bool, np.bool_)):
            _fail("small_box_relax is a boolean")
        if not hasattr(gt_area, "__len__"):
            _fail("gt_area must be float64 of shape (G,)")
        G = len(gt_area)
        boxes = _f64_array(gt_boxes_xywh, "gt_boxes_xywh", (G, 4))
        area = _f64_array(gt_area, "gt_area", (G,))
        crowd = _int_array(gt_iscrowd, "gt_iscrowd", G)
        image = _int_array(gt_image, "gt_image", G)
        cat = _int_array(gt_category, "gt_category", G)
        if G and (image.min() < 0 or image.max() >= I):
            _fail("gt_image must lie in [0, num_images)")
        if G and (cat.min() < 0 or cat.max() >= Kc):
            _fail("gt_category must lie in [0, num_categories)")
        if G and (crowd.min() < 0 or crowd.max() > 1):
            _fail("gt_iscrowd must be 0 or 1")
        if not (np.all(np.isfinite(boxes)) and np.all(np.isfinite(area))):
            _fail("ground-truth boxes and areas must be finite")
        iou = np.linspace(.5, .95, 10) if iou_thrs is None else np.asarray(iou_thrs)
        rec = np.linspace(0, 1, 101) if rec_thrs is None else np.asarray(rec_thrs)
        if iou.dtype != np.float64 or iou.ndim != 1 or iou.size == 0 or not np.all((iou > 0) & (iou <= 1)):
            _fail("iou_thrs must be a float64 vector of thresholds in (0, 1]")
        if rec.dtype != np.float64 or rec.ndim != 1 or rec.size == 0 or not np.all((rec >= 0) & (rec <= 1)) or \
                np.any(np.diff(rec) < 0):
            _fail("rec_thrs must be an ascending float64 vector of recalls in [0, 1]")
        md = list(max_dets)
        if not md or any(not isinstance(m, (int, np.integer)) or isinstance(m, bool) or m <= 0 for m in md) or \
                any(b <= a for a, b in zip(md, md[1:])):
            _fail("max_dets must be positive integers in ascending order")
        from . import kernels as DK
        if md[-1] > DK.MAX_DETS:
            _fail("max_dets above %d are not supported" % DK.MAX_DETS)
        rng = np.asarray(area_rng, np.float64)
        if rng.ndim != 2 or rng.shape[1] != 2 or rng.shape[0] == 0 or np.any(rng[:, 0] > rng[:, 1]):
            _fail("area_rng must be [A][2] with lo <= hi")
        self.I, self.K, self.cap, self.G = I, Kc, cap, G
        self.T, self.R, self.A, self.M = iou.size, rec.size, rng.shape[0], len(md)
        self.iou_thrs, self.rec_thrs, self.max_dets, self.area_rng = iou.copy(), rec.copy(), md, rng
        self.relax = bool(small_box_relax)
        # ground truth by cell, in the given order within a cell (the order `_gts[image, category]` is filled in)
        order = np.argsort(image * Kc + cat, kind="stable")
        off = np.zeros(I * Kc + 1, np.int64)
        np.cumsum(np.bincount(image * Kc + cat, minlength=I * Kc), out=off[1:])
        dev = torch.device(device)
        to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dt).to(dev)
        self._DK = DK
        self.device = dev
        self.gt_xywh = to(boxes[order], torch.float64)
        self.gt_area = to(area[order], torch.float64)
        self.gt_crowd = to(crowd[order].astype(np.uint8), torch.uint8)
        self.gt_off = to(off, torch.int32)
        self.d_iou, self.d_rec, self.d_rng = to(iou, torch.float64), to(rec, torch.float64), to(rng, torch.float64)
        self.d_max_dets = to(np.asarray(md, np.int32), torch.int32)
        self.det_xywh = torch.zeros((I, cap, 4), dtype=torch.float64, device=dev)
        self.det_score = torch.zeros((I, cap), dtype=torch.float64, device=dev)
        self.det_cat = torch.full((I, cap), -1, dtype=torch.int32, device=dev)
        self.bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self._added = set()

    # ------------------------------------------------------------------ input
    def _image(self, image_index, n):
        if not isinstance(image_index, (int, np.integer)) or isinstance(image_index, bool) or \
                not 0 <= image_index < self.I:
            _fail("image_index must lie in [0, %d)" % self.I)
        if int(image_index) in self._added:
            _fail("image %d was added before" % image_index)
        if n > self.cap:
            _fail("%d detections for image %d exceed max_dets_per_image = %d" % (n, image_index, self.cap))
        return int(image_index)

    def add(self, image_index, dets):
        if not isinstance(dets, torch.Tensor) or dets.dim() != 2 or dets.shape[1] != 6 or \
                dets.dtype != torch.float32 or not dets.is_cuda or (dets.shape[0] and dets.stride(1) != 1):
            _fail("dets must be [n][6] float32 device rows (x1, y1, x2, y2, score, class)")
        n = int(dets.shape[0])
        img = self._image(image_index, n)
        rs = int(dets.stride(0)) if n else 6
        if n and rs < 6:
            _fail("dets rows overlap")
        base = dets.data_ptr()
        col = lambda c: K.C.c_void_p(base + 4 * c) if n else K.C.c_void_p(0)
        K._check(self._DK.lib().ssad_coco_eval_add(
            col(0), rs, col(4), rs, col(5), rs, K.C.c_void_p(0), n, self.cap, self.K, img, K._ptr(self.det_xywh),
            K._ptr(self.det_score), K._ptr(self.det_cat), K._ptr(self.bad), K._stream()), "coco_eval_add")
        self._added.add(img)

    def add_detections(self, image_index, boxes_xyxy, scores, categories):
        def dev(x, dt, shape, name, kinds):
            if isinstance(x, torch.Tensor):
                ok = (x.dtype == dt) if dt == torch.float32 else (not x.dtype.is_floating_point and
                                                                 x.dtype != torch.bool)
                t = x
            else:
                a = np.asarray(x)
                ok = a.dtype.kind in kinds and (dt != torch.float32 or a.dtype == np.float32)
                t = torch.from_numpy(np.ascontiguousarray(a)) if ok else None
            if not ok or tuple(t.shape) != shape:
                _fail("%s must be %s of shape %r" % (name, "float32" if dt == torch.float32 else "integers", shape))
            return t
        n = len(scores)
        b = dev(boxes_xyxy, torch.float32, (n, 4), "boxes_xyxy", "f")
        s = dev(scores, torch.float32, (n,), "scores", "f")
        c = dev(categories, torch.int32, (n,), "categories", "iu")
        img = self._image(image_index, n)
        if not c.is_cuda and n and (int(c.min()) < 0 or int(c.max()) >= self.K):
            _fail("categories must lie in [0, num_categories)")
        b = b.to(self.device).contiguous()
        s = s.to(self.device).contiguous()
        c = c.to(self.device, dtype=torch.int32).contiguous()
        self._DK.coco_eval_add(b, 4, s, 1, None, 0, c, n, self.cap, self.K, img, self.det_xywh, self.det_score,
                               self.det_cat, self.bad)
        self._added.add(img)

    # ------------------------------------------------------------------ evaluation
    def _buffers(self):
        """Everything evaluate() writes on the way lives in the shared, cached workspace: nothing in it is assumed
        to be zero -- the kernels write what they read."""
        DK, n, AT, cells = self._DK, self.I * self.cap, self.A * self.T, self.I * self.K
        parts = [("det_rank", 4 * n, torch.int32), ("dt_match", 4 * n * AT, torch.int32),
                 ("dt_ignore", n * AT, torch.uint8), ("cell_npig", 4 * cells * self.A, torch.int32),
                 ("cell_eval", cells, torch.uint8),
                 ("ws_match", DK.coco_eval_match_workspace_bytes(self.G, self.A, self.T), torch.uint8),
                 ("ws_acc", DK.coco_eval_accumulate_workspace_bytes(self.K, self.A), torch.uint8)]
        buf = K._workspace(sum(_al(nb) for _, nb, _ in parts), "coco_eval")
        out, off = {}, 0
        for name, nb, dt in parts:
            out[name] = buf[off:off + nb].view(dt)
            off += _al(nb)
        return out

    def evaluate(self, return_matches=False, timing=False):
        DK, I, Kc, cap, A, T, M, R = self._DK, self.I, self.K, self.cap, self.A, self.T, self.M, self.R
        w = self._buffers()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if timing else None
        mark = (lambda i: ev[i].record()) if timing else (lambda i: None)
        mark(0)
        DK.coco_eval_match(I, Kc, cap, self.det_xywh, self.det_score, self.det_cat, self.gt_xywh, self.gt_area,
                           self.gt_crowd, self.gt_off, self.G, self.d_iou, T, self.d_rng, A, self.max_dets[-1],
                           self.relax, w["det_rank"], w["dt_match"], w["dt_ignore"], w["cell_npig"], w["cell_eval"],
                           w["ws_match"])
        mark(1)
        # the reference's stable mergesort of the per-image lists concatenated in image order (:363-375), for all
        # categories at once: by (image, rank), then stably by score descending, then stably by category
        rank = w["det_rank"].to(torch.int64)
        live = rank >= 0
        n = I * cap
        slot = torch.arange(n, device=self.device, dtype=torch.int64)
        first = torch.where(live, (slot // cap) * cap + rank, torch.full_like(slot, n))
        perm = torch.sort(first, stable=True)[1]
        perm = perm[torch.sort(-self.det_score.view(-1)[perm], stable=True)[1]]
        key = torch.where(live, self.det_cat.view(-1).to(torch.int64), torch.full_like(slot, Kc))[perm]
        key, idx = torch.sort(key, stable=True)
        perm = perm[idx].contiguous()
        seg = torch.searchsorted(key, torch.arange(Kc + 1, device=self.device, dtype=torch.int64)).contiguous()
        mark(2)
        precision = torch.empty((T, R, Kc, A, M), dtype=torch.float64, device=self.device)
        scores = torch.empty((T, R, Kc, A, M), dtype=torch.float64, device=self.device)
        recall = torch.empty((T, Kc, A, M), dtype=torch.float64, device=self.device)
        DK.coco_eval_accumulate(I, Kc, cap, A, T, M, R, self.d_max_dets, perm, seg, self.det_score, w["det_rank"],
                                w["dt_match"], w["dt_ignore"], w["cell_npig"], w["cell_eval"], self.d_rec, precision,
                                scores, recall, w["ws_acc"])
        mark(3)
        bad = int(self.bad.item())
        if bad:
            _fail("%d added detections carry a category outside [0, num_categories)" % bad)
        res = {"precision": precision.cpu().numpy(), "recall": recall.cpu().numpy(), "scores": scores.cpu().numpy()}
        res["stats"] = self._stats(res["precision"], res["recall"])
        ap = np.full(Kc, -1.0)
        for k in range(Kc):
            s = res["precision"][:, :, k, 0, -1]
            if np.any(s > -1):
                ap[k] = np.mean(s[s > -1])
        res["per_category_ap"] = ap
        if timing:
            torch.cuda.synchronize()
            res["timing_ms"] = {"matching": ev[0].elapsed_time(ev[1]), "ordering": ev[1].elapsed_time(ev[2]),
                                "accumulation": ev[2].elapsed_time(ev[3])}
        if return_matches:
            res["matches"] = self._matches(w)
        return res

    def _stats(self, precision, recall):
        """summarize's _summarizeDets (:432-477)."""
        md = self.max_dets
        if self.A != 4 or self.M != 3:
            return None

        def one(ap, iou_thr=None, a=0, max_det=100):
            mind = [i for i, m in enumerate(md) if m == max_det]
            s = precision if ap else recall
            if iou_thr is not None:
                s = s[np.where(iou_thr == self.iou_thrs)[0]]
            s = s[:, :, :, [a], mind] if ap else s[:, :, [a], mind]
            return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))

        return np.array([one(1), one(1, .5, max_det=md[2]), one(1, .75, max_det=md[2]), one(1, a=1, max_det=md[2]),
                         one(1, a=2, max_det=md[2]), one(1, a=3, max_det=md[2]), one(0, max_det=md[0]),
                         one(0, max_det=md[1]), one(0, max_det=md[2]), one(0, a=1, max_det=md[2]),
                         one(0, a=2, max_det=md[2]), one(0, a=3, max_det=md[2])], np.float64)

    def _matches(self, w):
        A, T, Kc, cap = self.A, self.T, self.K, self.cap
        rank = w["det_rank"].cpu().numpy()
        cat = self.det_cat.view(-1).cpu().numpy()
        slot = np.flatnonzero(rank >= 0)
        cell = (slot // cap) * Kc + cat[slot]
        slot = slot[np.lexsort((rank[slot], cell))]
        cells = np.flatnonzero(w["cell_eval"].cpu().numpy()).astype(np.int32)
        counts = np.bincount((slot // cap) * Kc + cat[slot], minlength=self.I * Kc)[cells]
        idx = torch.from_numpy(slot).to(self.device)
        dtm = w["dt_match"].view(-1, A, T)[idx].cpu().numpy()
        dti = w["dt_ignore"].view(-1, A, T)[idx].cpu().numpy()
        return {"cell": cells, "offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                "dt_match": np.ascontiguousarray(dtm.transpose(1, 2, 0)).astype(np.int32),
                "dt_ignore": np.ascontiguousarray(dti.transpose(1, 2, 0)).astype(bool),
                "npig": w["cell_npig"].view(-1, A).cpu().numpy()[cells].astype(np.int32)}
