"""ctypes binding of the COCO evaluation launchers (include/ssad_kernels.h, csrc/kernels/coco_eval.hip).

The library itself is loaded by ssad_amd.kernels.lib(); this module only declares the prototypes of the
ssad_coco_eval_* entry points on it, once.  No fallback: a launcher that fails raises KernelError."""
import ctypes as C

from .. import kernels as K

MAX_DETS = 1024        # SSAD_COCO_EVAL_MAX_DETS

_declared = False


def lib():
    global _declared
    L = K.lib()
    if not _declared:
        vp, sz, i32, i64 = C.c_void_p, C.c_size_t, C.c_int, C.c_longlong
        L.ssad_coco_eval_add.argtypes = [vp, i32, vp, i32, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
        L.ssad_coco_eval_match_workspace_bytes.restype = sz
        L.ssad_coco_eval_match_workspace_bytes.argtypes = [i64, i32, i32]
        L.ssad_coco_eval_match.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp, i32, vp, i32, i32, i32,
                                           vp, vp, vp, vp, vp, vp, sz, vp]
        L.ssad_coco_eval_accumulate_workspace_bytes.restype = sz
        L.ssad_coco_eval_accumulate_workspace_bytes.argtypes = [i32, i32]
        L.ssad_coco_eval_accumulate.argtypes = [i32, i32, i32, i32, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp,
                                                vp, vp, vp, vp, vp, vp, vp, sz, vp]
        _declared = True
    return L


def coco_eval_add(boxes, box_stride, scores, score_stride, cls1, cls_stride, cats, n, cap, num_categories, image,
                  det_xywh, det_score, det_cat, bad_count):
    K._check(lib().ssad_coco_eval_add(K._ptr(boxes), box_stride, K._ptr(scores), score_stride, K._ptr(cls1),
                                      cls_stride, K._ptr(cats), n, cap, num_categories, image, K._ptr(det_xywh),
                                      K._ptr(det_score), K._ptr(det_cat), K._ptr(bad_count), K._stream()),
             "coco_eval_add")


def coco_eval_match_workspace_bytes(G, A, T):
    return int(lib().ssad_coco_eval_match_workspace_bytes(G, A, T))


def coco_eval_match(I, Kc, cap, det_xywh, det_score, det_cat, gt_xywh, gt_area, gt_crowd, gt_cell_off, G, iou_thrs, T,
                    area_rng, A, max_det, relax, det_rank, dt_match, dt_ignore, cell_npig, cell_eval, ws):
    K._check(lib().ssad_coco_eval_match(
        I, Kc, cap, K._ptr(det_xywh), K._ptr(det_score), K._ptr(det_cat), K._ptr(gt_xywh), K._ptr(gt_area),
        K._ptr(gt_crowd), K._ptr(gt_cell_off), G, K._ptr(iou_thrs), T, K._ptr(area_rng), A, max_det, int(bool(relax)),
        K._ptr(det_rank), K._ptr(dt_match), K._ptr(dt_ignore), K._ptr(cell_npig), K._ptr(cell_eval), K._ptr(ws),
        ws.numel(), K._stream()), "coco_eval_match")


def coco_eval_accumulate_workspace_bytes(Kc, A):
    return int(lib().ssad_coco_eval_accumulate_workspace_bytes(Kc, A))


def coco_eval_accumulate(I, Kc, cap, A, T, M, R, max_dets, perm, seg, det_score, det_rank, dt_match, dt_ignore,
                         cell_npig, cell_eval, rec_thrs, precision, scores, recall, ws):
    K._check(lib().ssad_coco_eval_accumulate(
        I, Kc, cap, A, T, M, R, K._ptr(max_dets), K._ptr(perm), perm.numel(), K._ptr(seg), K._ptr(det_score),
        K._ptr(det_rank), K._ptr(dt_match), K._ptr(dt_ignore), K._ptr(cell_npig), K._ptr(cell_eval), K._ptr(rec_thrs),
        K._ptr(precision), K._ptr(scores), K._ptr(recall), K._ptr(ws), ws.numel(), K._stream()),
        "coco_eval_accumulate")
