#!/usr/bin/env python3
"""Capture what the REFERENCE's head builder emits with RETINANET.SHARE_CLS_BBOX_TOWER and
RETINANET.CLASS_SPECIFIC_BBOX (detectron/lib/modeling/retinanet_heads.py:83-85,164-171,214-245): one
capture per switch and one with both on, student (train) and teacher (test mode, under "teacher/")
subnets plus the supervised losses.  Other settings as in make_head_graph.py, whose stubs and
recording model this generator reuses; that file stays as it is.

Runs ONLY in the build container.  Output: tests/golden/head_graph_options.json -- op lists,
parameter shapes and fillers only (data).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_head_graph_options.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_head_graph as mh  # noqa: E402

OUT = os.path.join(HERE, "head_graph_options.json")
CAPTURES = {"shared": (True, False), "class_specific": (False, True), "both": (True, True)}


def main():
    mh.install_stubs()
    sys.path.insert(0, mh.REF)
    from core.config import cfg
    import modeling.retinanet_heads as rh

    cfg.NUM_GPUS = 8
    cfg.MODEL.NUM_CLASSES = 81
    cfg.FPN.RPN_MAX_LEVEL, cfg.FPN.RPN_MIN_LEVEL = 7, 3
    cfg.RETINANET.NUM_CONVS = 4
    cfg.RETINANET.ASPECT_RATIOS = (1.0, 2.0, 0.5)
    cfg.RETINANET.SCALES_PER_OCTAVE = 3
    cfg.RETINANET.LOSS_GAMMA, cfg.RETINANET.LOSS_ALPHA = 2.0, 0.25
    blobs_in = ["fpn_%d" % l for l in range(7, 2, -1)]

    out = {}
    for key, (shared, specific) in CAPTURES.items():
        cfg.RETINANET.SHARE_CLS_BBOX_TOWER = shared
        cfg.RETINANET.CLASS_SPECIFIC_BBOX = specific
        student = mh.RecModel(train=True)
        rh.add_fpn_retinanet_outputs(student, blobs_in, 256, None)
        n_head = len(student.ops)
        loss_grads = rh.add_fpn_retinanet_losses(student)
        teacher = mh.RecModel(train=False, scope="teacher/")
        rh.add_fpn_retinanet_outputs(teacher, ["teacher/" + b for b in blobs_in], 256, None)
        out[key] = {
            "share_cls_bbox_tower": shared,
            "class_specific_bbox": specific,
            "student_ops": student.ops,
            "student_head_op_count": n_head,
            "student_params": student.params,
            "student_losses": student.losses,
            "loss_gradients": {str(k): str(v) for k, v in sorted(loss_grads.items())},
            "teacher_ops": teacher.ops,
        }
        print(key, n_head, len(student.ops), len(student.params), len(teacher.ops))
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
