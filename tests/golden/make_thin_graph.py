#!/usr/bin/env python3
"""Capture what the REFERENCE's builders emit for a thin student (RESNETS.CHANNEL_RATIO < 1):
the ResNet-50-FPN body (detectron/lib/modeling/ResNet.py:88-131 with the ratio at :99-124,
FPN.py:116-250 with it at :122 and :501) and the RetinaNet subnets on the dim the body returns
(retinanet_heads.py:63-245, dim_in).  Settings of configs/model_comp/
retinanet_R-50-FPN_distillation_half.yaml (:34-35 CHANNEL_RATIO: 0.5); 0.25 is the same builder
one halving further.

Runs ONLY in the build container: it imports the reference's modules with the stubs and the
recording models of make_head_graph.py / make_backbone_graph.py, which stay as they are.
Output: tests/golden/thin_graph_r50_fpn_ratio{50,25}.json -- op lists, parameter shapes and
fillers only (data).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_thin_graph.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_head_graph as mh  # noqa: E402
import make_backbone_graph as mb  # noqa: E402

RATIOS = {"thin_graph_r50_fpn_ratio50.json": 0.5, "thin_graph_r50_fpn_ratio25.json": 0.25}


def main():
    mh.install_stubs()
    sys.path.insert(0, mh.REF)
    mb.install_backbone_stubs()
    from core.config import cfg
    import modeling.FPN as FPN
    import modeling.retinanet_heads as rh
    from collections import Counter

    cfg.FPN.FPN_ON = True
    cfg.FPN.MULTILEVEL_RPN = True
    cfg.FPN.RPN_MAX_LEVEL, cfg.FPN.RPN_MIN_LEVEL = 7, 3
    cfg.FPN.COARSEST_STRIDE = 128
    cfg.FPN.EXTRA_CONV_LEVELS = True
    cfg.RETINANET.RETINANET_ON = True
    cfg.RESNETS.TRANS_FUNC = "bottleneck_transformation"
    cfg.NUM_GPUS = 8
    cfg.MODEL.NUM_CLASSES = 81
    cfg.RETINANET.NUM_CONVS = 4
    cfg.RETINANET.ASPECT_RATIOS = (1.0, 2.0, 0.5)
    cfg.RETINANET.SCALES_PER_OCTAVE = 3

    for fname, ratio in RATIOS.items():
        cfg.RESNETS.CHANNEL_RATIO = ratio
        body = mb.RecBackboneModel(train=True)
        blobs, dim, scales = FPN.add_fpn_ResNet50_conv5_body(body)
        heads = mh.RecModel(train=True)
        rh.add_fpn_retinanet_outputs(heads, [str(b) for b in blobs], dim, None)
        out = {
            "config": "configs/model_comp/retinanet_R-50-FPN_distillation_half.yaml (student body + subnets)",
            "channel_ratio": ratio,
            "resnets": {k: getattr(cfg.RESNETS, k) for k in ("STRIDE_1X1", "NUM_GROUPS", "WIDTH_PER_GROUP")},
            "fpn_dim_cfg": int(cfg.FPN.DIM),
            "ops": body.ops,
            "params": body.params,
            "fpn_blobs": [str(b) for b in blobs],
            "fpn_dim": int(dim),
            "spatial_scales": [float(s) for s in scales],
            "op_histogram": dict(Counter(o["type"] for o in body.ops)),
            "head_ops": heads.ops,
            "head_params": heads.params,
        }
        with open(os.path.join(HERE, fname), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
        print(fname, out["op_histogram"], len(body.params), out["fpn_dim"], len(heads.ops), len(heads.params))


if __name__ == "__main__":
    main()
