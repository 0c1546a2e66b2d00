#!/usr/bin/env python3
"""Capture the operator list the REFERENCE's body builder emits for the ResNeXt-101-32x8d-FPN RetinaNet body
(configs/12_2017_baselines/retinanet_X-101-32x8d-FPN_1x.yaml: RESNETS.STRIDE_1X1 False, NUM_GROUPS 32,
WIDTH_PER_GROUP 8), with the recording model and the stubs of make_backbone_graph.py.

Runs ONLY in the build container (it imports the reference's ResNet.py / FPN.py).
Output: tests/golden/backbone_graph_x101_32x8d_fpn.json (data only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_backbone_graph_32x8d.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_backbone_graph as mb  # noqa: E402

CASES = {
    "backbone_graph_x101_32x8d_fpn.json": (
        "configs/12_2017_baselines/retinanet_X-101-32x8d-FPN_1x.yaml (body)",
        "add_fpn_ResNet101_conv5_body",
        {"STRIDE_1X1": False, "NUM_GROUPS": 32, "WIDTH_PER_GROUP": 8}),
}


if __name__ == "__main__":
    mb.CASES = CASES          # main() walks the module's table: this capture only
    mb.main()
