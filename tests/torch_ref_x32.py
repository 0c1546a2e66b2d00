"""tests/torch_ref.RefResNetFPN for ResNeXt-101-32x8d (RESNETS.NUM_GROUPS 32, WIDTH_PER_GROUP 8, STRIDE_1X1 False:
the reference's configs/12_2017_baselines/retinanet_X-101-32x8d-FPN_*.yaml): the same float64 network, built by
torch_ref_thin's width-from-expressions constructor at ratio 1 with this architecture's row added to the table it
reads.  Neither module is edited, and torch_ref.ARCHS itself is left as it is.
"""
import torch_ref_thin
from torch_ref import ARCHS as _BASE

ARCHS = dict(_BASE)
ARCHS["x101-32x8d"] = ((3, 4, 23, 3), 32, 8, False)     # (block counts, groups, width per group, stride on the 1x1)


class RefX32ResNetFPN(torch_ref_thin.RefThinResNetFPN):
    def __init__(self, arch="x101-32x8d", **kw):
        saved = torch_ref_thin.ARCHS
        torch_ref_thin.ARCHS = ARCHS          # the constructor looks its architecture up in its module's table
        try:
            super().__init__(arch, channel_ratio=1.0, **kw)
        finally:
            torch_ref_thin.ARCHS = saved
