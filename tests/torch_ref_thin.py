"""tests/torch_ref.RefResNetFPN with the reference's width multiplier (RESNETS.CHANNEL_RATIO): the same
float64 network and `calibrate()`, its widths written out from the reference's expressions
(detectron/lib/modeling/ResNet.py:99-124, FPN.py:122,501; Python's int() truncates) instead of literals.

Strides go by stage index, as in ssad_amd.backbone_pipeline.NativeResNetFPN (at ratio 0.25 the reference's
own `dim_in != 64` test would leave res3_0 at stride 1).  A block has a projection shortcut
where its width or stride changes, so res2.0 of a quarter-width network (64 -> 64) has none.
"""
import numpy as np
import torch

from torch_ref import ARCHS, RefResNetFPN


def reference_widths(r, groups=1, width=64, fpn_dim=256):
    """(inner width per stage, stage outputs, FPN dimension), the reference's expressions verbatim in meaning."""
    dim_bottleneck = int(groups * width * r)                                       # ResNet.py:99
    inner = [dim_bottleneck, dim_bottleneck * 2, dim_bottleneck * 4, dim_bottleneck * 8]
    stage = [int(256 * r), int(512 * r), int(1024 * r), int(2048 * r)]             # ResNet.py:102-118
    return inner, stage, int(fpn_dim * r)                                          # FPN.py:122


class RefThinResNetFPN(RefResNetFPN):
    def __init__(self, arch="r50", channel_ratio=1.0, fpn_dim=256, seed=11, device="cuda", bias_std=0.05,
                 c3_scale=0.25):
        blocks, groups, width, s1x1 = ARCHS[arch]
        inner, stage_out, D = reference_widths(channel_ratio, groups, width, fpn_dim)
        self.arch, self.D, self.device, self.channel_ratio = arch, D, device, channel_ratio
        self.blocks_per_stage, self.groups, self.s1x1 = blocks, groups, s1x1
        gen = torch.Generator().manual_seed(seed)
        self.p, self.scales, self.spec = {}, {}, []

        def add(name, cout, cin_g, k, train, he=True, scale=1.0):
            fan_in = cin_g * k * k
            if he:
                w = torch.randn((cout, cin_g, k, k), generator=gen, dtype=torch.float64) * np.sqrt(2.0 / fan_in) * scale
            else:
                bound = np.sqrt(6.0 / (fan_in + cout * k * k))
                w = (torch.rand((cout, cin_g, k, k), generator=gen, dtype=torch.float64) * 2 - 1) * bound
            b = torch.randn((cout,), generator=gen, dtype=torch.float64) * bias_std
            self.p[name + ".weight"] = w.to(device).requires_grad_(train)
            self.p[name + ".bias"] = b.to(device).requires_grad_(train and not name.startswith(("stem", "res")))
            if scale != 1.0:
                self.scales[name] = scale

        add("stem.0", 64, 3, 7, False)
        cin = 64
        for si, n in enumerate(blocks):
            stage = si + 2
            cmid, cout = inner[si], stage_out[si]
            tr = stage > 2
            for j in range(n):
                stride = 2 if (j == 0 and si > 0) else 1
                pre = "res%d.%d" % (stage, j)
                add(pre + ".c1", cmid, cin, 1, tr)
                add(pre + ".c2", cmid, cmid // groups, 3, tr)
                add(pre + ".c3", cout, cmid, 1, tr, scale=c3_scale)
                proj = cin != cout or stride != 1
                if proj:
                    add(pre + ".proj", cout, cin, 1, tr)
                self.spec.append((pre, cin, cmid, cout, stride, proj, tr))
                cin = cout
        for i, c in enumerate((stage_out[3], stage_out[2], stage_out[1])):
            add("lat.%d" % i, D, c, 1, True, he=False)
        for i in range(3):
            add("out.%d" % i, D, D, 3, True, he=False)
        add("p6", D, stage_out[3], 3, True, he=False)
        add("p7", D, D, 3, True, he=False)
