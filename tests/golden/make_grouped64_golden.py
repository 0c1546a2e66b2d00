#!/usr/bin/env python3
"""tests/golden/grouped64_ref.npz: the grouped 3x3 convolution with 64 channels per group (ResNeXt-101-32x8d's
res5 layers) through the REFERENCE'S OWN compiled ConvOp<float, CPUContext> (oracle.ref_conv_forward on
oracle/_ref/libref_conv.so, which oracle/build_ref_conv.sh builds from the reference's sources).

Runs ONLY in the build container.  The inputs come from make_golden.conv_ref_inputs, so only the seed and the
dimensions are stored; the layout is conv_ref.npz's: <name>_dims = (seed, N, Cin, M, H, W, kernel, stride, pad,
group), <name>_Y_idx = up to 4096 sampled flat indices, <name>_Y = the operator's float32 outputs there.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_grouped64_golden.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from oracle import oracle  # noqa: E402

# (name, seed, N, Cin, M, H, W, stride, group): ragged 8 x 16 tiles and a second image; an odd map at stride 2
CASES = [("k3g2c64", 6401, 2, 128, 128, 9, 13, 1, 2), ("k3g3c64s2", 6402, 1, 192, 192, 10, 15, 2, 3)]


def main():
    assert oracle.load_ref_conv() is not None, "make -C oracle refconv first"
    out = {}
    for ci, (name, seed, N, Cin, M, H, W, s, g) in enumerate(CASES):
        X, Wt, b, _ = mg.conv_ref_inputs(seed, N, Cin, M, H, W, 3, s, 1, g)
        Y = oracle.ref_conv_forward(X, Wt, b, kernel=3, stride=s, pad=1, group=g)
        srng = np.random.default_rng(6500 + ci)
        idx = np.sort(srng.choice(Y.size, min(4096, Y.size), replace=False)).astype(np.int64)
        out[name + "_Y_idx"] = idx
        out[name + "_Y"] = Y.ravel()[idx].astype(np.float32)
        out[name + "_dims"] = np.array([seed, N, Cin, M, H, W, 3, s, 1, g])
    np.savez_compressed(os.path.join(HERE, "grouped64_ref.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
