#!/usr/bin/env python3
"""tests/golden/grouped_grad_ref.npz: the two gradients of the grouped 3x3 convolution through the REFERENCE'S OWN
compiled ConvGradientOp<float, CPUContext> with `group` (oracle.ref_conv_backward on oracle/_ref/libref_conv.so,
which oracle/build_ref_conv.sh builds from the reference's sources).

Runs ONLY in the build container.  The inputs come from make_golden.conv_ref_inputs, so only the seed and the
dimensions are stored; the layout is grouped64_ref.npz's: <name>_dims = (seed, N, Cin, M, H, W, kernel, stride, pad,
group), <name>_dX_idx = up to 4096 sampled flat indices of dX, <name>_dX = the operator's float32 values there,
<name>_dW_idx / <name>_dW likewise for the filter gradient (whole when it has at most 4096 elements).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_grouped_grad_golden.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from oracle import oracle  # noqa: E402

# (name, seed, N, C, H, W, stride, group): cg 4 / stride 2 on an odd map with two images; cg 16 / stride 1 over
# several pixel tiles; cg 64 / stride 1 with ragged 8 x 16 tiles; cg 32 / stride 2 with a ragged half-resolution grid
CASES = [("g8c4s2", 7401, 2, 32, 11, 21, 2, 8), ("g3c16s1", 7402, 1, 48, 12, 24, 1, 3),
         ("g2c64s1", 7403, 1, 128, 9, 19, 1, 2), ("g2c32s2", 7404, 1, 64, 10, 35, 2, 2)]


def main():
    assert oracle.load_ref_conv() is not None, "make -C oracle refconv first"
    out = {}
    for ci, (name, seed, N, Cc, H, W, s, g) in enumerate(CASES):
        X, Wt, _, dY = mg.conv_ref_inputs(seed, N, Cc, Cc, H, W, 3, s, 1, g)
        dW, _, dX = oracle.ref_conv_backward(X, Wt, dY, kernel=3, stride=s, pad=1, group=g)
        srng = np.random.default_rng(7500 + ci)
        for key, arr in (("dX", dX), ("dW", dW)):
            idx = np.sort(srng.choice(arr.size, min(4096, arr.size), replace=False)).astype(np.int64)
            out[name + "_" + key + "_idx"] = idx
            out[name + "_" + key] = arr.ravel()[idx].astype(np.float32)
        out[name + "_dims"] = np.array([seed, N, Cc, Cc, H, W, 3, s, 1, g])
    np.savez_compressed(os.path.join(HERE, "grouped_grad_ref.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
