"""The launch counts of the Winograd F(2x2) engine, as literal tables: ssad_conv3x3_forward_wino_launches and
ssad_conv3x3_forward_wino_launches_for are loops over the launcher's own pass planner and split-tail decision
(csrc/kernels/wino_launch.h).  The tables were recorded from the library of the commit before that header existed,
where the counts were a hand-kept copy of the launcher's arithmetic; host arithmetic only, no device (without one
ssad_cu_count() is 256, an MI355X's)."""
import os

import pytest

import ssad_amd  # noqa: F401
from ssad_amd import kernels as K

MIXED = [(1, 8, 16), (3, 8, 8), (1, 0, 0), (2, 5, 7)]     # patches, pairs with an absent partner, empty, ragged pairs
CASES = [("mixed", MIXED)] + [("%dx%dx%d" % s, [s]) for s in MIXED] + [("16x40x56", [(16, 40, 56)]),
                                                                       ("1x128x136", [(1, 128, 136)])]
CHANNELS = [(36, 20), (136, 20), (136, 64), (256, 256)]
SETTINGS = [0, 1, 2]
FLAGS = [0, K.CONV_SPLIT_TAIL]

# ssad_conv3x3_forward_wino_launches per case
LAUNCHES = {"mixed": 2, "1x8x16": 1, "3x8x8": 1, "1x0x0": 0, "2x5x7": 1, "16x40x56": 1, "1x128x136": 1}
# ssad_conv3x3_forward_wino_launches_for per case: one row per (Cout, Cin) of CHANNELS, in a row setting 0, 1, 2, each
# with flags 0 and SSAD_CONV_SPLIT_TAIL.  A split that replaces the launch (no full round: mixed, 3x8x8, 2x5x7 at 136
# and 256 channels) does not add one; 16x40x56 and 1x128x136 have full rounds, whose tail only setting 2 or the flag
# under setting 1 splits off (136 -> 20 has a single chunk, nothing to cut; 36 channels run the half-block kernels).
ONES, NONE = [1] * 6, [0] * 6
TAIL = [1, 1, 1, 2, 2, 2]
LAUNCHES_FOR = {
    "mixed": [[2] * 6] * 4,
    "1x8x16": [ONES] * 4,
    "3x8x8": [ONES] * 4,
    "1x0x0": [NONE] * 4,
    "2x5x7": [ONES] * 4,
    "16x40x56": [ONES, ONES, TAIL, TAIL],
    "1x128x136": [ONES, ONES, TAIL, TAIL],
}


def levels(shapes):
    arr = (K.ConvLevel * len(shapes))()
    for i, (n, h, w) in enumerate(shapes):
        arr[i].N, arr[i].H, arr[i].W = n, h, w
    return arr


def record():
    L = K.lib()
    plain, rows = {}, {}
    try:
        for name, shapes in CASES:
            arr = levels(shapes)
            plain[name] = L.ssad_conv3x3_forward_wino_launches(arr, len(shapes))
            rows[name] = []
            for cout, cin in CHANNELS:
                row = []
                for s in SETTINGS:
                    L.ssad_conv_wino_split_tail(s)
                    row += [L.ssad_conv3x3_forward_wino_launches_for(arr, len(shapes), cout, cin, f) for f in FLAGS]
                rows[name].append(row)
    finally:
        L.ssad_conv_wino_split_tail(1)
    return plain, rows


def test_launch_counts_are_the_recorded_tables():
    if os.environ.get("SSAD_WINO_PAIRS") or os.environ.get("SSAD_WINO_VARIANT"):
        pytest.skip("geometry forced through the environment")
    plain, rows = record()
    assert plain == LAUNCHES
    assert rows == LAUNCHES_FOR
    assert K.lib().ssad_conv_wino_split_tail(-1) == 1


def test_no_levels_launch_nothing():
    L = K.lib()
    arr = levels(MIXED)
    assert L.ssad_conv3x3_forward_wino_launches(None, 0) == 0
    assert L.ssad_conv3x3_forward_wino_launches(None, 4) == 0
    assert L.ssad_conv3x3_forward_wino_launches(arr, 0) == 0
    for cout, cin in CHANNELS:
        for f in FLAGS:
            assert L.ssad_conv3x3_forward_wino_launches_for(None, 0, cout, cin, f) == 0
            assert L.ssad_conv3x3_forward_wino_launches_for(None, 4, cout, cin, f) == 0
            assert L.ssad_conv3x3_forward_wino_launches_for(arr, 0, cout, cin, f) == 0
