"""The convolution operators give the bits of the commit named in tests/golden/conv_operator_bits.json: Conv,
ConvGradient, ConvGroup and ConvGradientGroup on every 3x3 engine the rule of csrc/ops/conv3x3_engine.h can pick, the
`grouped` route, the four float16 routes and the default engine, driven through CreateOperator / RunOperatorOnce /
FetchBlob by the fixture's own generator (tests/golden/make_conv_operator_bits.py), sha256 of the raw output words.
An output the generator found to differ between two runs of that commit ("unstable") is held to the float64
reference at CONV_RTOL / CONV_FLOOR instead.  Then the pack and launch counts of a created Conv / ConvGradient."""
import json
import os

import pytest

torch = pytest.importorskip("torch")

import make_conv_operator_bits as gen  # noqa: E402
from test_gpu_kernels import CONV_FLOOR, CONV_RTOL, close  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pinned(golden_dir):
    return json.load(open(os.path.join(golden_dir, "conv_operator_bits.json")))


@pytest.mark.parametrize("case", gen.CASES, ids=lambda c: c["name"])
def test_operators_give_the_pinned_commits_bits(pinned, case):
    assert torch.cuda.is_available()
    want = pinned["sha256"][case["name"]]
    got = gen.run_case(case)
    assert sorted(got) == sorted(want)
    wrong = []
    for name, arr in got.items():
        if want[name] == "unstable":
            close(arr, gen.reference(case, name), CONV_RTOL, CONV_FLOOR, case["name"] + " " + name)
        elif gen.sha_words(arr) != want[name]:
            wrong.append(name)
    assert not wrong, "%s: outputs whose words differ from commit %s: %s" % (case["name"], pinned["commit"][:7], wrong)


def test_pack_and_launch_counts_of_created_operators(pinned):
    """hip_algo = split, 256 -> 256: a created Conv packs once and launches once a run, a created ConvGradient packs
    once (the data gradient's layout) and launches twice a run (filter gradient, data gradient)."""
    want = pinned["counters"]
    assert want == {"Conv": [{"filter_packs": 1, "conv_launch_calls": 1}, {"filter_packs": 0, "conv_launch_calls": 1}],
                    "ConvGradient": [{"filter_packs": 1, "conv_launch_calls": 2},
                                     {"filter_packs": 0, "conv_launch_calls": 2}]}
    assert gen.run_counters() == want
