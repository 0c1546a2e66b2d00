"""The fp32 3x3 launchers give the bits of the commit named in tests/golden/wino_launch_bits.json -- the last one whose
Winograd launchers each planned their passes themselves (csrc/kernels/wino_launch.h plans them for both since): the
F(2x2) and F(2x4) engines through ssad_amd.kernels on a level table that takes every branch of the planner, the F(2x2)
split tail in both of its places, and the table form of the three pack launchers.  sha256 of the raw output words, by
the fixture's own generator (tests/golden/make_wino_launch_bits.py); no case is exempt."""
import json
import os

import pytest

torch = pytest.importorskip("torch")

import make_wino_launch_bits as gen  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pinned(golden_dir):
    return json.load(open(os.path.join(golden_dir, "wino_launch_bits.json")))


def test_fixture_covers_the_cases(pinned):
    assert sorted(pinned["sha256"]) == sorted(c["name"] for c in gen.CASES)
    assert pinned["levels"] == [list(s) for s in gen.MIXED]
    t = pinned["sha256"]
    assert t["tail_replaces_launch_1x8x8"]["launches"] == 1 and t["tail_off_1x128x136"]["launches"] == 1
    for name in ("tail_behind_round_setting2_1x128x136", "tail_behind_round_flag_1x128x136"):
        assert t[name]["launches"] == 2
        assert t[name]["y"] != t["tail_off_1x128x136"]["y"]       # the hash tells the split from the unsplit launch
    assert t["tail_behind_round_setting2_1x128x136"]["y"] == t["tail_behind_round_flag_1x128x136"]["y"]


@pytest.mark.parametrize("case", gen.CASES, ids=lambda c: c["name"])
def test_launchers_give_the_pinned_commits_bits(pinned, case):
    assert torch.cuda.is_available()
    want = pinned["sha256"][case["name"]]
    got = {k: gen.sha_words(v) if hasattr(v, "tobytes") else v for k, v in gen.run_case(case).items()}
    assert sorted(got) == sorted(want)
    wrong = [k for k in got if got[k] != want[k]]
    assert not wrong, "%s: outputs whose words differ from commit %s: %s" % (case["name"], pinned["commit"][:7], wrong)


@pytest.mark.parametrize("engine,route", gen.MASKED_REFUSALS)
def test_masked_table_with_an_empty_level_is_refused_as_before(pinned, engine, route):
    want = pinned["masked_refusals"]["%s_%s" % (engine, route)]
    assert want is not None and "failed with code -1" in want
    assert gen.masked_table_is_refused(engine, route) == want
