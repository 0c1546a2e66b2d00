"""The native programs over a matrix of engine switches, launch record by launch record and table by table, equal
the ones recorded in tests/golden/program_fingerprints.json (written by tests/golden/make_program_fingerprints.py at
the commit the file names).  The programs are built over CPU tensors; nothing is launched.  With equal records the
device executes equal launches, so a change to how the pipelines choose engines, pack filters or book timing
classes that is meant to keep behaviour must keep every fingerprint.  To locate a mismatch, diff
`make_program_fingerprints.py --dump NAME` of the two commits."""
import json
import os

import ssad_amd  # noqa: F401
import make_program_fingerprints as mpf


def test_programs_equal_the_recorded_fingerprints(golden_dir):
    with open(os.path.join(golden_dir, "program_fingerprints.json")) as f:
        want = json.load(f)["configurations"]
    got = mpf.fingerprints()
    assert sorted(got) == sorted(want)
    assert len({v[0] for v in want.values()}) >= 38          # the matrix tells the switches apart
    differ = sorted(name for name in want if got[name] != want[name])
    assert not differ, "%d of %d programs differ from the recorded ones (hash, op count): %s" % (
        len(differ), len(want), ", ".join("%s %r != %r" % (n, got[n], want[n]) for n in differ[:6]))
