"""The activation, gradient and scratch buffers of every backbone of the fingerprint matrix equal the ones recorded in
tests/golden/backbone_buffers.json (written with program_fingerprints.json by tests/golden/make_program_fingerprints.py
at the commit the file names).  A launch record names a buffer that is not in Program.keep only by its order of
appearance, so the fingerprints do not pin a buffer's shape; this does: per backbone the count of its `_bufs` and a
sha256 over the sorted list of their (dtype, shape).  Order of allocation is free.  Built over CPU tensors (the same
builds the fingerprint test uses, made once per session); nothing is launched."""
import json
import os

import ssad_amd  # noqa: F401
import make_program_fingerprints as mpf


def test_backbone_buffers_equal_the_recorded_ones(golden_dir):
    with open(os.path.join(golden_dir, "backbone_buffers.json")) as f:
        want = json.load(f)["configurations"]
    got = mpf.backbone_buffers()
    assert sorted(got) == sorted(want)
    # every configuration that builds a backbone, and both backbones of the fp16 student / teacher pair
    assert len(want) >= 40 and len(want["f16_pair"]) == 2
    differ = sorted(name for name in want if got[name] != want[name])
    assert not differ, "%d of %d backbones differ from the recorded buffers [count, hash]: %s" % (
        len(differ), len(want), ", ".join("%s %r != %r" % (n, got[n], want[n]) for n in differ[:6]))


def test_buffer_record_tells_shapes_and_dtypes_apart():
    import torch

    class Net(object):
        def __init__(self, *bufs):
            self._bufs = list(bufs)
    a, b = torch.empty(2, 3), torch.empty(4, dtype=torch.float16)
    assert mpf.buffer_record(Net(a, b)) == mpf.buffer_record(Net(b, a))                  # order of allocation is free
    assert mpf.buffer_record(Net(a, b)) != mpf.buffer_record(Net(a.t(), b))              # a shape
    assert mpf.buffer_record(Net(a, b)) != mpf.buffer_record(Net(a, b.float()))          # a dtype
    assert mpf.buffer_record(Net(a, b)) != mpf.buffer_record(Net(a, b, b))               # a count
