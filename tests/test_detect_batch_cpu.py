"""ssad_retinanet_detect_batch / ssad_detections_to_gt / BatchedRetinanetDetector without a device: the entry points
refuse inconsistent arguments before they touch one, the workspace size is monotone, the ABI number stays, and the
Python class checks its arguments before it calls the library."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ssad_amd  # noqa: E402,F401
from ssad_amd import kernels as K  # noqa: E402
from ssad_amd.roi_data.retinanet import BatchedRetinanetDetector  # noqa: E402

SHAPES = [(10, 14), (5, 7), (3, 4), (2, 2), (1, 1)]
LEVELS, A, CLS = 5, 9, 80
IntArr = C.c_int * LEVELS
H, W = IntArr(*[h for h, _ in SHAPES]), IntArr(*[w for _, w in SHAPES])
BADARG, WORKSPACE = -1, -2


def ws_bytes(N=3, levels=LEVELS, a=A, c=CLS, h=H, w=W, topn=100, cap=720):
    return int(K.lib().ssad_retinanet_detect_batch_workspace_bytes(N, levels, a, c, h, w, topn, cap))


def test_abi_version_stays():
    assert K.lib().ssad_kernels_abi_version() == 3 == K.ABI_VERSION


def test_workspace_bytes_nonzero_and_monotone():
    base = ws_bytes()
    assert base > 0
    sizes_n = [ws_bytes(N=n) for n in (1, 2, 3, 16, 64)]
    assert sizes_n == sorted(sizes_n) and len(set(sizes_n)) == len(sizes_n)
    sizes_cap = [ws_bytes(cap=c) for c in (100, 101, 720, 4096, 1 << 16)]
    assert sizes_cap == sorted(sizes_cap) and sizes_cap[0] < sizes_cap[-1]
    # the candidate lists are what the capacity buys: 8 bytes a key, per (image, level)
    assert ws_bytes(cap=4096 + 32 * 64) - ws_bytes(cap=4096) == 3 * LEVELS * 32 * 64 * 8


@pytest.mark.parametrize("kw", [
    dict(N=0), dict(N=65), dict(levels=0), dict(levels=9), dict(a=0), dict(c=0), dict(c=0x8000), dict(topn=0),
    dict(topn=4097, cap=8192), dict(cap=99), dict(h=IntArr(10, 5, -1, 2, 1)), dict(h=None),
    dict(N=64, cap=1 << 23),                       # N * levels * cap reaches 2^31
    dict(a=1 << 10, c=1 << 12),                    # a level of 2^29 scores: no index bits left in the key
], ids=lambda kw: ",".join(sorted(kw)))
def test_workspace_bytes_is_zero_for_unsupported_geometry(kw):
    assert ws_bytes(**kw) == 0


def call_batch(**over):
    """the entry with arguments that are consistent except for `over`; every pointer is a host address the call must
    not follow (there is no device here)"""
    junk = (C.c_double * 16)()
    ptr = C.cast(junk, C.c_void_p)
    ptrs = (C.c_void_p * LEVELS)(*[ptr.value] * LEVELS)
    a = dict(prob=ptrs, delta=ptrs, cells=ptr, N=3, levels=LEVELS, A=A, C=CLS, k_min=3, H=H, W=W, th=0.05, topn=100,
             cap=720, nms=0.5, keep=100, scale=(C.c_float * 3)(1.0, 0.5, 2.0), im_h=(C.c_int * 3)(80, 80, 80),
             im_w=(C.c_int * 3)(112, 112, 112), clip=4.135, cs=0, dets=ptr, counts=ptr, overflow=ptr, ws=ptr,
             ws_bytes=ws_bytes(), stream=None)
    a.update(over)
    return K.lib().ssad_retinanet_detect_batch(*[a[k] for k in (
        "prob", "delta", "cells", "N", "levels", "A", "C", "k_min", "H", "W", "th", "topn", "cap", "nms", "keep", "scale",
        "im_h", "im_w", "clip", "cs", "dets", "counts", "overflow", "ws", "ws_bytes", "stream")])


@pytest.mark.parametrize("over", [
    dict(prob=None), dict(delta=None), dict(cells=None), dict(scale=None), dict(im_h=None), dict(im_w=None),
    dict(dets=None), dict(counts=None), dict(overflow=None), dict(H=None),
    dict(prob=(C.c_void_p * LEVELS)(1, 1, 0, 1, 1)),
    dict(N=0), dict(N=65), dict(levels=0), dict(topn=0), dict(cap=99), dict(keep=0), dict(keep=501), dict(cs=2),
    dict(cs=-1), dict(scale=(C.c_float * 3)(1.0, 0.0, 1.0)), dict(scale=(C.c_float * 3)(1.0, float("nan"), 1.0)),
    dict(C=0x8000), dict(topn=4097, cap=8192, keep=100),
], ids=lambda o: ",".join(sorted(o)))
def test_detect_batch_refuses_bad_arguments_without_a_device(over):
    assert call_batch(**over) == BADARG


def test_detect_batch_reports_a_short_workspace():
    assert call_batch(ws_bytes=ws_bytes() - 1) == WORKSPACE
    assert call_batch(ws=None) == WORKSPACE


def test_detections_to_gt_refuses_bad_arguments_without_a_device():
    junk = (C.c_double * 16)()
    ptr = C.cast(junk, C.c_void_p)
    good = dict(dets=ptr, counts=ptr, scale=ptr, N=3, keep=100, th=0.5, gmax=8, gb=ptr, gc=ptr, gn=ptr)
    order = ("dets", "counts", "scale", "N", "keep", "th", "gmax", "gb", "gc", "gn")
    for over in (dict(dets=None), dict(counts=None), dict(scale=None), dict(gb=None), dict(gc=None), dict(gn=None),
                 dict(N=0), dict(keep=0), dict(gmax=0)):
        a = dict(good, **over)
        assert K.lib().ssad_detections_to_gt(*[a[k] for k in order], None) == BADARG, over


# ---------------------------------------------------------------------------------------------------------------------
# the Python class: every check below fails before the library is called (a host-only build of the buffers)
# ---------------------------------------------------------------------------------------------------------------------

def host_detector(**kw):
    return BatchedRetinanetDetector(2, [(2, 3), (1, 1)], pre_nms_topn=10, dets_per_im=5, device="cpu", **kw)


def host_inputs(N=2, ac=720, bc=36, dtype=torch.float32):
    return ([torch.zeros((N, ac, h, w), dtype=dtype) for h, w in [(2, 3), (1, 1)]],
            [torch.zeros((N, bc, h, w), dtype=dtype) for h, w in [(2, 3), (1, 1)]])


def test_capacity_default_and_floor():
    # max(4 * topn, scores of one image on the last level, at most 65536)
    assert host_detector().capacity == 720
    assert BatchedRetinanetDetector(1, [(2, 3)], pre_nms_topn=2000, dets_per_im=5, device="cpu").capacity == 8000
    assert BatchedRetinanetDetector(1, [(20, 30)], pre_nms_topn=100, dets_per_im=5, device="cpu").capacity == 1 << 16
    assert host_detector(candidate_capacity=10).capacity == 10
    with pytest.raises(K.KernelError, match="below pre_nms_topn"):
        host_detector(candidate_capacity=9)
    with pytest.raises(K.KernelError, match="boolean"):
        host_detector(class_specific_bbox=1)
    with pytest.raises(K.KernelError, match="unsupported geometry"):
        BatchedRetinanetDetector(65, [(2, 3)], pre_nms_topn=10, dets_per_im=5, device="cpu")


def test_call_rejects_wrong_inputs_before_the_library(monkeypatch):
    det = host_detector()
    monkeypatch.setattr(K, "lib", lambda: pytest.fail("the library was reached"))
    probs, deltas = host_inputs()
    sizes = ([16, 16], [24, 24], [1.0, 1.0])
    with pytest.raises(K.KernelError, match="device tensors"):          # host tensors
        det(probs, deltas, *sizes)
    with pytest.raises(K.KernelError, match="cls_prob"):                # a wrong batch size
        det(host_inputs(N=1)[0], deltas, *sizes)
    with pytest.raises(K.KernelError, match="cls_prob"):                # a wrong dtype
        det(host_inputs(dtype=torch.float64)[0], deltas, *sizes)
    with pytest.raises(K.KernelError, match="cls_prob"):                # not contiguous
        det([t.transpose(2, 3) for t in host_inputs()[0]], deltas, *sizes)
    with pytest.raises(K.KernelError, match="per level"):
        det(probs[:1], deltas, *sizes)
    with pytest.raises(K.KernelError, match="pseudo|dets must be"):
        det.pseudo_labels(torch.zeros((2, 4, 6)), torch.zeros(2, dtype=torch.int32), [1.0, 1.0], 0.5, 8)


@pytest.mark.gpu
def test_call_rejects_wrong_shapes_on_the_device():
    """the same checks with device tensors, where only the named property is wrong"""
    det = BatchedRetinanetDetector(2, [(2, 3), (1, 1)], pre_nms_topn=10, dets_per_im=5)
    probs, deltas = [[t.cuda() for t in ts] for ts in host_inputs()]
    sizes = ([16, 16], [24, 24], [1.0, 1.0])
    dets, counts = det(probs, deltas, *sizes)
    assert counts.tolist() == [0, 0] and det.last_fallback == []
    with pytest.raises(K.KernelError, match="box_pred"):
        det(probs, [t.cuda() for t in host_inputs(bc=35)[1]], *sizes)
    with pytest.raises(K.KernelError, match="box_pred"):
        det(probs, [t.double() for t in deltas], *sizes)
    with pytest.raises(K.KernelError, match="cls_prob"):
        det([t.cpu() for t in probs], deltas, *sizes)
    with pytest.raises(K.KernelError, match="sequences of N"):
        det(probs, deltas, [16], [24, 24], [1.0, 1.0])
    with pytest.raises(K.KernelError, match="positive"):
        det(probs, deltas, [16, 16], [24, 24], [1.0, 0.0])
    with pytest.raises(K.KernelError, match="counts must be"):
        det.pseudo_labels(dets, counts.long(), [1.0, 1.0], 0.5, 8)
    with pytest.raises(K.KernelError, match="one value per image"):
        det.pseudo_labels(dets, counts, [1.0], 0.5, 8)
    with pytest.raises(K.KernelError, match="Gmax"):
        det.pseudo_labels(dets, counts, [1.0, 1.0], 0.5, 0)
    assert np.isfinite(dets.cpu().numpy()).all()
