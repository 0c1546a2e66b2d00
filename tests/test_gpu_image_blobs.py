"""ssad_image_blobs / ImageBlobBuilder on the GPU against a numpy restatement of the kernel's definition
(include/ssad_kernels.h): coordinates in float64 cast to float32, weights float32, taps by float32
numpy operations, the interpolation sum in float64.

cv2 is not available to these tests, so bit parity with cv2.resize is UNPINNED: they pin the kernel to the
definition written from cv2's algorithm, not to cv2."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REF_NORM = (1.0, (102.9801, 115.9465, 122.7717), (1.0, 1.0, 1.0))
IMAGENET_NORM = (255.0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
NORMS = (REF_NORM, IMAGENET_NORM)


def taps(im, norm):
    """preprocess_im in float32: ((u8 / div) - mean) / std, [h][w][3]"""
    div, mean, std = norm
    t = im.astype(np.float32) / np.float32(div)
    t = t - np.asarray(mean, np.float32)
    return t / np.asarray(std, np.float32)


def vmax(norm):
    """largest |tap| per channel over u8 0..255"""
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)       # [256][1][3]
    return np.abs(taps(ramp, norm)).max(axis=(0, 1)).astype(np.float64)


def axis(count, scale, length):
    f = ((np.arange(count, dtype=np.float64) + 0.5) * (1.0 / np.float64(scale)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    a = f - s.astype(np.float32)
    assert a.dtype == np.float32
    low, high = s < 0, s >= length - 1
    s[low], a[low] = 0, 0
    s[high], a[high] = length - 1, 0
    return s, np.minimum(s + 1, length - 1), a


def restate(images, flipped, scales, out_hw, blob_hw, norm):
    """float64 [N][3][Hb][Wb] and the mask of the elements inside (oh, ow)"""
    Hb, Wb = blob_hw
    blob = np.zeros((len(images), 3, Hb, Wb), np.float64)
    inside = np.zeros(blob.shape, bool)
    for n, (im, flip, s, (oh, ow)) in enumerate(zip(images, flipped, scales, out_hw)):
        t = taps(im[:, ::-1, :] if flip else im, norm).astype(np.float64)
        sy, sy1, ay = axis(oh, s, im.shape[0])
        sx, sx1, ax = axis(ow, s, im.shape[1])
        bx, by = (np.float32(1) - ax), (np.float32(1) - ay)                           # float32 weights
        ax, bx = ax.astype(np.float64)[None, :, None], bx.astype(np.float64)[None, :, None]
        ay, by = ay.astype(np.float64)[:, None, None], by.astype(np.float64)[:, None, None]
        top = bx * t[sy][:, sx] + ax * t[sy][:, sx1]
        bot = bx * t[sy1][:, sx] + ax * t[sy1][:, sx1]
        blob[n, :, :oh, :ow] = (by * top + ay * bot).transpose(2, 0, 1)
        inside[n, :, :oh, :ow] = True
    return blob, inside


def run_kernel(images, flipped, scales, out_hw, blob_hw, norms):
    """the raw entry point; outputs pre-filled with NaN, so an element the kernel leaves out fails"""
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd import kernels as K
    L = K.lib()
    N, (Hb, Wb) = len(images), blob_hw
    src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).cuda()
    sizes = [im.size for im in images]
    offsets = [int(sum(sizes[:i])) for i in range(N)]
    outs = [torch.full((N, 3, Hb, Wb), float("nan"), dtype=torch.float32, device="cuda") for _ in norms]
    tab = (K.ImageNorm * len(norms))()
    for k, ((div, mean, std), o) in enumerate(zip(norms, outs)):
        tab[k] = K.ImageNorm(div, (C.c_float * 3)(*mean), (C.c_float * 3)(*std), o.data_ptr())
    ws = torch.empty(L.ssad_image_blobs_workspace_bytes(N, Hb, Wb), dtype=torch.uint8, device="cuda")
    ints = lambda v: (C.c_int * N)(*[int(x) for x in v])
    rc = L.ssad_image_blobs(
        src.data_ptr(), src.numel(), (C.c_longlong * N)(*offsets), ints(im.shape[0] for im in images),
        ints(im.shape[1] for im in images), ints(o[0] for o in out_hw), ints(o[1] for o in out_hw),
        (C.c_double * N)(*[float(s) for s in scales]), ints(flipped), N, Hb, Wb, tab, len(norms), ws.data_ptr(),
        ws.numel(), K._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return outs


def assert_padding_is_plus_zero(got, inside, what):
    bits = got.cpu().numpy().view(np.int32)
    assert not bits[~inside].any(), "%s: padding is not +0.0 everywhere" % what


def assert_within_bound(got, want, inside, norm, what):
    """|kernel - restatement| <= 16 * 2^-24 * Vmax per channel: the result is a convex combination of four
    taps of magnitude <= Vmax reached in six float32 roundings (with or without FMA contraction), taps and
    weights being identical on both sides."""
    g = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all(), "%s: an element was not written" % what
    unit = 2.0 ** -24 * vmax(norm)
    err = (np.abs(g - want) * inside / unit[None, :, None, None]).max()
    assert err <= 16.0, "%s: max error %.3f in units of 2^-24 Vmax (bound 16)" % (what, err)
    assert_padding_is_plus_zero(got, inside, what)
    return err


def images_of(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def test_identity_scale_is_bit_exact():
    import torch
    images, flipped = images_of([(17, 23), (8, 8)], 1), [0, 1]
    out_hw, blob_hw = [(17, 23), (8, 8)], (32, 32)
    outs = run_kernel(images, flipped, [1.0, 1.0], out_hw, blob_hw, NORMS)
    for got, norm in zip(outs, NORMS):
        want = np.zeros((2, 3, 32, 32), np.float32)
        inside = np.zeros(want.shape, bool)
        for n, (im, flip, (h, w)) in enumerate(zip(images, flipped, out_hw)):
            want[n, :, :h, :w] = taps(im[:, ::-1, :] if flip else im, norm).transpose(2, 0, 1)
            inside[n, :, :h, :w] = True
        assert torch.equal(got.cpu(), torch.from_numpy(want))
        assert_padding_is_plus_zero(got, inside, "identity")


RESIZE_CASES = {
    # the shorter side reaches the target in all four (up- and down-scaling, the w = 1 clamp)
    "target_size": ([(37, 53), (64, 48), (5, 7), (1, 1)], [0, 1, 0, 1]),
    # 32 / 20 * 90 = 144 > 48 and 32 / 30 * 75 = 80 > 48: plan_image_blob's max_size branch
    "max_size": ([(20, 90), (75, 30)], [1, 0]),
}


@pytest.fixture(scope="module")
def resized():
    """each case's inputs, kernel outputs for both norms and restatements, computed once"""
    import ssad_amd  # noqa: F401
    from ssad_amd.roi_data.minibatch import plan_image_blob
    cases = {}
    for name, (shapes, flipped) in RESIZE_CASES.items():
        images = images_of(shapes, 2)
        scales, out_hw, minimal = plan_image_blob(shapes, target_size=32, max_size=48)
        blob_hw = (64, 96)
        assert minimal[0] <= blob_hw[0] and minimal[1] <= blob_hw[1]
        outs = run_kernel(images, flipped, scales, out_hw, blob_hw, NORMS)
        refs = [restate(images, flipped, scales, out_hw, blob_hw, norm) for norm in NORMS]
        cases[name] = dict(images=images, flipped=flipped, scales=scales, out_hw=out_hw, blob_hw=blob_hw, outs=outs,
                           refs=refs)
    return cases


@pytest.mark.parametrize("case", sorted(RESIZE_CASES))
def test_resize_matches_the_restatement(resized, case):
    c = resized[case]
    if case == "target_size":
        assert c["scales"] == [32 / 37.0, 32 / 48.0, 32 / 5.0, 32.0]
    else:
        assert c["scales"] == [48 / 90.0, 48 / 75.0]
    for k, norm in enumerate(NORMS):
        want, inside = c["refs"][k]
        err = assert_within_bound(c["outs"][k], want, inside, norm, "%s norm %d" % (case, k))
        print("%s norm %d: max error %.3f x 2^-24 Vmax" % (case, k, err))


def test_one_norm_equals_the_student_blob_of_two(resized):
    import torch
    c = resized["target_size"]
    one, = run_kernel(c["images"], c["flipped"], c["scales"], c["out_hw"], c["blob_hw"], NORMS[:1])
    assert torch.equal(one, c["outs"][0])
    other, = run_kernel(c["images"], c["flipped"], c["scales"], c["out_hw"], c["blob_hw"], NORMS[1:])
    assert torch.equal(other, c["outs"][1])


def test_quad_straddling_the_image_edge():
    """ow % 4 = 1, 2, 3: the four-element store that holds the image's last column selects per element"""
    shapes = [(9, 13), (9, 14), (9, 15)]
    images = images_of(shapes, 3)
    got, = run_kernel(images, [0, 0, 1], [1.0] * 3, shapes, (32, 32), [REF_NORM])
    g = got.cpu().numpy()
    for n, (im, flip, (h, w)) in enumerate(zip(images, [0, 0, 1], shapes)):
        assert np.array_equal(g[n, :, :h, :w], taps(im[:, ::-1, :] if flip else im, REF_NORM).transpose(2, 0, 1))
        assert (g[n, :, :h, :w] != 0).all()                    # u8 - a non-integer mean is never 0
        pad = np.ones((3, 32, 32), bool)
        pad[:, :h, :w] = False
        assert not g[n].view(np.int32)[pad].any()


def test_builder_alternates_slots_and_writes_into_out():
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd.roi_data.minibatch import ImageBlobBuilder, ImageNorm, plan_image_blob
    shapes_a, shapes_b = [(37, 53), (5, 7)], [(20, 90), (64, 48)]
    blob_hw = (64, 96)
    out = torch.full((2, 3) + blob_hw, float("nan"), dtype=torch.float32, device="cuda")
    b = ImageBlobBuilder(2, blob_hw, teacher_norm=ImageNorm(*IMAGENET_NORM), out=out)
    batches = [(images_of(shapes_a, 4), [1, 0]), (images_of(shapes_b, 5), [0, 1]), (images_of(shapes_a, 4), [1, 0])]
    kept = []
    for images, flipped in batches:              # three calls: both slots, then the first one again
        r = b(images, flipped, target_size=32, max_size=48)
        assert r["data"].data_ptr() == out.data_ptr() and r["teacher/data"].data_ptr() == b.teacher_out.data_ptr()
        torch.cuda.current_stream().synchronize()
        assert r["event"].query()
        kept.append((r["data"].clone(), r["teacher/data"].clone(), r["im_scales"], r["im_info"]))
    assert kept[0][0].data_ptr() != kept[1][0].data_ptr()
    for (images, flipped), (data, tdata, scales, info) in zip(batches, kept):
        shapes = [im.shape[:2] for im in images]
        want_s, out_hw, _ = plan_image_blob(shapes, 32, 48)
        assert list(scales) == want_s
        assert np.array_equal(info, np.array([(oh, ow, s) for (oh, ow), s in zip(out_hw, want_s)], np.float32))
        for got, norm in ((data, REF_NORM), (tdata, IMAGENET_NORM)):
            want, inside = restate(images, flipped, want_s, out_hw, blob_hw, norm)
            assert_within_bound(got, want, inside, norm, "builder")
    assert torch.equal(kept[0][0], kept[2][0]) and torch.equal(kept[0][1], kept[2][1])
    assert not torch.equal(kept[0][0], kept[1][0])


def test_builder_refuses_what_does_not_fit():
    import ssad_amd  # noqa: F401
    from ssad_amd import kernels as K
    from ssad_amd.roi_data.minibatch import ImageBlobBuilder
    b = ImageBlobBuilder(1, (32, 32), max_src_bytes=3 * 40 * 40)
    with pytest.raises(K.KernelError, match="does not fit"):
        b(images_of([(33, 8)], 6), [0], im_scales=[1.0])                 # taller than the blob
    with pytest.raises(K.KernelError, match="does not fit"):
        b(images_of([(16, 16)], 6), [0], im_scales=[2.5])                # 40 x 40 after the resize
    with pytest.raises(K.KernelError, match="max_src_bytes"):
        b(images_of([(50, 50)], 6), [0], im_scales=[0.5])
    r = b(images_of([(32, 32)], 6), [0], im_scales=[1.0])                # the builder is still usable
    assert tuple(r["data"].shape) == (1, 3, 32, 32)
