"""Input blobs from uint8 images, the part that needs no GPU: plan_image_blob's host arithmetic against
hand-computed rows, and the launcher's argument validation through the raw library (every rejected call
returns before any launch, so none of the pointers passed here is ever dereferenced)."""
import ctypes

import pytest

import ssad_amd  # noqa: F401
from ssad_amd.caffe2_hip import _capi, dyndep
from ssad_amd.roi_data.minibatch import plan_image_blob

BADARG, WORKSPACE = -1, -2


def test_plan_scales_and_sizes_against_hand_computed_rows():
    # the shorter side reaches the target: 600 / 480 = 1.25, 640 * 1.25 = 800 <= 1000
    scales, out_hw, blob = plan_image_blob([(480, 640)], 600, 1000)
    assert scales == [1.25] and out_hw == [(600, 800)]
    assert blob == (608, 800)                                  # 600 -> 19 * 32, 800 = 25 * 32
    # 600 / 333 * 1000 = 1801.8 > 1000: the longer side is capped, s = 1000 / 1000
    scales, out_hw, blob = plan_image_blob([(333, 1000)], 600, 1000)
    assert scales == [1.0] and out_hw == [(333, 1000)] and blob == (352, 1024)
    # 800 / 375 * 1242 = 2649.6 > 1333: s = 1333 / 1242; 375 s = 402.48 -> 402, 1242 s -> 1333
    scales, out_hw, blob = plan_image_blob([(375, 1242)], 800, 1333)
    assert scales == [1333.0 / 1242.0] and out_hw == [(402, 1333)] and blob == (416, 1344)
    # the issue's example row: 6 / 5 = 1.2 (in double 5 * 1.2 rounds to 6.0, 10 * 1.2 to 12.0: no tie here)
    scales, out_hw, _ = plan_image_blob([(5, 10)], 6, 100)
    assert scales == [1.2] and out_hw == [(6, 12)]


def test_plan_rounds_halves_to_even():
    # s = 3 / 2 = 1.5 exactly (a dyadic scale, so the products below are exact halves):
    # 3 * 1.5 = 4.5 -> 4 (half up would give 5); 5 * 1.5 = 7.5 -> 8; 7 * 1.5 = 10.5 -> 10
    scales, out_hw, blob = plan_image_blob([(2, 3), (2, 5), (2, 7)], 3, 100, coarsest_stride=0)
    assert scales == [1.5, 1.5, 1.5]
    assert out_hw == [(3, 4), (3, 8), (3, 10)]
    assert blob == (3, 10)                                     # stride 0: the largest image, unpadded
    # the max-size test itself uses np.round (half to even): 1.5 * 3 = 4.5 -> 4, not above max_size 4
    assert plan_image_blob([(2, 3)], 3, 4)[0] == [1.5]
    assert plan_image_blob([(2, 3)], 3, 3)[0] == [1.0]


def test_plan_blob_is_the_largest_image_rounded_up_to_the_stride():
    _, out_hw, blob = plan_image_blob([(480, 640), (640, 480), (333, 1000)], 600, 1000)
    assert out_hw == [(600, 800), (800, 600), (333, 1000)]
    assert blob == (800, 1024)
    assert plan_image_blob([(480, 640)], 600, 1000, coarsest_stride=128)[2] == (640, 896)
    with pytest.raises(ValueError):
        plan_image_blob([(0, 4)], 600, 1000)


@pytest.fixture(scope="module")
def raw():
    dyndep.InitOpsLibrary()
    _capi.load()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    from ssad_amd import kernels as K
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    lib.ssad_image_blobs_workspace_bytes.restype = sz
    lib.ssad_image_blobs_workspace_bytes.argtypes = [i32, i32, i32]
    lib.ssad_image_blobs.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32,
                                     ctypes.POINTER(K.ImageNorm), i32, vp, sz, vp]
    return lib


# a consistent call: two images (17 x 23 and 8 x 8, packed back to back) into 32 x 32 blobs at scale 1;
# the addresses are made up (16-byte aligned) and every case below breaks exactly one thing
GOOD = dict(src=0x10000, src_bytes=3 * 17 * 23 + 3 * 8 * 8, offset=[0, 3 * 17 * 23], h=[17, 8], w=[23, 8],
            out_h=[17, 8], out_w=[23, 8], scale=[1.0, 1.0], flipped=[0, 1], N=2, Hb=32, Wb=32, n_norms=2,
            div=[1.0, 255.0], mean=[(0.5, 0.5, 0.5), (0.5, 0.5, 0.5)],
            std=[(1.0, 1.0, 1.0), (0.229, 0.224, 0.225)], out=[0x20000, 0x30000], ws=0x40000, ws_short=0)


def call(raw, **changes):
    from ssad_amd import kernels as K
    a = dict(GOOD)
    a.update(changes)
    n = len(a["h"] if a["h"] is not None else a["w"])

    def arr(ctype, key):
        return None if a[key] is None else (ctype * n)(*a[key])
    norms = None
    if a["out"] is not None:
        norms = (K.ImageNorm * 2)()
        for k in range(2):
            norms[k] = K.ImageNorm(a["div"][k], (ctypes.c_float * 3)(*a["mean"][k]),
                                   (ctypes.c_float * 3)(*a["std"][k]), a["out"][k])
    need = raw.ssad_image_blobs_workspace_bytes(a["N"], a["Hb"], a["Wb"])
    return raw.ssad_image_blobs(
        a["src"], a["src_bytes"], arr(ctypes.c_longlong, "offset"), arr(ctypes.c_int, "h"), arr(ctypes.c_int, "w"),
        arr(ctypes.c_int, "out_h"), arr(ctypes.c_int, "out_w"), arr(ctypes.c_double, "scale"),
        arr(ctypes.c_int, "flipped"), a["N"], a["Hb"], a["Wb"], norms, a["n_norms"], a["ws"],
        (need or 1 << 20) - a["ws_short"], None)


def test_workspace_query(raw):
    need = raw.ssad_image_blobs_workspace_bytes(16, 640, 896)
    # the tap table of both blobs and three words per row and per column of every image
    assert need >= 2 * 3 * 256 * 4 + 16 * (640 + 896) * 12
    assert raw.ssad_image_blobs_workspace_bytes(16, 640, 898) == 0          # Wb % 4
    assert raw.ssad_image_blobs_workspace_bytes(0, 640, 896) == 0
    assert raw.ssad_image_blobs_workspace_bytes(65, 64, 64) == 0            # SSAD_IMAGE_BLOBS_MAX_BATCH = 64
    assert raw.ssad_image_blobs_workspace_bytes(64, 4096, 4096) == 0        # 3.2e9 elements per blob


@pytest.mark.parametrize("what,changes", [
    ("null src", dict(src=None)),
    ("null offsets", dict(offset=None)),
    ("null heights", dict(h=None)),
    ("null widths", dict(w=None)),
    ("null resized heights", dict(out_h=None)),
    ("null resized widths", dict(out_w=None)),
    ("null scales", dict(scale=None)),
    ("null flip flags", dict(flipped=None)),
    ("null norms", dict(out=None)),
    ("null output", dict(out=[0x20000, None])),
    ("null workspace", dict(ws=None)),
    ("empty batch", dict(N=0)),
    ("negative batch", dict(N=-1)),
    ("no norm", dict(n_norms=0)),
    ("three norms", dict(n_norms=3)),
    ("blob width not a multiple of 4", dict(Wb=34)),
    ("source height 0", dict(h=[17, 0])),
    ("source width 0", dict(w=[0, 8])),
    ("resized height beyond the blob", dict(out_h=[33, 8])),
    ("resized width beyond the blob", dict(out_w=[23, 33])),
    ("resized height 0", dict(out_h=[0, 8])),
    ("resized width 0", dict(out_w=[23, 0])),
    ("negative offset", dict(offset=[-1, 3 * 17 * 23])),
    ("last image one byte past the source", dict(src_bytes=3 * 17 * 23 + 3 * 8 * 8 - 1)),
    ("offset past the source", dict(offset=[0, 1 << 40])),
    ("scale 0", dict(scale=[1.0, 0.0])),
    ("negative scale", dict(scale=[-1.0, 1.0])),
    ("infinite scale", dict(scale=[float("inf"), 1.0])),
    ("NaN scale", dict(scale=[1.0, float("nan")])),
    ("div 0", dict(div=[1.0, 0.0])),
    ("a std of 0", dict(std=[(1.0, 0.0, 1.0), (1.0, 1.0, 1.0)])),
    ("output not 16-byte aligned", dict(out=[0x20000, 0x30004])),
    ("workspace not 16-byte aligned", dict(ws=0x40008)),
    ("infinite div", dict(div=[float("inf"), 255.0])),
    ("NaN div", dict(div=[1.0, float("nan")])),
    ("infinite std", dict(std=[(1.0, 1.0, 1.0), (0.229, float("inf"), 0.225)])),
    ("NaN std", dict(std=[(float("nan"), 1.0, 1.0), (1.0, 1.0, 1.0)])),
    ("infinite mean", dict(mean=[(0.5, 0.5, float("-inf")), (0.5, 0.5, 0.5)])),
    ("NaN mean", dict(mean=[(0.5, 0.5, 0.5), (0.5, float("nan"), 0.5)])),
    ("blob of 2^31 elements and more", dict(N=64, Hb=4096, Wb=4096, h=[1] * 64, w=[1] * 64, out_h=[1] * 64,
                                             out_w=[1] * 64, offset=[0] * 64, scale=[1.0] * 64, flipped=[0] * 64)),
    ("batch above the cap", dict(N=65, h=[1] * 65, w=[1] * 65, out_h=[1] * 65, out_w=[1] * 65, offset=[0] * 65,
                                 scale=[1.0] * 65, flipped=[0] * 65)),
])
def test_launcher_rejects_before_launching(raw, what, changes):
    assert call(raw, **changes) == BADARG, what


def test_launcher_reports_a_short_workspace(raw):
    assert call(raw, ws_short=1) == WORKSPACE
