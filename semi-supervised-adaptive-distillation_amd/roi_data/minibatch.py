"""The image half of a minibatch built on the GPU: the device replacement of `_get_image_blob`
(detectron/lib/roi_data/minibatch.py:102-134) with `prep_im_for_blob` / `im_list_to_blob`
(detectron/lib/utils/blob.py:40-106).

The reference normalises, resizes (cv2.resize, INTER_LINEAR) and pads every image on the host, once
for the student and once more for the teacher under `teacher_cfg`'s PIXEL_MEANS / PIXEL_DIV /
PIXEL_STD, and uploads two float blobs.  Here the host uploads the decoded uint8 pixels once and one
`ssad_image_blobs` call (csrc/kernels/image_blobs.hip) writes `data` and `teacher/data`.

cv2 is not installed where this project is built, so bit parity with `cv2.resize` is UNPINNED: the
kernel's definition (include/ssad_kernels.h) is written from cv2's algorithm, and the tests
pin the kernel to that definition, not to cv2."""
import collections
import ctypes as C

import numpy as np
import torch

from .. import kernels as K

ImageNorm = collections.namedtuple("ImageNorm", ["div", "mean", "std"])
# cfg.PIXEL_DIV / PIXEL_MEANS / PIXEL_STD of detectron/lib/core/config.py:929-933 (BGR)
REFERENCE_NORM = ImageNorm(1.0, (102.9801, 115.9465, 122.7717), (1.0, 1.0, 1.0))


def plan_image_blob(shapes, target_size, max_size, coarsest_stride=32):
    """Host arithmetic of prep_im_for_blob (blob.py:92-103) and im_list_to_blob (:50-56) for source
    sizes `shapes` = [(h, w), ...]: returns (im_scales, out_hw, blob_hw).

    im_scales[i] = target_size / min(h, w), or max_size / max(h, w) when the longer side would round
    above max_size; out_hw[i] = (rint(h s), rint(w s)) in double with halves to even, as cv2.resize
    sizes its output for fx = fy = s; blob_hw = the largest of them rounded up to a multiple of
    coarsest_stride (0: no rounding).  Never touches the GPU."""
    im_scales, out_hw = [], []
    for h, w in shapes:
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise ValueError("image of size %d x %d" % (h, w))
        s = float(target_size) / float(min(h, w))
        if np.round(s * max(h, w)) > max_size:
            s = float(max_size) / float(max(h, w))
        im_scales.append(s)
        out_hw.append((int(np.rint(h * s)), int(np.rint(w * s))))
    bh, bw = max(o[0] for o in out_hw), max(o[1] for o in out_hw)
    if coarsest_stride:
        stride = float(coarsest_stride)
        bh, bw = int(np.ceil(bh / stride) * stride), int(np.ceil(bw / stride) * stride)
    return im_scales, out_hw, (bh, bw)


class ImageBlobBuilder(object):
    """Pre-allocates everything once; `__call__` turns one minibatch of decoded images into the two
    input blobs with one upload and one kernel call.

    N, blob_hw     batch size and the blobs' (Hb, Wb); Wb % 4 == 0 (any FPN stride gives that)
    student_norm / teacher_norm   ImageNorm(div, mean[3], std[3]) of `data` / `teacher/data`;
                   None = the reference's default (REFERENCE_NORM)
    max_src_bytes  capacity for the packed uint8 pixels of one batch (default: N images as large as
                   the blob)
    out / teacher_out   float32 [N][3][Hb][Wb] device tensors to write into, e.g. the `image` buffer of
                   the student's and the teacher's NativeResNetFPN, whose forward() then skips its copy

    Two staging slots alternate between calls, each a pinned host buffer, a device source buffer and
    an event: the host may fill the next batch while the previous one is still being copied.  The
    per-image sizes travel as a kernel argument, so the pixels are all that is staged."""

    def __init__(self, N, blob_hw, student_norm=None, teacher_norm=None, max_src_bytes=None, device="cuda",
                 out=None, teacher_out=None):
        self.N, (self.Hb, self.Wb) = int(N), (int(blob_hw[0]), int(blob_hw[1]))
        self.device = torch.device(device)
        L = K.lib()
        nb = L.ssad_image_blobs_workspace_bytes(self.N, self.Hb, self.Wb)
        if nb == 0:
            raise K.KernelError("image_blobs: unsupported shape N %d, blob %d x %d (N <= %d, Wb %% 4 == 0, "
                                "a blob below 2^31 elements)" % (self.N, self.Hb, self.Wb, K.IMAGE_BLOBS_MAX_BATCH))
        shape = (self.N, 3, self.Hb, self.Wb)
        outs = []
        for t, name in ((out, "out"), (teacher_out, "teacher_out")):
            if t is None:
                t = torch.empty(shape, dtype=torch.float32, device=self.device)
            elif tuple(t.shape) != shape or t.device.type != "cuda":
                raise K.KernelError("%s must be a float32 device tensor of shape %s" % (name, shape))
            outs.append(K._f32c(t, name))
        self.out, self.teacher_out = outs
        self.max_src_bytes = int(max_src_bytes) if max_src_bytes is not None else self.N * 3 * self.Hb * self.Wb
        self.ws = torch.empty(int(nb), dtype=torch.uint8, device=self.device)
        self._norms = (K.ImageNorm * 2)()
        for k, (norm, t) in enumerate(((student_norm, self.out), (teacher_norm, self.teacher_out))):
            norm = REFERENCE_NORM if norm is None else norm
            self._norms[k] = K.ImageNorm(float(norm.div), (C.c_float * 3)(*norm.mean), (C.c_float * 3)(*norm.std),
                                         t.data_ptr())
        self._slots = []
        for _ in range(2):
            pinned = torch.empty(self.max_src_bytes, dtype=torch.uint8, pin_memory=True)
            self._slots.append((pinned, pinned.numpy(),
                                torch.empty(self.max_src_bytes, dtype=torch.uint8, device=self.device),
                                torch.cuda.Event()))
        self._next = 0

    def __call__(self, images, flipped, im_scales=None, target_size=None, max_size=None):
        """images: N contiguous np.uint8 [h][w][3] arrays (BGR, as cv2.imread returns them); flipped: N
        flags (roidb[i]['flipped']).  The scales are `im_scales` or, when that is None, those of
        plan_image_blob(shapes, target_size, max_size).

        Returns {"data", "teacher/data"} (device float32 [N][3][Hb][Wb]), "im_scales" (float64 [N]),
        "im_info" (float32 [N][3] = resized height, resized width, scale) and "event", recorded behind
        the kernel: what NativeDistillModel.step(images_event=...) accepts.  im_scales is what the
        caller multiplies ground-truth boxes by before RetinanetLabeler and what RetinanetDetector
        takes as im_scale.

        One scale per image serves both blobs.  The reference draws the teacher's scale index in a
        second np.random.randint call (minibatch.py:77, :108-110), which gives the same scale whenever
        TRAIN.SCALES has one entry, as in every configuration it ships."""
        N = self.N
        if len(images) != N or len(flipped) != N:
            raise K.KernelError("image_blobs: expected %d images and flags" % N)
        for im in images:
            if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or \
                    not im.flags.c_contiguous or im.size == 0:
                raise K.KernelError("image_blobs: images must be contiguous uint8 [h][w][3] arrays")
        shapes = [im.shape[:2] for im in images]
        if im_scales is None:
            if target_size is None or max_size is None:
                raise K.KernelError("image_blobs: give im_scales, or target_size and max_size")
            im_scales = plan_image_blob(shapes, target_size, max_size)[0]
        if len(im_scales) != N:
            raise K.KernelError("image_blobs: expected %d scales" % N)
        scales = np.asarray(im_scales, np.float64)
        out_hw = [(int(np.rint(h * s)), int(np.rint(w * s))) for (h, w), s in zip(shapes, scales)]
        for (oh, ow), (h, w) in zip(out_hw, shapes):
            if oh > self.Hb or ow > self.Wb:
                raise K.KernelError("image_blobs: a %d x %d image resized to %d x %d does not fit the %d x %d blob"
                                    % (h, w, oh, ow, self.Hb, self.Wb))
        sizes = [im.size for im in images]
        total = int(sum(sizes))
        if total > self.max_src_bytes:
            raise K.KernelError("image_blobs: %d source bytes exceed max_src_bytes %d" % (total, self.max_src_bytes))
        pinned, host, src, event = self._slots[self._next]
        self._next ^= 1
        event.synchronize()              # the copy that last read this slot's staging memory has finished
        offsets = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
        for im, off in zip(images, offsets):
            host[off:off + im.size] = im.reshape(-1)
        ints = lambda v: (C.c_int * N)(*[int(x) for x in v])
        with torch.cuda.device(self.device):     # copy, launch and event on the current stream of the builder's device
            src[:total].copy_(pinned[:total], non_blocking=True)
            rc = K.lib().ssad_image_blobs(
                C.c_void_p(src.data_ptr()), C.c_size_t(total), (C.c_longlong * N)(*[int(o) for o in offsets]),
                ints(s[0] for s in shapes), ints(s[1] for s in shapes), ints(o[0] for o in out_hw),
                ints(o[1] for o in out_hw), (C.c_double * N)(*[float(s) for s in scales]),
                ints(bool(f) for f in flipped), N, self.Hb, self.Wb, self._norms, 2,
                C.c_void_p(self.ws.data_ptr()), C.c_size_t(self.ws.numel()), K._stream())
            if rc:
                raise K.KernelError("image_blobs failed (%d)" % rc)
            event.record()
        im_info = np.array([(oh, ow, s) for (oh, ow), s in zip(out_hw, scales)], np.float32)
        return {"data": self.out, "teacher/data": self.teacher_out, "im_scales": scales, "im_info": im_info,
                "event": event}
