"""Times ssad_image_blobs at BASELINE config 3's input (N = 16 images of 480 x 640 into two 640 x 896 blobs)
against ssad_fill over the same number of output bytes, in one process (profiles/image_blobs.md).

Both kernels store 2 x 16 x 3 x 640 x 896 x 4 B = 220 MB; the new one adds reads of a 15 MB source that
stays cache resident, so their ratio should be near 1.  Timing: HIP events around the call alone, the two
kernels alternating, a warm-up and then the median of --iters calls each.  Also times the 15 MB pinned
host-to-device copy of the pixels.  Prints one JSON line.

    python tools/image_blob_bench.py [--iters 100] [--warmup 5]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_TBS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--source", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--blob", type=int, nargs=2, default=(640, 896))
    args = ap.parse_args()
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd import kernels as K
    from ssad_amd.roi_data.minibatch import REFERENCE_NORM, plan_image_blob
    if not torch.cuda.is_available():
        raise SystemExit("image_blob_bench needs a GPU: nothing is estimated without one")
    L = K.lib()
    N, (h, w), (Hb, Wb) = args.batch, args.source, args.blob
    scales, out_hw, minimal = plan_image_blob([(h, w)] * N, Hb, Wb)
    assert minimal[0] <= Hb and minimal[1] <= Wb, minimal
    rng = np.random.default_rng(0)
    pinned = torch.from_numpy(rng.integers(0, 256, N * h * w * 3, dtype=np.uint8)).pin_memory()
    src = torch.empty(pinned.numel(), dtype=torch.uint8, device="cuda")
    blobs = torch.empty((2, N, 3, Hb, Wb), dtype=torch.float32, device="cuda")
    norms = (K.ImageNorm * 2)()
    imagenet = (255.0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    for k, (div, mean, std) in enumerate((REFERENCE_NORM, imagenet)):
        norms[k] = K.ImageNorm(div, (C.c_float * 3)(*mean), (C.c_float * 3)(*std), blobs[k].data_ptr())
    ws = torch.empty(L.ssad_image_blobs_workspace_bytes(N, Hb, Wb), dtype=torch.uint8, device="cuda")
    ints = lambda v: (C.c_int * N)(*v)
    table = ((C.c_longlong * N)(*[i * h * w * 3 for i in range(N)]), ints([h] * N), ints([w] * N),
             ints([o[0] for o in out_hw]), ints([o[1] for o in out_hw]), (C.c_double * N)(*scales),
             ints([i & 1 for i in range(N)]))

    def image_blobs():
        K._check(L.ssad_image_blobs(src.data_ptr(), src.numel(), *table, N, Hb, Wb, norms, 2, ws.data_ptr(),
                                    ws.numel(), K._stream()), "image_blobs")

    def fill():
        K._check(L.ssad_fill(blobs.data_ptr(), 0.0, blobs.numel(), K._stream()), "fill")

    def upload():
        src.copy_(pinned, non_blocking=True)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    upload()
    for _ in range(args.warmup):
        image_blobs(), fill(), upload()
    torch.cuda.synchronize()
    events = {"image_blobs": [], "fill": [], "h2d": []}
    for _ in range(args.iters):
        events["image_blobs"].append(timed(image_blobs))
        events["fill"].append(timed(fill))
        events["h2d"].append(timed(upload))
    torch.cuda.synchronize()
    ms = {k: float(np.median([a.elapsed_time(b) for a, b in v])) for k, v in events.items()}
    spread = {k: [float(np.min([a.elapsed_time(b) for a, b in v])), float(np.max([a.elapsed_time(b) for a, b in v]))]
              for k, v in events.items()}
    out_bytes = blobs.numel() * 4
    print(json.dumps({
        "shape": {"N": N, "source": [h, w], "resized": list(out_hw[0]), "blob": [Hb, Wb], "norms": 2},
        "iters": args.iters, "out_bytes": out_bytes, "src_bytes": src.numel(),
        "image_blobs_ms": ms["image_blobs"], "fill_ms": ms["fill"], "ratio": ms["image_blobs"] / ms["fill"],
        "image_blobs_write_TBs": out_bytes / ms["image_blobs"] * 1e-9,
        "fill_write_TBs": out_bytes / ms["fill"] * 1e-9,
        "image_blobs_share_of_hbm_peak": out_bytes / ms["image_blobs"] * 1e-9 / HBM_PEAK_TBS,
        "h2d_ms": ms["h2d"], "h2d_GBs": src.numel() / ms["h2d"] * 1e-6, "min_max_ms": spread}))


if __name__ == "__main__":
    main()
