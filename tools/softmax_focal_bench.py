"""Times SoftmaxFocalLoss forward and backward (csrc/kernels/softmax_focal.hip, C = 81) beside the existing
SigmoidFocalLoss pair (ssad_focal_loss_forward / _backward, C = 80) at config 2's five level shapes (batch 2,
640 x 896), in one process, and writes profiles/softmax_focal.md.

Each of the four calls is ONE multi-level call (all five levels).  Timing: HIP events around one call alone, the four
variants alternating, a warm-up and then the median and spread of --iters calls each.  Bytes moved are computed from
the shapes: what the algorithm has to read and write once (logits / probabilities / gradients as float32, labels as
int32); "floor" is those bytes over the 8 TB/s HBM peak.  Also times GroupSpatialSoftmax with drop_background at the
same shapes with batch 1 (inference).  Prints one JSON line.

    python tools/softmax_focal_bench.py [--iters 200] [--warmup 10] [--out profiles/softmax_focal.md]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(80, 112), (40, 56), (20, 28), (10, 14), (5, 7)]
N, A = 2, 9
HBM_BYTES_PER_S = 8.0e12


def traffic(C, has_prob):
    """(forward bytes, backward bytes) of one five-level call"""
    cells = sum(N * A * h * w for h, w in SHAPES)
    logits = 4 * cells * C
    labels = 4 * cells
    fwd = logits + labels + (logits if has_prob else 0)          # read X, labels (+ write P)
    bwd = logits + labels + logits                               # read X or P, labels, write dX
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_focal.md"))
    args = ap.parse_args()
    import torch
    import ssad_amd  # noqa: F401
    from ssad_amd import kernels as K
    if not torch.cuda.is_available():
        raise SystemExit("softmax_focal_bench needs a GPU: nothing is estimated without one")
    rng = np.random.default_rng(0)

    def levels(C):
        out = []
        for h, w in SHAPES:
            x = torch.from_numpy(rng.standard_normal((N, A * C, h, w)).astype(np.float32)).cuda()
            t = np.zeros((N, A, h, w), np.int32)
            u = rng.random(t.shape)
            t[u < 0.05] = rng.integers(1, 81, int((u < 0.05).sum()))
            t[u > 0.95] = -1
            out.append((x, torch.from_numpy(t).cuda()))
        return out

    soft, sig = levels(81), levels(80)
    fg = torch.tensor([1000.0], device="cuda")
    dl = torch.tensor([1.0], device="cuda")
    kw = dict(gamma=2.0, alpha=0.25, scale=0.125)
    probs = [torch.empty_like(x) for x, _ in soft]
    d_soft = [torch.empty_like(x) for x, _ in soft]
    d_sig = [torch.empty_like(x) for x, _ in sig]
    infer = [x[:1].contiguous() for x, _ in soft]
    infer_out = [torch.empty((1, A * 80, h, w), device="cuda") for h, w in SHAPES]
    variants = [
        ("SoftmaxFocalLoss forward (C = 81)",
         lambda: K.softmax_focal_loss_forward(soft, fg, num_classes=81, probs=probs, **kw)),
        ("SigmoidFocalLoss forward (C = 80)", lambda: K.focal_loss_forward(sig, fg, num_classes=80, **kw)),
        ("SoftmaxFocalLoss backward (C = 81)",
         lambda: K.softmax_focal_loss_backward(soft, probs, fg, dl, num_classes=81, out=d_soft, **kw)),
        ("SigmoidFocalLoss backward (C = 80)",
         lambda: K.focal_loss_backward(sig, fg, dl, num_classes=80, out=d_sig, **kw)),
        ("GroupSpatialSoftmax, drop_background, batch 1, five calls",
         lambda: [K.group_spatial_softmax(x, 81, drop_background=True, out=o) for x, o in zip(infer, infer_out)]),
    ]
    f_soft, b_soft = traffic(81, True)
    f_sig, b_sig = traffic(80, False)
    inf_bytes = sum(4 * A * h * w * (81 + 80) for h, w in SHAPES)
    nbytes = [f_soft, f_sig, b_soft, b_sig, inf_bytes]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    for _ in range(args.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in variants]
    for _ in range(args.iters):
        evs = [timed(fn) for _, fn in variants]            # alternating, same process
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(evs):
            ms[i].append(a.elapsed_time(b))
    rows = []
    for (label, _), t, nb in zip(variants, ms, nbytes):
        t = np.sort(np.asarray(t))
        med = float(np.median(t))
        rows.append(dict(call=label, ms_median=med, ms_p10=float(t[len(t) // 10]), ms_p90=float(t[(9 * len(t)) // 10]),
                         mbytes=nb / 1e6, floor_ms=nb / HBM_BYTES_PER_S * 1e3, ns_per_kb=med * 1e6 / (nb / 1e3)))
    ratio_f = rows[0]["ns_per_kb"] / rows[1]["ns_per_kb"]
    ratio_b = rows[2]["ns_per_kb"] / rows[3]["ns_per_kb"]
    with open(args.out, "w") as f:
        f.write("# SoftmaxFocalLoss beside SigmoidFocalLoss\n\n")
        f.write("`python tools/softmax_focal_bench.py --iters %d --warmup %d` on %s; config 2's level shapes "
                "(batch 2, 640 x 896: %s), A = 9, all five levels per call, HIP events around each call, the "
                "variants alternating in one process; median (10th - 90th percentile) of %d calls.  Bytes = what "
                "the call must read and write once; floor = bytes / 8 TB/s.\n\n"
                % (args.iters, args.warmup, torch.cuda.get_device_name(0),
                   ", ".join("%dx%d" % s for s in SHAPES), args.iters))
        f.write("| call | ms | MB moved | floor ms | time / floor |\n|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %.4f (%.4f - %.4f) | %.1f | %.4f | %.1fx |\n" % (
                r["call"], r["ms_median"], r["ms_p10"], r["ms_p90"], r["mbytes"], r["floor_ms"],
                r["ms_median"] / r["floor_ms"]))
        f.write("\nTime per byte, softmax pair over sigmoid pair: forward %.2fx, backward %.2fx.\n" % (ratio_f, ratio_b))
    print(json.dumps(dict(rows=rows, per_byte_ratio_forward=ratio_f, per_byte_ratio_backward=ratio_b)))


if __name__ == "__main__":
    main()
