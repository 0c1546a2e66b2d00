"""Times SoftmaxFocalLoss forward and backward (csrc/kernels/softmax_focal.hip, C = 81) beside the existing
SigmoidFocalLoss pair (ssad_focal_loss_forward / _backward, C = 80) at config 2's five level shapes (batch 2,
640 x 896), in one process, and writes profiles/softmax_focal.md.

Each of the four calls is ONE multi-level call (all five levels).  Timing: HIP events around one call alone, the four
variants alternating, a warm-up and then the median and spread of --iters calls each.  Bytes moved are computed from
the shapes: what the algorithm has to read and write once (logits / probabilities / gradients as float32, labels as
int32); "floor" is those bytes over the 8 TB/s HBM peak.  Also times GroupSpatialSoftmax with drop_background at the
same shapes with batch 1 (inference).  The fused call (ssad_softmax_focal_loss_fused: loss and dX in one pass, no P) is
timed beside the forward + backward pair it replaces inside a training step; the whole measurement is repeated --rounds
times and the fused call and the pair are compared round by round.  Prints one JSON line.

    python tools/softmax_focal_bench.py [--iters 200] [--warmup 10] [--rounds 3] [--out profiles/softmax_focal.md]"""
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
    ap.add_argument("--rounds", type=int, default=3)
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
    d_fused = [torch.empty_like(x) for x, _ in soft]
    l_fused = torch.empty(len(SHAPES), device="cuda")
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
        ("SoftmaxFocalLoss fused loss + gradient, no P (C = 81)",
         lambda: K.softmax_focal_loss_fused(soft, fg, num_classes=81, out=(l_fused, d_fused), **kw)),
    ]
    f_soft, b_soft = traffic(81, True)
    f_sig, b_sig = traffic(80, False)
    inf_bytes = sum(4 * A * h * w * (81 + 80) for h, w in SHAPES)
    nbytes = [f_soft, f_sig, b_soft, b_sig, inf_bytes, b_soft]      # fused: read X and labels, write dX

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
    rounds = []                                             # per round: medians of forward, backward, fused
    for _ in range(max(args.rounds, 1)):
        this = [[] for _ in variants]
        for _ in range(args.iters):
            evs = [timed(fn) for _, fn in variants]            # alternating, same process
            torch.cuda.synchronize()
            for i, (a, b) in enumerate(evs):
                this[i].append(a.elapsed_time(b))
        for i, t in enumerate(this):
            ms[i].extend(t)
        rounds.append(dict(forward_ms=float(np.median(this[0])), backward_ms=float(np.median(this[2])),
                           fused_ms=float(np.median(this[5]))))
    # the fused call gives the pair's results (same formulas; tests/test_gpu_softmax_step.py holds it to the gate)
    same = all(torch.equal(a, b) for a, b in zip(d_fused, d_soft))
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
                "variants alternating in one process; median (10th - 90th percentile) of %d calls (%d rounds).  Bytes = what "
                "the call must read and write once; floor = bytes / 8 TB/s.\n\n"
                % (args.iters, args.warmup, torch.cuda.get_device_name(0),
                   ", ".join("%dx%d" % s for s in SHAPES), args.iters * max(args.rounds, 1), max(args.rounds, 1)))
        f.write("| call | ms | MB moved | floor ms | time / floor |\n|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %.4f (%.4f - %.4f) | %.1f | %.4f | %.1fx |\n" % (
                r["call"], r["ms_median"], r["ms_p10"], r["ms_p90"], r["mbytes"], r["floor_ms"],
                r["ms_median"] / r["floor_ms"]))
        f.write("\nTime per byte, softmax pair over sigmoid pair: forward %.2fx, backward %.2fx.\n" % (ratio_f, ratio_b))
        f.write("\nFused call against the forward + backward pair, per round of %d alternating calls (medians, ms); "
                "dX bit-identical to the pair's: %s.\n\n" % (args.iters, "yes" if same else "no"))
        f.write("| round | forward | backward | pair | fused | pair / fused |\n|---|---|---|---|---|---|\n")
        for k, r in enumerate(rounds):
            pair = r["forward_ms"] + r["backward_ms"]
            f.write("| %d | %.4f | %.4f | %.4f | %.4f | %.2fx |\n" % (k + 1, r["forward_ms"], r["backward_ms"], pair,
                                                                  r["fused_ms"], pair / r["fused_ms"]))
    print(json.dumps(dict(rows=rows, per_byte_ratio_forward=ratio_f, per_byte_ratio_backward=ratio_b, rounds=rounds,
                          fused_dx_equals_pair=same)))


if __name__ == "__main__":
    main()
